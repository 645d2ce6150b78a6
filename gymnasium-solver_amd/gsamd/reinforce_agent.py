"""Device REINFORCE agent — the reference's second algorithm (agents/reinforce/reinforce_agent.py:8-88)
on the device path: Monte Carlo targets from the collector (gs_mc_returns_f32) and one large-minibatch
policy-gradient step per batch (gs_pg_update: a row-parallel forward / loss / backward launch and a
step launch; csrc/gs_pg.hip).

It reuses DevicePPOAgent's env, model, checkpoint and schedule plumbing and replaces the update:
  update_phase()        gs_pg_update over the rollout's index stream, mapped through the collector's
                        idx_map (utils/rollout_collector.py:657-669)
  losses_for_batch()    gs_pg_loss: {loss, early_stop_epoch=False}
  epoch_metrics()       the reference's keys: opt/loss/{total,policy,entropy}, opt/policy/entropy,
                        policy_targets_mean / _std, opt/ppo/{kl,approx_kl}, and roll/{return,adv}/norm/*
                        of the field that is the policy target when it is batch-normalised (the
                        reference also records the other field's when its mode is "batch"; that field
                        does not reach the loss and is not normalised here)
Upstream defects handled here and in gsamd.config / gsamd.presets: Bandit-v0.yaml's reinforce variant
names no model_id (mlp_small is taken), REINFORCEConfig has no normalize_advantages (the field exists
here, default "off"), n_envs "auto" is 32.
Out of scope, refused with ValueError before any device work: pixel observations, one-hidden-layer
models, world_size > 1, precision "bf16", dp_mode "global".
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ._lib import GS_NUM_METRICS, M, OPT_FLAGS, PGHparams, RolloutView, check, lib, ptr, stream_handle
from .ppo_agent import DevicePPOAgent, MinibatchIndices
from .rollout import DeviceRolloutCollector
from .samplers import IndexStreamPrefetcher

PG_KEYS = ("opt/loss/total", "opt/loss/policy", "opt/loss/entropy", "opt/policy/entropy", "policy_targets_mean",
           "policy_targets_std", "opt/ppo/kl", "opt/ppo/approx_kl")


def pg_records(rows: np.ndarray) -> np.ndarray:
    """Records -> the columns of PG_KEYS (+ the two norm columns; opt/loss/entropy = -entropy)."""
    rows = np.asarray(rows, np.float32).reshape(-1, GS_NUM_METRICS)
    return np.stack([rows[:, M["loss"]], rows[:, M["policy_loss"]], -rows[:, M["entropy"]], rows[:, M["entropy"]],
                     rows[:, M["pg_target_mean"]], rows[:, M["pg_target_std"]], rows[:, M["kl"]],
                     rows[:, M["approx_kl"]], rows[:, M["adv_norm_mean"]], rows[:, M["adv_norm_std"]]], axis=1)


class DeviceREINFORCEAgent(DevicePPOAgent):
    HP_KEYS = ("n_epochs", "ent_coef", "policy_lr")

    def __init__(self, config, env=None, device=None, rank: int = 0, world_size: int = 1, comm=None, **kwargs):
        self._check_scope(config, world_size, comm)
        super().__init__(config, env=env, device=device, rank=rank, world_size=world_size, comm=comm, **kwargs)

    @staticmethod
    def _check_scope(c, world_size, comm) -> None:
        if str(getattr(c, "obs_type", "vector")) == "rgb":
            raise ValueError("REINFORCE on the device serves vector observations (MLP policies): pixel observations "
                             "are not supported")
        if len(tuple(c.hidden_dims)) != 2:
            raise ValueError(f"model_id {c.model_id!r}: the REINFORCE update serves two hidden layers, a policy with "
                             "one hidden layer is not supported")
        if c.valid_actions is not None:
            raise ValueError(f"action_space.valid {list(c.valid_actions)}: the REINFORCE update has no masked head "
                             "(the masked MLP policy trains with algo_id 'ppo')")
        if int(world_size) > 1 or comm:
            raise ValueError(f"the REINFORCE update has no gradient exchange: world_size={world_size} is not "
                             "supported (use one GPU)")
        if str(getattr(c, "precision", "fp32")) == "bf16":
            raise ValueError("the REINFORCE update is fp32 only: precision 'bf16' is a mode of the PPO chain")
        if str(getattr(c, "dp_mode", "local")) == "global":
            raise ValueError("dp_mode 'global' is a mode of the multi-GPU PPO update: REINFORCE runs on one GPU")

    # ---- collectors ---------------------------------------------------------------------------
    def _collector(self, stage: str, seed: int, **kw) -> DeviceRolloutCollector:
        c = self.config
        ck = c.get_rollout_collector_kwargs()
        return DeviceRolloutCollector(self.get_env(stage), self.policy_model, c.n_steps, gamma=c.gamma,
                                      gae_lambda=c.gae_lambda, rng_seed=seed, returns_type=ck["returns_type"],
                                      advantages_type=ck["advantages_type"], normalize_returns=ck["normalize_returns"],
                                      normalize_advantages=ck["normalize_advantages"], **kw)

    def build_rollout_collector(self, stage: str):
        self._rollout_collectors[stage] = self._collector(
            stage, self.config.seed + 7919 * self.rank, track_stats=self.track_stats, use_graph=self.use_graph,
            one_launch=self.one_launch)

    def get_rollout_collector(self, stage: str) -> DeviceRolloutCollector:
        if stage not in self._rollout_collectors and stage in ("val", "test"):
            self.build_env(stage)
            self._rollout_collectors[stage] = self._collector(stage, self.config.seed + 1000 + 7919 * self.rank,
                                                              track_stats=True)
        return self._rollout_collectors[stage]

    # ---- optimizer state ----------------------------------------------------------------------
    def configure_optimizers(self):
        """Adam / AdamW / SGD(params, lr=policy_lr) by config.optimizer, state in HBM.  The loss never
        touches the value head: its .grad stays None in the reference, so clip_grad_norm_ and the
        optimizer skip it — its moments stay zero here, and AdamW does not decay it."""
        c = self.config
        P = self.policy_model.n_params
        z = dict(dtype=torch.float32, device=self.device)
        self.grads, self.adam_m, self.adam_v = torch.zeros(P, **z), torch.zeros(P, **z), torch.zeros(P, **z)
        self.adam_step = 0
        self.batch_size = int(c.batch_size)
        self.data_len = c.n_envs * c.n_steps
        if self.data_len % self.batch_size != 0:
            raise ValueError(f"Batch size must divide rollout size exactly: data_len={self.data_len}, "
                             f"batch_size={self.batch_size}.")
        self.n_minibatches = self.data_len // self.batch_size * c.n_epochs
        self.global_mode = False
        self._base_seed = int(torch.initial_seed())
        self.workspace = self._workspace(self.batch_size)
        self.stop_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.metrics_buf = torch.zeros(self.n_minibatches, GS_NUM_METRICS, **z)
        self._step_metrics = torch.zeros(GS_NUM_METRICS, **z)
        self.prefetcher = IndexStreamPrefetcher(self.data_len, c.n_epochs, self._base_seed, self.device)
        return None

    def _workspace(self, batch: int) -> torch.Tensor:
        nb = int(lib.gs_pg_update_workspace_bytes(self.policy_model.dims, int(batch)))
        if nb == 0:
            raise ValueError(f"the REINFORCE update does not serve this policy shape or batch size ({batch}): "
                             "two hidden layers of at most 512 units, obs_dim <= 64, n_actions <= 32, batch in [2, 2^20]")
        return torch.zeros(nb, dtype=torch.uint8, device=self.device)

    BASELINE_FILE = "mc_baseline.json"

    def save_checkpoint(self, checkpoint_dir) -> None:
        """The parent's files plus mc_baseline.json, the collector's running baseline (count, sum,
        sum_squared).  optimizer.pt keeps torch.optim.Adam's layout with one entry per tensor: the
        value head's two entries carry zero moments, where torch would write no state at all (a
        parameter whose .grad is None never gets one)."""
        import json
        from pathlib import Path
        super().save_checkpoint(checkpoint_dir)
        base = dict(self.get_rollout_collector("train")._base_stats)
        (Path(checkpoint_dir) / self.BASELINE_FILE).write_text(json.dumps(base))

    def load_checkpoint(self, checkpoint_dir, resume_training: bool = True, strict: bool = True) -> None:
        import json
        from pathlib import Path
        super().load_checkpoint(checkpoint_dir, resume_training=resume_training, strict=strict)
        f = Path(checkpoint_dir) / self.BASELINE_FILE
        if resume_training and f.exists():
            b = json.loads(f.read_text())
            self.get_rollout_collector("train")._base_stats = {
                "count": int(b["count"]), "sum": float(b["sum"]), "sum_squared": float(b["sum_squared"])}

    # ---- the update ---------------------------------------------------------------------------
    @property
    def device_activation_stats(self) -> bool:
        return False            # the REINFORCE update records no activation statistics

    def activation_keys(self):
        return ()

    @property
    def targets_field(self) -> str:
        return "returns" if self.config.policy_targets == "returns" else "advantages"

    @property
    def normalize_targets(self) -> bool:
        """The policy target's own mode is "batch" (reinforce_agent.py:22-36)."""
        c = self.config
        mode = c.normalize_returns if self.targets_field == "returns" else c.normalize_advantages
        return mode == "batch"

    def hparams(self) -> PGHparams:
        c = self.config
        return PGHparams(float(self.ent_coef), float(c.max_grad_norm if c.max_grad_norm is not None else 0.0),
                         float(self.policy_lr), 0.9, 0.999, 1e-8, 1 if self.normalize_targets else 0,
                         OPT_FLAGS[self.optimizer_name])

    def _rollout_view(self, buf) -> RolloutView:
        """The update's view: `advantages` carries the policy targets (returns or advantages)."""
        return RolloutView(ptr(buf.obs), ptr(buf.actions), ptr(buf.logprobs), None,
                           ptr(getattr(buf, self.targets_field)), None, buf.T, buf.N)

    def _mapped(self, idx: torch.Tensor) -> torch.Tensor:
        """Every sampled index -> its nearest earlier valid position (rollout_collector.py:657-669)."""
        imap = self.get_rollout_collector("train").idx_map
        return idx if imap is None else imap[idx.long()].contiguous()

    def _epoch_batches(self, epoch: int):
        idx = self._mapped(self.prefetcher.upload(epoch))
        self.prefetcher.prefetch(epoch + 1)
        B = self.batch_size
        return [MinibatchIndices(idx[k * B:(k + 1) * B], self._trajectories) for k in range(self.n_minibatches)]

    def _stage_batch(self, batch):
        """A tensor batch -> a one-step rollout of B envs whose `advantages` are the policy targets."""
        obs = torch.as_tensor(batch.observations)
        B = int(obs.shape[0])
        st = self._staged
        if st is None or st["B"] != B:
            dev = self.device
            st = {"B": B, "idx": torch.arange(B, dtype=torch.int32, device=dev),
                  "obs": torch.empty((1, *obs.shape), dtype=torch.float32, device=dev),
                  "act": torch.empty(1, B, dtype=torch.int64, device=dev),
                  "lp": torch.empty(1, B, dtype=torch.float32, device=dev),
                  "t": torch.empty(1, B, dtype=torch.float32, device=dev)}
            st["ws"] = self.workspace if B == self.batch_size else self._workspace(B)
            self._staged = st
        st["obs"][0].copy_(obs.to(torch.float32).reshape(st["obs"].shape[1:]))
        st["act"][0].copy_(torch.as_tensor(batch.actions).reshape(B).to(torch.int64))
        st["lp"][0].copy_(torch.as_tensor(batch.logprobs).reshape(B).to(torch.float32))
        st["t"][0].copy_(torch.as_tensor(getattr(batch, self.targets_field)).reshape(B).to(torch.float32))
        view = RolloutView(ptr(st["obs"]), ptr(st["act"]), ptr(st["lp"]), None, ptr(st["t"]), None, 1, B)
        return view, st["idx"], B, st["ws"]

    def _batch_view(self, batch):
        if isinstance(batch, MinibatchIndices):
            buf = self.get_rollout_collector("train").buffer
            return self._rollout_view(buf), batch.idx, len(batch), self.workspace
        return self._stage_batch(batch)

    def metric_keys(self):
        keys = PG_KEYS
        if self.normalize_targets:
            prefix = "roll/return" if self.targets_field == "returns" else "roll/adv"
            keys = keys + (f"{prefix}/norm/mean", f"{prefix}/norm/std")
        return keys

    def _record_step(self, rec: torch.Tensor) -> np.ndarray:
        row = rec.detach().cpu().numpy().reshape(1, GS_NUM_METRICS)
        keys = self.metric_keys()
        self.metrics_recorder.record("train", dict(zip(keys, pg_records(row)[0, :len(keys)].tolist())))
        return row[0]

    def losses_for_batch(self, batch, batch_idx: int):
        """REINFORCEAgent.losses_for_batch (reinforce_agent.py:11-88): forward + loss + metrics of one
        minibatch (and its gradient, into self.grads), no optimizer step."""
        view, idx, B, ws = self._batch_view(batch)
        check(lib.gs_pg_loss(ptr(self.policy_model.params), ptr(self.grads), self.policy_model.dims, self.hparams(),
                             view, ptr(idx), B, ptr(self._step_metrics), ptr(ws), ws.numel(), stream_handle()),
              "gs_pg_loss")
        self._record_step(self._step_metrics)
        return dict(loss=self._step_metrics[M["loss"]].clone(), early_stop_epoch=False)

    def training_step(self, batch, batch_idx: int):
        view, idx, B, ws = self._batch_view(batch)
        rec = self.metrics_buf[batch_idx % self.n_minibatches]
        check(lib.gs_pg_update(ptr(self.policy_model.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                               self.policy_model.dims, self.hparams(), view, ptr(idx), B, 1, self.adam_step, ptr(rec),
                               ptr(ws), ws.numel(), None, stream_handle()), "gs_pg_update")
        self.adam_step += 1
        row = self._record_step(rec)
        keys, slots = self.grad_norm_keys()
        self.metrics_recorder.record("train", {k: float(row[j]) for k, j in zip(keys, slots)})
        return None

    def update_phase(self, ev=None) -> None:
        """The update half of an epoch: the n_epochs passes over the rollout as one gs_pg_update call
        (two launches per optimizer step), then the epoch's bookkeeping."""
        self._epoch_hp = self.hyperparameter_record()
        epoch = self.current_epoch
        collector = self.get_rollout_collector("train")
        idx = self._mapped(self.prefetcher.upload(epoch))
        self.prefetcher.prefetch(epoch + 1)
        if ev:
            ev[-1][1].record()
        check(lib.gs_pg_update(ptr(self.policy_model.params), ptr(self.grads), ptr(self.adam_m), ptr(self.adam_v),
                               self.policy_model.dims, self.hparams(), self._rollout_view(collector.buffer), ptr(idx),
                               self.batch_size, self.n_minibatches, self.adam_step, ptr(self.metrics_buf),
                               ptr(self.workspace), self.workspace.numel(), None, stream_handle()), "gs_pg_update")
        if ev:
            ev[-1][2].record()
        self.adam_step += self.n_minibatches
        self.current_epoch += 1
        self.on_train_epoch_end()

    def record_epoch_metrics(self) -> np.ndarray:
        rec = self.metrics_buf.cpu().numpy()
        keys = self.metric_keys()
        self.metrics_recorder.record_rows("train", keys, pg_records(rec)[:, :len(keys)])
        if getattr(self, "_epoch_hp", None):
            self.metrics_recorder.record("train", self._epoch_hp)
        gkeys, slots = self.grad_norm_keys()
        self.metrics_recorder.record_rows("train", gkeys, rec[:, slots])
        return rec

    def epoch_metric_keys(self):
        hp = tuple(f"hp/{k}" for k in self.HP_KEYS if getattr(self, k, None) is not None)
        return tuple(self.metric_keys()) + self.grad_norm_keys()[0] + hp

    def epoch_metrics(self) -> Dict[str, float]:
        self.metrics_recorder.reset_epoch("train")
        self.record_epoch_metrics()
        return {k: float(v) for k, v in self.metrics_recorder.compute_epoch_means("train").items()}
