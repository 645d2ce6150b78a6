"""Generate the REINFORCE fixtures FROM THE REFERENCE ITSELF (build container only; see make_golden.py
for the import stubs this reuses).  Writes next to this script:

  reinforce.npz          * Monte Carlo targets: compute_batched_mc_returns, convert_returns_to_full_episode
                           and _build_valid_mask_and_index_map (utils/returns_advantages.py:19-113) on
                           (T, N) in {(1, 1), (5, 3), (64, 37)} x gamma in {1.0, 0.99, 0.98} x both kinds x
                           both timeout settings (the zero mask the collector passes by default, and a
                           0/1 mask), with the reference KAT [3, 2, 7, 4]
                         * the collector's mc:* branch (RolloutCollector._compute_targets) over three
                           rollouts: the running baseline, advantages, the rollout normalisations
                         * REINFORCEAgent.losses_for_batch + backward + clip_grad_norm_(0.5) + Adam(1e-3)
                           over three minibatches for the cases of tests/reinforce_twin.loss_cases():
                           the first minibatch's record, gradient norms, sampled gradient entries, and
                           sampled parameters after the three steps
  config_reinforce.json  every field the reference resolves for Bandit-v0:reinforce

Upstream defects this generator has to step around (each recorded in the json):
  1. Bandit-v0.yaml's reinforce variant has no model_id: load_config asserts (utils/config.py:463).
     The record is taken with _resolve_policy skipped, so model_id stays null.
  2. REINFORCEConfig has no normalize_advantages: base_agent.py:117 raises AttributeError on the first
     minibatch.  The agent here gets a config namespace that carries the field.
  3. n_envs "auto" resolves to the host's core count (and below 32 cores the reference then refuses
     batch_size 2048): resolved as on a 32-core host, kept as "auto" in the record.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (reference on sys.path, third-party stubs, torch)
import torch  # noqa: E402

sys.path.insert(0, os.path.join(HERE, ".."))
import reinforce_twin as tw  # noqa: E402  (case list and deterministic inputs shared with the tests)

from agents.reinforce.reinforce_agent import REINFORCEAgent  # noqa: E402
from utils.models import MLPActorCritic  # noqa: E402
from utils.returns_advantages import (_build_valid_mask_and_index_map, compute_batched_mc_returns,  # noqa: E402
                                      convert_returns_to_full_episode)
from utils.rollout_collector import RolloutCollector  # noqa: E402

RETURN_SHAPES = ((1, 1), (5, 3), (64, 37))
GAMMAS = (1.0, 0.99, 0.98)


def _dones(rng, T, N):
    """10 % dones with forced columns: no terminal in env 0 and in two adjacent later envs, a
    terminal only at t = 0, a terminal at t = T - 1 (as far as N has the envs)."""
    d = rng.random((T, N)) < 0.1
    d[:, 0] = False
    if N >= 3:
        d[:, 1] = False
        d[0, 1] = True
        d[T - 1, 2] = True
    if N >= 16:
        d[:, 10:12] = False
    return d


def make_returns(out):
    rng = np.random.default_rng(20260)
    for T, N in RETURN_SHAPES:
        tag = f"ret/{T}x{N}"
        rew = rng.normal(size=(T, N)).astype(np.float32)
        dones = _dones(rng, T, N)
        mask = dones & (rng.random((T, N)) < 0.5)
        out[f"{tag}/rewards"], out[f"{tag}/dones"], out[f"{tag}/timeouts"] = rew, dones.astype(np.uint8), mask.astype(np.uint8)
        for to_name, to in (("default", np.zeros_like(dones)), ("mask", mask)):
            valid, idx_map = _build_valid_mask_and_index_map(dones, to)
            real = dones & ~to
            last = np.array([np.flatnonzero(real[:, j])[-1] if real[:, j].any() else -1 for j in range(N)], np.int32)
            out[f"{tag}/{to_name}/last_terminal"] = last
            out[f"{tag}/{to_name}/has_map"] = np.array(idx_map is not None)
            out[f"{tag}/{to_name}/idx_map"] = (np.arange(N * T) if idx_map is None else idx_map).astype(np.int32)
            out[f"{tag}/{to_name}/valid"] = (np.zeros(N * T, bool) if valid is None else valid)
            for g in GAMMAS:
                rtg = compute_batched_mc_returns(rew, dones, to, g)
                epi = convert_returns_to_full_episode(rtg.copy(), dones, to)
                assert rtg.dtype == np.float32 and epi.dtype == np.float32
                out[f"{tag}/{to_name}/g{g}/rtg"], out[f"{tag}/{to_name}/g{g}/episode"] = rtg, epi
        if (T, N) == (64, 37):
            free = int((~dones.any(axis=0)).sum())
            share = float(out[f"{tag}/default/valid"].mean())
            assert free == 3, free
            print(f"(64, 37): {free} terminal-free envs, valid share {share:.3f}")
    # the reference's known-answer test: rewards 1, 1, 1 | 2, 2 with terminals after each -> [3, 2, 1 ...]
    kat = compute_batched_mc_returns(np.array([[1.0], [2.0], [3.0], [4.0]], np.float32),
                                     np.array([[0], [1], [0], [1]], bool), np.zeros((4, 1), bool), 1.0)
    out["ret/kat"] = kat
    assert kat[:, 0].tolist() == [3.0, 2.0, 7.0, 4.0], kat


def make_collector_targets(out):
    """RolloutCollector._compute_targets on three recorded rollouts per setting (the buffer filled by
    hand): the running baseline carries over."""
    rng = np.random.default_rng(20261)
    T, N = 16, 5
    rolls = []
    for _ in range(3):
        rolls.append((rng.normal(size=(T, N)).astype(np.float32) + 1.0, _dones(rng, T, N)))
    for r, (rew, dones) in enumerate(rolls):
        out[f"coll/rewards{r}"], out[f"coll/dones{r}"] = rew, dones.astype(np.uint8)
    for tag, kw in {"rtg": dict(returns_type="mc:rtg"), "episode": dict(returns_type="mc:episode"),
                    "rtg_norm": dict(returns_type="mc:rtg", normalize_returns=True, normalize_advantages=True)}.items():
        coll = object.__new__(RolloutCollector)
        coll.returns_type, coll.advantages_type = kw["returns_type"], "baseline"
        coll.normalize_returns = kw.get("normalize_returns", False)
        coll.normalize_advantages = kw.get("normalize_advantages", False)
        coll.mc_treat_timeouts_as_terminals = True
        coll.gamma, coll.gae_lambda = 0.99, 0.95
        from utils.rollout_stats import RunningStats
        for n in ("_base_stats", "_adv_stats", "_adv_norm_stats", "_ret_stats"):
            setattr(coll, n, RunningStats())
        for r, (rew, dones) in enumerate(rolls):
            coll._buffer = types.SimpleNamespace(values_buf=np.zeros((T, N), np.float32), rewards_buf=rew, dones_buf=dones,
                                                 timeouts_buf=np.zeros((T, N), bool),
                                                 bootstrapped_values_buf=np.zeros((T, N), np.float32))
            adv, ret = coll._compute_targets(0, T, None)
            out[f"coll/{tag}/adv{r}"], out[f"coll/{tag}/ret{r}"] = adv.astype(np.float32), ret.astype(np.float32)
            out[f"coll/{tag}/baseline{r}"] = np.array([coll._base_stats.count, coll._base_stats.sum,
                                                       coll._base_stats.sum_squared, coll._base_stats.mean(),
                                                       coll._base_stats.std()], np.float64)
            im = coll._last_rollout_index_map
            out[f"coll/{tag}/idx_map{r}"] = (np.arange(N * T) if im is None else im).astype(np.int32)


def _set_params(model, flat):
    o = 0
    with torch.no_grad():
        for name, p in model.named_parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(flat[o:o + n]).reshape(p.shape))
            o += n
    assert o == flat.size and tuple(n for n, _ in model.named_parameters()) == tw.PARAM_NAMES


def _flat(model, grads=False):
    return np.concatenate([(torch.zeros_like(p) if grads and p.grad is None else (p.grad if grads else p)).detach()
                           .reshape(-1).numpy() for p in model.parameters()])


def make_pools(out):
    rng = np.random.default_rng(20262)
    pools = {}
    for name, (D, A) in {"d4a2": (4, 2), "d10a10": (10, 10)}.items():
        T, N = tw.POOL_T, tw.POOL_N
        rew = rng.normal(size=(T, N)).astype(np.float32) + 0.5
        dones = rng.random((T, N)) < 0.1
        pool = dict(obs=rng.normal(size=(T, N, D)).astype(np.float32),          # random normal, not zeros
                    actions=rng.integers(0, A, size=(T, N)).astype(np.int64),
                    logprobs=(np.log(1.0 / A) + 0.1 * rng.normal(size=(T, N))).astype(np.float32),
                    returns=compute_batched_mc_returns(rew, dones, np.zeros_like(dones), 0.99),
                    perms=np.stack([rng.permutation(T * N) for _ in range(3)]).astype(np.int32))
        pools[name] = pool
        for k, v in pool.items():
            out[f"pool/{name}/{k}"] = v
    return pools


def make_loss(out, pools):
    for tag, shape, B, norm, ent in tw.loss_cases():
        D, H1, H2, A = tw.LOSS_SHAPES[shape]
        pool = pools[tw.POOLS[shape]]
        model = MLPActorCritic(input_shape=(D,), hidden_dims=(H1, H2), output_shape=(A,), activation="relu")
        P = tw.n_params(D, H1, H2, A)
        _set_params(model, tw.hash_params(P))
        agent = object.__new__(REINFORCEAgent)
        torch.nn.Module.__init__(agent)
        # defect 2: the namespace carries normalize_advantages, which REINFORCEConfig lacks
        agent.config = types.SimpleNamespace(normalize_returns="batch" if norm else "off", normalize_advantages="off",
                                             policy_targets="returns")
        agent.ent_coef = ent
        agent.policy_model = model
        recs = []
        agent.metrics_recorder = types.SimpleNamespace(record=lambda ns, d: recs.append(dict(d)))
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        pos = tw.sample_positions(P)
        for step in range(3):
            o, a, lp, t = tw.batch_rows(pool, pool["perms"][step], B)
            batch = types.SimpleNamespace(observations=torch.from_numpy(o), actions=torch.from_numpy(a),
                                          logprobs=torch.from_numpy(lp), returns=torch.from_numpy(t),
                                          advantages=torch.from_numpy(t) - 0.25)
            opt.zero_grad(set_to_none=True)
            res = agent.losses_for_batch(batch, step)
            assert res["early_stop_epoch"] is False
            res["loss"].backward()
            assert model.value_head.weight.grad is None and model.value_head.bias.grad is None
            if step == 0:
                g = _flat(model, grads=True)
                gn = model.compute_grad_norms()
                m = {k: float(v) for k, v in recs[0].items()}
                out[f"loss/{tag}/loss"] = np.float32(res["loss"].item())
                out[f"loss/{tag}/metric_names"] = np.array(sorted(m))
                out[f"loss/{tag}/metric_values"] = np.array([m[k] for k in sorted(m)], np.float64)
                out[f"loss/{tag}/grad_norm_names"] = np.array(sorted(gn))
                out[f"loss/{tag}/grad_norm_values"] = np.array([gn[k] for k in sorted(gn)], np.float64)
                out[f"loss/{tag}/grad_sample"] = g[pos]
                out[f"loss/{tag}/grad_absmax"] = np.float32(np.abs(g).max())
                out[f"loss/{tag}/tensor_norms"] = np.array(
                    [0.0 if p.grad is None else float(p.grad.double().norm()) for p in model.parameters()], np.float64)
            total = torch.nn.utils.clip_grad_norm_(model.parameters(), 0.5)
            if step == 0:
                out[f"loss/{tag}/total_norm"] = np.float32(total.item())
            opt.step()
        p3 = _flat(model)
        out[f"loss/{tag}/params3_sample"] = p3[pos]
        nv = H2 + 1
        assert np.array_equal(p3[-nv:], tw.hash_params(P)[-nv:])      # the value head never moves
        assert all(len(opt.state[p]) == 0 for p in (model.value_head.weight, model.value_head.bias))


def make_config():
    import dataclasses
    from utils.config import REINFORCEConfig
    rec = {}
    try:
        G.load_config("Bandit-v0", "reinforce")
        rec["_reference_load_config"] = "ok"
    except AssertionError as e:
        rec["_reference_load_config"] = f"AssertionError: {str(e)[:60]}"      # defect 1
    keep = REINFORCEConfig._resolve_policy

    def _skip_without_model(self):
        if self.model_id is not None:
            keep(self)
    REINFORCEConfig._resolve_policy = _skip_without_model
    # defect 3: "auto" is the host's core count, and the reference refuses batch_size 2048 on a host
    # with fewer than 32 cores (n_envs * 64 < 2048): resolved as on a 32-core host, the presets' count
    cores, os.cpu_count = os.cpu_count, (lambda: 32)
    try:
        c = G.load_config("Bandit-v0", "reinforce")
    finally:
        REINFORCEConfig._resolve_policy = keep
        os.cpu_count = cores
    d = {k: getattr(v, "value", v) for k, v in dataclasses.asdict(c).items()}
    d["algo_id"] = c.algo_id
    assert d["n_envs"] == 32
    d["n_envs"] = "auto"                                                       # defect 3
    d.update({k: v for k, v in vars(c).items() if "_schedule" in k and not k.startswith("_")})
    d["_has_normalize_advantages"] = hasattr(c, "normalize_advantages")         # defect 2
    d["_n_actions"] = c.spec.get("action_space", {}).get("discrete")
    rec["Bandit-v0:reinforce"] = json.loads(json.dumps(d, default=lambda o: getattr(o, "value", str(o))))
    with open(os.path.join(HERE, "config_reinforce.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("config_reinforce.json written")


if __name__ == "__main__":
    torch.manual_seed(0)
    out = {}
    make_returns(out)
    make_collector_targets(out)
    make_loss(out, make_pools(out))
    path = os.path.join(HERE, "reinforce.npz")
    np.savez_compressed(path, **out)
    print("reinforce.npz written:", len(out), "arrays,", os.path.getsize(path), "bytes")
    make_config()
