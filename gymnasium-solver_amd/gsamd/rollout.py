"""Device-resident rollout: SoA buffer in HBM, fused policy-act kernels, GAE scan.

Mirrors the reference's RolloutBuffer (utils/rollout_buffer.py:28-173) and
RolloutCollector (utils/rollout_collector.py:22-777) for the PPO path
(returns_type "gae:rtg", advantages_type "gae"):

  * buffers are allocated once, time-major ``(T, N, ...)`` like the reference's numpy
    buffers, but in HBM; a rollout never copies them to the host;
  * per step: ``gs_policy_act`` (MLP forward + categorical sample + log_prob, writes
    the step's obs/action/logp/value rows) then the env step;  with the device
    synthetic env (``env.device_native``) the env step is a kernel writing the
    reward/done/timeout rows, so the whole rollout is stream-ordered kernels;  a host
    gymnasium-style env goes through one H2D/D2H per step as in the reference;
  * last-obs value + ``gs_gae_f32`` produce advantages/returns in place;
  * ``bootstrapped_values`` stays all-zero: with gymnasium 1.x vector envs the
    reference never receives ``final_observation``, so its
    ``bootstrapped_values_buf`` is never written yet IS read at timeouts; this
    reproduces that behaviour (pass ``bootstrap_timeouts=True`` to opt out is future work).

The returned trajectory keeps the reference's field names; env-major ``(N*T, ...)``
views (utils/rollout_buffer.py:105-173) are materialised only when accessed — the
device update reads the time-major buffers directly through sampler indices.
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional

import numpy as np
import torch

from ._lib import (GS_BANDIT_MAX_ARMS, GS_ENCODINGS, GS_ENV_ACROBOT, GS_ENV_BANDIT, GS_ENV_CARTPOLE,
                   GS_ENV_MOUNTAINCAR, GS_MC_BONUS_TYPES, GS_MC_WRAP_BONUS, GS_MC_WRAP_NONE, GS_MC_WRAP_SHAPER,
                   BanditSpec, CartPoleWrappers, MountainCarWrappers, TabularSpec, check, lib, ptr, stream_handle)
from .atari_env import DeviceAtariVecEnv
from .config import (TABULAR_KINDS, bandit_arms, device_env_kind, resolve_bandit_env, resolve_cartpole_wrappers,
                     resolve_mountaincar_wrappers, resolve_tabular_env)
from .distributed import allreduce_sum_f64
from .rollout_stats import RollingWindow

BANDIT_MAX_TRAINABLE_ARMS = 15      # see DeviceBanditVecEnv.from_config: what the MLP update's forward staging covers


def _is_pixel(c) -> bool:
    return str(getattr(c, "obs_type", "vector")) == "rgb"


class DeviceVecEnv:
    """What the device env classes share: the tensors every env kernel takes (meta, the running
    return, the observation, the three finished-episode counters) and the four calls into the
    library: reset(), step_into(), rollout_into() and rollout1_into().  An env class adds its own
    tensors and parameters, names its entries, and states once, in _env_args(), the argument group
    every one of them takes (include/gsamd.h: `state, meta, ep_ret, obs, ...`); each call's list is
    formed here from that group.  An entry is looked up on this module's `lib` when it is called."""

    device_native = True
    entry_stem = None            # "<x>": reset() calls gs_<x>_reset, step_into() gs_<x>_step
    rollout_entry = None         # the gs_rollout_* entry (two hidden layers) behind rollout_into(), or None
    rollout1_entry = None        # the gs_rollout1_* entry (one hidden layer) behind rollout1_into(), or None
    env_kind = None              # GS_ENV_*: what gs_rollout_env / gs_rollout1_env and gs_rollout_env_supported take
    # One-launch rollouts (two hidden layers) are the default only up to this many envs.  None = always.
    one_launch_max_envs = None
    needs_actions = "the env needs the step's actions"       # step_into()'s refusal without them

    def _alloc(self, n_envs, obs_dim, n_actions, seed, env_offset, device, meta=True):
        self.num_envs, self.obs_dim, self.n_actions = int(n_envs), int(obs_dim), int(n_actions)
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.obs_shape, self.obs_dtype = (self.obs_dim,), torch.float32
        self.device = torch.device(device)
        N, z = self.num_envs, dict(device=self.device)
        if meta:
            self.meta = torch.zeros(N, 3, dtype=torch.int32, **z)         # steps, episodes, pending
        self.ep_ret = torch.zeros(N, dtype=torch.float32, **z)
        self.obs = torch.zeros(N, self.obs_dim, dtype=torch.float32, **z)
        self.ep_count = torch.zeros(N, dtype=torch.int32, **z)
        self.ep_ret_sum = torch.zeros(N, dtype=torch.float32, **z)
        self.ep_len_sum = torch.zeros(N, dtype=torch.float32, **z)
        return N, z

    def _episode_counters(self):
        return ptr(self.ep_count), ptr(self.ep_ret_sum), ptr(self.ep_len_sum)

    def _policy_args(self, pm, buf, mode, rng_seed, counter0):
        """The leading arguments of every gs_rollout_* entry."""
        return ptr(pm.params), pm.dims, self.num_envs, buf.T, int(mode), int(rng_seed), int(counter0)

    @staticmethod
    def _row_args(buf):
        """The trailing arguments of every gs_rollout_* entry: the buffer's rows and the stream."""
        return (ptr(buf.obs), ptr(buf.actions), ptr(buf.logprobs), ptr(buf.values), ptr(buf.rewards),
                ptr(buf.dones), ptr(buf.timeouts), stream_handle())

    def _env_args(self):
        """The env's own tensors and parameters, in the order every one of its entries takes them."""
        raise NotImplementedError

    def _reset_args(self):
        """What gs_<x>_reset takes before the stream."""
        return (*self._env_args(), self.num_envs, self.seed, self.env_offset)

    def reset(self):
        entry = f"gs_{self.entry_stem}_reset"
        check(getattr(lib, entry)(*self._reset_args(), stream_handle()), entry)
        return self.obs, {}

    def step_into(self, rewards_row, dones_row, timeouts_row, actions=None, clock=None, step=None):
        """One vector step into the rollout rows (clock / step are the synthetic env's)."""
        if actions is None:
            raise ValueError(self.needs_actions)
        entry = f"gs_{self.entry_stem}_step"
        check(getattr(lib, entry)(*self._env_args(), ptr(actions), self.num_envs, self.max_steps, self.seed,
                                  self.env_offset, ptr(rewards_row), ptr(dones_row), ptr(timeouts_row),
                                  *self._episode_counters(), stream_handle()), entry)

    def _rollout(self, entry, pm, buf, mode, rng_seed, counter0):
        if entry is None:
            raise NotImplementedError(f"{type(self).__name__} has no one-launch rollout of this form")
        kind = (int(self.env_kind),) if entry in ("gs_rollout_env", "gs_rollout1_env") else ()
        check(getattr(lib, entry)(*self._policy_args(pm, buf, mode, rng_seed, counter0), *kind, *self._env_args(),
                                  self.max_steps, self.seed, self.env_offset, *self._episode_counters(),
                                  *self._row_args(buf)), entry)

    def rollout_into(self, pm, buf, mode, rng_seed, counter0):
        """The whole rollout of a two-hidden-layer policy in one launch."""
        self._rollout(self.rollout_entry, pm, buf, mode, rng_seed, counter0)

    def rollout1_into(self, pm, buf, mode, rng_seed, counter0):
        """rollout_into for a one-hidden-layer policy: the gs_rollout1_* entry of the same arguments."""
        self._rollout(self.rollout1_entry, pm, buf, mode, rng_seed, counter0)

    def one_launch_supported(self, dims) -> bool:
        """Whether rollout_into() serves a two-hidden-layer policy of these dims (a host computation)."""
        cap = self.one_launch_max_envs
        if self.rollout_entry is None or (cap is not None and self.num_envs > int(cap)):
            return False
        v = ctypes.c_int()
        check(lib.gs_rollout_env_supported(dims, int(self.env_kind), ctypes.byref(v)), "gs_rollout_env_supported")
        return bool(v.value)

    def one_launch_mlp1_supported(self, dims) -> bool:
        """Whether rollout1_into() serves a one-hidden-layer policy of these dims (a host computation)."""
        if self.rollout1_entry is None:
            return False
        v = ctypes.c_int()
        check(lib.gs_rollout1_supported(dims, ctypes.byref(v)), "gs_rollout1_supported")
        return bool(v.value)


class DeviceSyntheticVecEnv(DeviceVecEnv):
    """Device twin of gsamd.synthetic_env.SyntheticVecEnv (same hash, same episodes).  Its entries
    take a step count kept on the host (or the captured rollout's clock), so it writes out its own
    three calls; there is no one-hidden-layer one-launch rollout."""

    rollout_entry = "gs_rollout_synth"

    def __init__(self, n_envs, obs_dim, n_actions, episode_len=200, seed=42, truncate_every=0, env_offset=0,
                 reward=1.0, device="cuda"):
        N, z = self._alloc(n_envs, obs_dim, n_actions, seed, env_offset, device, meta=False)
        self.episode_len, self.truncate_every, self.reward = int(episode_len), int(truncate_every), float(reward)
        self.state = torch.zeros(4 * N, dtype=torch.int32, **z)
        self.step_count = 0

    def reset(self):
        self.step_count = 0
        check(lib.gs_env_reset(ptr(self.state), ptr(self.ep_ret), ptr(self.obs), self.num_envs, self.obs_dim,
                               self.episode_len, self.seed, self.env_offset, stream_handle()), "gs_env_reset")
        return self.obs, {}

    def step_into(self, rewards_row, dones_row, timeouts_row, actions=None, clock=None, step=None):
        """One vector step into the rollout rows.  clock/step: inside a captured rollout the
        step count is clock[1] (device) + step instead of the host counter."""
        if clock is None:
            self.step_count += 1
        check(lib.gs_env_step(ptr(self.state), ptr(self.ep_ret), ptr(self.obs), self.num_envs, self.obs_dim,
                              self.episode_len, self.truncate_every, self.reward, self.seed, self.env_offset,
                              self.step_count if clock is None else int(step), ptr(rewards_row), ptr(dones_row),
                              ptr(timeouts_row), *self._episode_counters(), ptr(clock), stream_handle()),
              "gs_env_step")

    def rollout_into(self, pm, buf, mode, rng_seed, counter0):
        """gs_rollout_synth, after which the host step counter advances by the rollout's T."""
        check(lib.gs_rollout_synth(*self._policy_args(pm, buf, mode, rng_seed, counter0), ptr(self.state),
                                   ptr(self.ep_ret), ptr(self.obs), self.episode_len, self.truncate_every,
                                   self.reward, self.seed, self.env_offset, self.step_count,
                                   *self._episode_counters(), *self._row_args(buf)), "gs_rollout_synth")
        self.step_count += buf.T

    def one_launch_supported(self, dims) -> bool:
        v = ctypes.c_int()
        check(lib.gs_rollout_synth_supported(dims, ctypes.byref(v)), "gs_rollout_synth_supported")
        return bool(v.value)


class DeviceCartPoleVecEnv(DeviceVecEnv):
    """CartPole-v1 on device (gymnasium 1.x dynamics restated in
    csrc/gs_cartpole.hip, NEXT_STEP autoreset, TimeLimit 500).  Parity with gymnasium's own
    episodes is unpinned (reset draws use a counter hash, not PCG64)."""

    env_kind = GS_ENV_CARTPOLE       # gs_rollout_env's kind: one-launch rollouts when the policy fits in LDS
    entry_stem, rollout_entry, rollout1_entry = "cartpole", "gs_rollout_env", "gs_rollout1_env"
    needs_actions = "CartPole dynamics need the step's actions"

    def __init__(self, n_envs, seed=42, env_offset=0, max_steps=500, wrappers=(), device="cuda", **_):
        """`wrappers` is the config's env_wrappers list: empty, or the reference's
        CartPoleV1_RewardShaper (CartPole-v1:ppo_rewardshaped), which the gs_cartpole_shaped_*
        entries apply on the env's own thread with its previous potential in `prev_phi` (N) f64.
        Without a shaper the env calls the unshaped entries and has no prev_phi."""
        N, z = self._alloc(n_envs, 4, 2, seed, env_offset, device)
        self.max_steps = int(max_steps)
        self.wrappers = [dict(w) for w in (wrappers or ())]
        resolved = resolve_cartpole_wrappers(self.wrappers)
        if resolved is None:
            raise ValueError(f"the device CartPole-v1 does not apply env_wrappers={self.wrappers!r} "
                             "(gsamd.config.resolve_cartpole_wrappers)")
        self.wrappers_c, self.prev_phi = None, None
        if resolved:                             # the reward shaper rides along: the shaped entries
            kw = resolved[0][1]
            self.wrappers_c = CartPoleWrappers(1, int(kw["clip_potential"]), float(kw["angle_reward_scale"]),
                                               float(kw["position_reward_scale"]))
            self.prev_phi = torch.zeros(N, dtype=torch.float64, **z)
            self.entry_stem = "cartpole_shaped"
            self.rollout_entry, self.rollout1_entry = "gs_rollout_cartpole_shaped", "gs_rollout1_cartpole_shaped"
        self.state = torch.zeros(N, 4, dtype=torch.float64, **z)

    @classmethod
    def from_config(cls, c, kind, **kw):
        """The env a config names (device_env_from_config; kw: the stage's seed, the rank's
        env_offset, the device)."""
        if _is_pixel(c) or c.resolved_obs_dim() != 4 or c.resolved_n_actions() != 2:
            raise ValueError("env_dynamics='cartpole' needs vector observations of dim 4 and 2 actions")
        # every stage's env carries the config's reward shaper (the reference builds each from the same list)
        return cls(c.n_envs, max_steps=int(c.max_episode_steps or 500), wrappers=list(c.env_wrappers or ()), **kw)

    def _env_args(self):
        if self.wrappers_c is None:
            return ptr(self.state), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs)
        return ptr(self.state), ptr(self.prev_phi), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs), self.wrappers_c


class DeviceAcrobotVecEnv(DeviceVecEnv):
    """Acrobot-v1 on device (gymnasium 1.x "book" dynamics restated in
    csrc/gs_acrobot_env.h: RK4 of dt 0.2 in double precision, NEXT_STEP autoreset, TimeLimit 500).
    Parity with gymnasium's own episodes is unpinned (reset draws use a counter hash, not PCG64)."""

    env_kind = GS_ENV_ACROBOT
    entry_stem, rollout_entry, rollout1_entry = "acrobot", "gs_rollout_env", "gs_rollout1_env"
    needs_actions = "Acrobot dynamics need the step's actions"
    # One-launch rollouts are the default only up to this many envs: past it the graph-replayed
    # step loop measured faster (profiles/acrobot_collect.json).  None = always.
    one_launch_max_envs = None

    def __init__(self, n_envs, seed=42, env_offset=0, max_steps=500, device="cuda", **_):
        N, z = self._alloc(n_envs, 6, 3, seed, env_offset, device)
        self.max_steps = int(max_steps)
        self.state = torch.zeros(N, 4, dtype=torch.float64, **z)      # theta1, theta2, omega1, omega2

    @classmethod
    def from_config(cls, c, kind, **kw):
        if _is_pixel(c) or c.resolved_obs_dim() != 6 or c.resolved_n_actions() != 3:
            raise ValueError("env_dynamics='acrobot' needs vector observations of dim 6 and 3 actions")
        return cls(c.n_envs, max_steps=int(c.max_episode_steps or 500), **kw)

    def _env_args(self):
        return ptr(self.state), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs)


def mountaincar_wrappers_struct(wrappers) -> MountainCarWrappers:
    """An env_wrappers list (config form: [{"id": ..., **kwargs}], first entry innermost) as the
    gs_mountaincar_wrappers the kernels take; ValueError for a list the device does not apply."""
    resolved = resolve_mountaincar_wrappers(list(wrappers or ()))
    if resolved is None or len(resolved) > 2:
        raise ValueError(f"the device MountainCar-v0 does not apply env_wrappers={list(wrappers)!r} "
                         "(gsamd.config.resolve_mountaincar_wrappers)")
    w = MountainCarWrappers()
    w.order[0] = w.order[1] = GS_MC_WRAP_NONE
    for i, (wid, kw) in enumerate(resolved):
        if wid == "MountainCarV0_RewardShaper":
            w.order[i] = GS_MC_WRAP_SHAPER
            w.position_reward_scale = float(kw["position_reward_scale"])
            w.velocity_reward_scale = float(kw["velocity_reward_scale"])
            w.height_reward_scale = float(kw["height_reward_scale"])
        else:
            w.order[i] = GS_MC_WRAP_BONUS
            w.position_bins, w.velocity_bins = int(kw["position_bins"]), int(kw["velocity_bins"])
            w.bonus_type, w.min_count = GS_MC_BONUS_TYPES[kw["bonus_type"]], int(kw["min_count"])
            w.bonus_scale = float(kw["bonus_scale"])
    return w


class DeviceMountainCarVecEnv(DeviceVecEnv):
    """MountainCar-v0 on device with the reference's reward shaper / state-count bonus wrappers
    (csrc/gs_mountaincar_env.h: gymnasium 1.x dynamics in double precision,
    NEXT_STEP autoreset, TimeLimit 200; the wrappers in double on the float32 observation, in list
    order).  `wrappers` is the config's env_wrappers list.  `counts` holds one int32 visit table
    per env, (N, position_bins * velocity_bins), (N, 0) without a count bonus; reset() zeroes it,
    an episode boundary does not.  Parity with gymnasium's own episodes is unpinned (reset draws
    use a counter hash, not PCG64); the wrappers' arithmetic is pinned to the reference's classes
    (tests/golden/mountaincar_wrappers.npz).  The wrappers' info diagnostics are not reproduced."""

    env_kind = GS_ENV_MOUNTAINCAR
    entry_stem, rollout_entry, rollout1_entry = "mountaincar", "gs_rollout_mountaincar", "gs_rollout1_mountaincar"
    needs_actions = "MountainCar dynamics need the step's actions"
    # One-launch rollouts are the default only up to this many envs: past it the graph-replayed
    # step loop measured faster (profiles/mountaincar_collect.json).  None = always.
    one_launch_max_envs = None

    def __init__(self, n_envs, seed=42, env_offset=0, max_steps=200, wrappers=(), device="cuda", **_):
        N, z = self._alloc(n_envs, 2, 3, seed, env_offset, device)
        self.max_steps = int(max_steps)
        self.wrappers = [dict(w) for w in (wrappers or ())]
        self.wrappers_c = mountaincar_wrappers_struct(self.wrappers)
        cells = self.wrappers_c.position_bins * self.wrappers_c.velocity_bins \
            if GS_MC_WRAP_BONUS in tuple(self.wrappers_c.order) else 0
        self.state = torch.zeros(N, 4, dtype=torch.float64, **z)      # p, v, prev obs p, prev obs v
        self.counts = torch.zeros(N, cells, dtype=torch.int32, **z)

    @classmethod
    def from_config(cls, c, kind, **kw):
        if _is_pixel(c) or c.resolved_obs_dim() != 2 or c.resolved_n_actions() != 3:
            raise ValueError("env_dynamics='mountaincar' needs vector observations of dim 2 and 3 actions")
        # every stage's env carries the config's wrappers (the reference builds each from the same list)
        return cls(c.n_envs, max_steps=int(c.max_episode_steps or 200), wrappers=list(c.env_wrappers or ()), **kw)

    def _env_args(self):
        """Its count tables (NULL without a count bonus) and wrappers ride along."""
        return (ptr(self.state), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs),
                ptr(self.counts) if self.counts.numel() else None, self.wrappers_c)


class DeviceBanditVecEnv(DeviceVecEnv):
    """Bandit-v0 on device (csrc/gs_bandit_env.h restates the reference's
    gym_envs/mab_env.py MultiArmedBanditEnv): a stateless Gaussian bandit whose observation is
    zeros(n_arms), reward mean[a] + std[a] z, terminated after episode_length steps, NEXT_STEP
    autoreset; `max_steps` (a config's max_episode_steps) adds the TimeLimit, default
    episode_length (the env's own spec).  means / stds as the class takes them (None: linspace(0,
    n_arms, n_arms); a scalar std is broadcast), kept as float32.  There is no state tensor.
    Parity with the reference's reward stream is unpinned (the normal draw is Box-Muller on the
    counter hash, not numpy's PCG64 ziggurat)."""

    env_kind = GS_ENV_BANDIT         # one-launch rollouts up to GS_BANDIT_ROLLOUT_MAX_ARMS arms
    # (two hidden layers; the one-hidden-layer entry serves any n_arms the env takes)
    entry_stem, rollout_entry, rollout1_entry = "bandit", "gs_rollout_bandit", "gs_rollout1_bandit"
    needs_actions = "the bandit needs the step's actions"

    def __init__(self, n_envs, n_arms=10, means=None, stds=1.0, episode_length=1, seed=42, env_offset=0,
                 max_steps=None, device="cuda", **_):
        n = int(n_arms)
        if not 2 <= n <= GS_BANDIT_MAX_ARMS:
            raise ValueError(f"n_arms must be in [2, {GS_BANDIT_MAX_ARMS}], got {n_arms}")
        if int(episode_length) < 1:
            raise ValueError("episode_length must be >= 1")
        m, s = bandit_arms(n, means, stds)
        if m.shape != (n,) or s.shape != (n,):
            raise ValueError("means / stds must have n_arms entries")
        if not (np.isfinite(m).all() and np.isfinite(s).all() and (s >= 0).all()):
            raise ValueError("means must be finite, stds finite and >= 0")
        self._alloc(n_envs, n, n, seed, env_offset, device)
        self.n_arms, self.means, self.stds, self.episode_length = n, m, s, int(episode_length)
        self.max_steps = int(max_steps if max_steps else episode_length)
        self.spec = BanditSpec()
        self.spec.n_arms, self.spec.episode_length = n, self.episode_length
        for a in range(n):
            self.spec.means[a], self.spec.stds[a] = float(m[a]), float(s[a])

    @classmethod
    def from_config(cls, c, kind, **kw):
        b = resolve_bandit_env(c)
        if _is_pixel(c) or b is None or c.resolved_n_actions() != b["n_arms"]:
            raise ValueError("env_dynamics='bandit' needs env_id Bandit-v0 with env_kwargs the device applies "
                             "(gsamd.config.resolve_bandit_env)")
        if b["n_arms"] > BANDIT_MAX_TRAINABLE_ARMS:
            # the env kernels take 32 arms; the two-hidden-layer update does not yet (measured at 20 arms:
            # NaN / inf losses).  Its forward stages a 16-row tile's observations and the 16 x (A + 1) head
            # weights with one element per thread of 256: complete only for obs_dim <= 16, n_actions <= 15.
            raise ValueError(f"Bandit-v0 with n_arms={b['n_arms']}: the MLP update serves obs_dim <= 16 and "
                             f"n_actions <= 15, so at most {BANDIT_MAX_TRAINABLE_ARMS} arms train on the device")
        return cls(c.n_envs, n_arms=b["n_arms"], means=b["means"], stds=b["stds"], episode_length=b["episode_length"],
                   max_steps=int(c.max_episode_steps or 0) or None, **kw)

    def _env_args(self):
        return ptr(self.meta), ptr(self.ep_ret), ptr(self.obs), self.spec

    def _reset_args(self):
        """A stateless env with no reset draw: gs_bandit_reset takes no seed and no offset."""
        return (*self._env_args(), self.num_envs)


class DeviceTabularVecEnv(DeviceVecEnv):
    """A tabular env on device (csrc/gs_tabular.hip): FrozenLake-v1 (`kind` "frozenlake", 4x4 or
    8x8, slippery or not) or Taxi-v3 ("taxi") on gsamd.toytext's tables, or any (next, reward,
    term, starts, n_states, n_actions, K) passed as `tables`.  The observation is the reference's
    DiscreteEncoder (`encoding` array / binary / onehot) of the state, as float32.  NEXT_STEP
    autoreset, TimeLimit `max_steps` (default: the registered id's, 100 / 200).  The tables are
    uploaded once, here.  No rollout_entry (the two-hidden-layer one-launch rollout does not serve it):
    by default the collector replays its step graph; a one-hidden-layer policy's whole rollout is
    one launch through rollout1_into when the collector is built with one_launch_mlp1=True.
    Parity with gymnasium's own episodes is unpinned (the outcome and reset draws use the counter
    hash, not PCG64)."""

    entry_stem, rollout1_entry = "tabular", "gs_rollout1_tabular"
    needs_actions = "a tabular env needs the step's actions"

    def __init__(self, n_envs, kind="frozenlake", encoding="binary", map_name="4x4", is_slippery=True, seed=42,
                 env_offset=0, max_steps=None, tables=None, device="cuda", **_):
        from . import toytext
        from .config import discrete_encoding_dim
        if encoding not in GS_ENCODINGS:
            raise ValueError(f"encoding must be one of {tuple(GS_ENCODINGS)}, got {encoding!r}")
        nxt, rew, term, starts, S, A, K = tables if tables is not None else toytext.tables_for(
            kind, map_name, bool(is_slippery))
        self.kind, self.encoding = str(kind), str(encoding)
        self.n_states, self.n_outcomes = int(S), int(K)
        N, z = self._alloc(n_envs, discrete_encoding_dim(self.encoding, self.n_states), A, seed, env_offset, device)
        self.max_steps = int(max_steps if max_steps else toytext.MAX_EPISODE_STEPS.get(self.kind, 100))
        shape = (self.n_states, self.n_actions, self.n_outcomes)
        self.next_table = torch.as_tensor(np.ascontiguousarray(nxt, np.int32).reshape(shape)).to(self.device)
        self.reward_table = torch.as_tensor(np.ascontiguousarray(rew, np.float32).reshape(shape)).to(self.device)
        self.term_table = torch.as_tensor(np.ascontiguousarray(term, np.uint8).reshape(shape)).to(self.device)
        self.starts = torch.as_tensor(np.ascontiguousarray(starts, np.int32).reshape(-1)).to(self.device)
        self.spec = TabularSpec(self.n_states, self.n_actions, self.n_outcomes, int(self.starts.numel()),
                                GS_ENCODINGS[self.encoding], self.obs_dim)
        self.state = torch.zeros(N, dtype=torch.int32, **z)

    @classmethod
    def from_config(cls, c, kind, **kw):
        tab = resolve_tabular_env(c)
        if _is_pixel(c) or tab is None or tab["kind"] != kind:
            raise ValueError(f"env_dynamics={kind!r} needs env_id FrozenLake-v1 / Taxi-v3 with exactly the "
                             "DiscreteEncoder wrapper (gsamd.config.resolve_tabular_env)")
        return cls(c.n_envs, kind=kind, encoding=tab["encoding"], map_name=tab["map_name"],
                   is_slippery=tab["is_slippery"], max_steps=int(c.max_episode_steps or 0) or None, **kw)

    def _env_args(self):
        return (ptr(self.state), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs), self.spec, ptr(self.next_table),
                ptr(self.reward_table), ptr(self.term_table), ptr(self.starts))

    def _reset_args(self):
        """gs_tabular_reset draws a start state: the spec and starts, none of the three tables."""
        return (ptr(self.state), ptr(self.meta), ptr(self.ep_ret), ptr(self.obs), self.spec, ptr(self.starts),
                self.num_envs, self.seed, self.env_offset)


# device_env_kind's strings -> the class that builds itself from the config (from_config); every other
# string is the synthetic env's, or the Atari one's for rgb observations
DEVICE_ENVS = {"cartpole": DeviceCartPoleVecEnv, "acrobot": DeviceAcrobotVecEnv, "mountaincar": DeviceMountainCarVecEnv,
               "bandit": DeviceBanditVecEnv, **{kind: DeviceTabularVecEnv for kind in TABULAR_KINDS}}


def device_env_from_config(c, stage, rank, device):
    """The device env of config.device_env_kind for a stage ("train": the training seeds) and a
    rank (its envs' offset); a config naming an env the device does not simulate raises."""
    kind = device_env_kind(c)
    if kind is None:
        raise ValueError(
            f"env_id {c.env_id!r} (obs_type {c.obs_type!r}) has no device dynamics: pass env=<the gymnasium "
            f"VectorEnv build_env_from_config(config, seed=config.seed_train) returns> (or env_factory=), or "
            f"set env_dynamics='synthetic' for the fixed-length synthetic env of the benchmark")
    off = rank * c.n_envs
    train = stage == "train"
    if kind in DEVICE_ENVS:
        return DEVICE_ENVS[kind].from_config(c, kind, seed=c.seed_train if train else c.seed_val, env_offset=off,
                                             device=device)
    seed = c.seed if train else c.seed + 1000
    if _is_pixel(c):
        return DeviceAtariVecEnv(n_envs=c.n_envs, n_actions=c.resolved_n_actions(), episode_len=c.episode_len,
                                 seed=seed, truncate_every=c.truncate_every, env_offset=off,
                                 frame_stack=int(c.frame_stack or 4), device=device)
    return DeviceSyntheticVecEnv(n_envs=c.n_envs, obs_dim=c.resolved_obs_dim(), n_actions=c.resolved_n_actions(),
                                 episode_len=c.episode_len, seed=seed, truncate_every=c.truncate_every,
                                 env_offset=off, device=device)


class DeviceRolloutBuffer:
    """Preallocated time-major SoA rollout storage in HBM (utils/rollout_buffer.py:28-80)."""

    def __init__(self, n_envs: int, obs_shape, n_steps: int, device, obs_dtype=torch.float32):
        T, N = int(n_steps), int(n_envs)
        self.obs_shape = (int(obs_shape),) if isinstance(obs_shape, int) else tuple(int(x) for x in obs_shape)
        self.T, self.N, self.device, self.obs_dtype = T, N, torch.device(device), obs_dtype
        self.obs_dim = self.obs_shape[0]
        z = dict(device=self.device)
        # (T, N, *obs_shape): f32 vectors, or the u8 frame stacks of the pixel path
        self.obs = torch.zeros(T, N, *self.obs_shape, dtype=obs_dtype, **z)
        self.actions = torch.zeros(T, N, dtype=torch.int64, **z)
        self.logprobs = torch.zeros(T, N, dtype=torch.float32, **z)
        self.values = torch.zeros(T, N, dtype=torch.float32, **z)
        self.rewards = torch.zeros(T, N, dtype=torch.float32, **z)
        self.dones = torch.zeros(T, N, dtype=torch.uint8, **z)
        self.timeouts = torch.zeros(T, N, dtype=torch.uint8, **z)
        self.bootstrapped_values = torch.zeros(T, N, dtype=torch.float32, **z)
        self.advantages = torch.zeros(T, N, dtype=torch.float32, **z)
        self.returns = torch.zeros(T, N, dtype=torch.float32, **z)
        self.last_values = torch.zeros(N, dtype=torch.float32, **z)

    def view(self):
        from ._lib import RolloutView, RolloutViewU8
        V = RolloutViewU8 if self.obs_dtype == torch.uint8 else RolloutView
        return V(ptr(self.obs), ptr(self.actions), ptr(self.logprobs), ptr(self.values),
                           ptr(self.advantages), ptr(self.returns), self.T, self.N)


def _env_major(t: torch.Tensor) -> torch.Tensor:
    T, N = t.shape[0], t.shape[1]
    return t.transpose(0, 1).reshape(N * T, *t.shape[2:])


class DeviceTrajectory:
    """RolloutTrajectory-compatible (utils/rollout_buffer.py:16-25) view of a device rollout."""

    _FIELDS = ("observations", "actions", "rewards", "dones", "logprobs", "values", "advantages", "returns",
               "next_observations")

    def __init__(self, buf: DeviceRolloutBuffer):
        self.buffer = buf

    def __len__(self):
        return self.buffer.T * self.buffer.N

    @property
    def observations(self):
        return _env_major(self.buffer.obs)

    @property
    def actions(self):
        return _env_major(self.buffer.actions)

    @property
    def rewards(self):
        return _env_major(self.buffer.rewards)

    @property
    def dones(self):
        return _env_major(self.buffer.dones).bool()

    @property
    def logprobs(self):
        return _env_major(self.buffer.logprobs)

    @property
    def values(self):
        return _env_major(self.buffer.values)

    @property
    def advantages(self):
        return _env_major(self.buffer.advantages)

    @property
    def returns(self):
        return _env_major(self.buffer.returns)

    @property
    def next_observations(self):
        raise NotImplementedError("next_observations are never read by PPO and are not stored on device")


def compute_batched_gae_advantages_and_returns(values, rewards, dones, timeouts, last_values,
                                               bootstrapped_next_values, gamma, gae_lambda, adv_out=None,
                                               ret_out=None):
    """Same signature and result as utils/returns_advantages.py:115-155, on device tensors
    (T, N); bit-exact with the reference's numpy float32 loop."""
    T, N = values.shape
    dev = values.device
    dones = dones.to(torch.uint8) if dones.dtype != torch.uint8 else dones
    timeouts = timeouts.to(torch.uint8) if timeouts.dtype != torch.uint8 else timeouts
    adv = adv_out if adv_out is not None else torch.empty(T, N, dtype=torch.float32, device=dev)
    ret = ret_out if ret_out is not None else torch.empty(T, N, dtype=torch.float32, device=dev)
    args = [values, rewards, dones, timeouts, bootstrapped_next_values, last_values]
    for a in args:
        if a is not None and not (a.is_cuda and a.is_contiguous()):
            raise ValueError("GAE inputs must be contiguous device tensors")
    check(lib.gs_gae_f32(ptr(values), ptr(rewards), ptr(dones), ptr(timeouts), ptr(bootstrapped_next_values),
                         ptr(last_values), T, N, float(gamma), float(gae_lambda), ptr(adv), ptr(ret),
                         stream_handle()), "gs_gae_f32")
    return adv, ret


class DeviceRolloutCollector:
    """RolloutCollector (utils/rollout_collector.py:22-777) for the device path."""

    def __init__(self, env, policy_model, n_steps, *, gamma: float = 0.99, gae_lambda: float = 0.95,
                 stats_window_size: int = 100, rng_seed: int = 42, track_stats: bool = True,
                 use_graph: bool = True, one_launch: bool = True, normalize_advantages: bool = False,
                 returns_type: str = "gae:rtg", advantages_type: str = "gae", normalize_returns: bool = False,
                 one_launch_mlp1: bool = False, **kwargs):
        self.env = env
        self.policy_model = policy_model
        self.n_steps = int(n_steps)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.n_envs = int(env.num_envs)
        self.device = policy_model.device
        self.rng_seed = int(rng_seed)
        self.track_stats = bool(track_stats)
        # the rollout-level advantage normalisation (normalize_advantages == "rollout":
        # utils/rollout_collector.py:441-442 with returns_advantages.py:61-64), after GAE on the device
        self.normalize_advantages = bool(normalize_advantages)
        self._adv_scratch = None
        # the targets: "gae:rtg" + "gae" (PPO, the default) or the Monte Carlo returns of REINFORCE
        # ("mc:rtg" / "mc:episode" with advantages_type "baseline"; utils/rollout_collector.py:385-426)
        self.returns_type, self.advantages_type = str(returns_type), str(advantages_type)
        if self.returns_type not in ("gae:rtg", "mc:rtg", "mc:episode"):
            raise ValueError(f"Invalid returns_type: {self.returns_type} and advantages_type: {self.advantages_type}")
        self.normalize_returns = bool(normalize_returns)
        # the running baseline over every rollout's valid returns: RunningStats' count / sum /
        # sum_squared as Python floats (utils/rollout_stats.py:34-67)
        self._base_stats = {"count": 0, "sum": 0.0, "sum_squared": 0.0}
        self._mc = None              # device idx_map / last_terminal / valid_sums of the MC targets
        self.idx_map = None          # this rollout's (N * T) int32 env-major index map on the device, or None
        # device envs: the T-step loop (policy act + env step per vector step) is captured once
        # per sampling mode into a hipGraph and replayed; the per-rollout counters reach the
        # kernels through a 2-word device clock (include/gsamd.h "Rollout clock")
        self.use_graph = bool(use_graph)
        # a device env with a policy that fits in LDS: the whole rollout is one launch
        # (gs_rollout_synth for the synthetic env, gs_rollout_env for an env that declares its
        # env_kind; rows bit-identical to the step-wise loop)
        self.one_launch = bool(one_launch) and hasattr(policy_model, "dims") and \
            self._one_launch_supported(env, policy_model)
        # opt-in: a one-hidden-layer policy on a device env with a gs_rollout1_* entry runs the whole
        # rollout as one launch too (gs_rollout1_*: one thread per env; rows bit-identical to the
        # step-wise loop).  Off by default: such a policy then takes the step graph, as before.
        self.one_launch_mlp1 = bool(one_launch_mlp1) and not self.one_launch and hasattr(policy_model, "dims") and \
            self._one_launch_mlp1_supported(env, policy_model)
        self._graphs = {}
        self._clock = None
        self.total_rollouts = self.total_steps = self.total_vec_steps = self.total_episodes = 0
        self.rollout_steps = self.rollout_vec_steps = self.rollout_episodes = 0
        self.stats_window_size = int(stats_window_size)
        self.rollout_fpss = RollingWindow(stats_window_size)
        # finished-episode statistics in the reference's processing order (step, then env):
        # rolling windows, best / last episode (utils/rollout_collector.py:93-98, 210-294)
        self.episode_reward_deque = RollingWindow(stats_window_size)
        self.episode_length_deque = RollingWindow(stats_window_size)
        self._best_episode_reward = -float("inf")
        self._last_episode_reward, self._last_episode_length = 0.0, 0
        self._recent_episodes = []       # (env, return, length, timeout) since the last consumer
        self._buffer: Optional[DeviceRolloutBuffer] = None
        self._started = False
        self._stats = None
        self._action_counts = None       # device int64 histogram of taken actions

    # ---- phases --------------------------------------------------------------------
    def _prepare(self):
        if self._started:
            return
        if getattr(self.env, "device_native", False):
            self.env.reset()
            obs_shape, obs_dtype = tuple(self.env.obs_shape), self.env.obs_dtype
        else:
            obs, _ = self.env.reset()
            obs = np.asarray(obs)
            obs_dtype = torch.uint8 if obs.dtype == np.uint8 else torch.float32
            self._host_obs = obs if obs_dtype == torch.uint8 else obs.astype(np.float32)
            obs_shape = tuple(obs.shape[1:])
        self._buffer = DeviceRolloutBuffer(self.n_envs, obs_shape, self.n_steps, self.device, obs_dtype)
        self._obs_dev = torch.zeros(self.n_envs, *obs_shape, dtype=obs_dtype, device=self.device)
        # running episode return / length per env (carried across rollouts) and this rollout's
        # completed-episode rows (gs_episode_stats)
        z = dict(device=self.device)
        self._run_ret = torch.zeros(self.n_envs, dtype=torch.float32, **z)
        self._run_len = torch.zeros(self.n_envs, dtype=torch.int32, **z)
        self._ep_ret_rows = torch.zeros(self.n_steps, self.n_envs, dtype=torch.float32, **z)
        self._ep_len_rows = torch.zeros(self.n_steps, self.n_envs, dtype=torch.int32, **z)
        self._started = True

    def _reset_env(self):
        """Fresh episodes on every env (evaluate_episodes; the reference sets obs = None)."""
        self._prepare()
        if getattr(self.env, "device_native", False):
            self.env.reset()
        else:
            obs, _ = self.env.reset()
            self._host_obs = np.asarray(obs, dtype=self._host_obs.dtype)
        self._run_ret.zero_()
        self._run_len.zero_()

    @property
    def buffer(self) -> DeviceRolloutBuffer:
        self._prepare()
        return self._buffer

    def collect(self, deterministic: bool = False, replay_actions: Optional[torch.Tensor] = None):
        """One rollout of n_steps vector steps; returns a DeviceTrajectory.

        replay_actions: optional (T, N) int64 device tensor of actions to take instead of
        sampling (parity tests replay a recorded reference rollout)."""
        self._prepare()
        buf, pm, N, T = self._buffer, self.policy_model, self.n_envs, self.n_steps
        t0 = time.time()
        mode = 2 if replay_actions is not None else (1 if deterministic else 0)
        native = getattr(self.env, "device_native", False)
        self.rollout_episodes = 0
        if self.one_launch or self.one_launch_mlp1:
            if replay_actions is not None:
                buf.actions.copy_(replay_actions)
            self._collect_one_launch(mode)
            T = 0                               # the steps ran inside the launch
        elif native and replay_actions is None and self.use_graph:
            self._collect_steps_graph(mode)
            T = 0                               # the steps ran inside the graph
        for t in range(T):
            if replay_actions is not None:
                buf.actions[t].copy_(replay_actions[t])
            counter = self.total_vec_steps + t
            if native:
                pm.act(self.env.obs, mode=mode, rng_seed=self.rng_seed, rng_counter=counter, actions=buf.actions[t],
                       logp=buf.logprobs[t], values=buf.values[t], obs_store=buf.obs[t])
                self.env.step_into(buf.rewards[t], buf.dones[t], buf.timeouts[t], actions=buf.actions[t])
            else:
                self._obs_dev.copy_(torch.from_numpy(self._host_obs))
                pm.act(self._obs_dev, mode=mode, rng_seed=self.rng_seed, rng_counter=counter, actions=buf.actions[t],
                       logp=buf.logprobs[t], values=buf.values[t], obs_store=buf.obs[t])
                actions_np = buf.actions[t].cpu().numpy()
                next_obs, rew, term, trunc, infos = self.env.step(actions_np)
                done = np.logical_or(term, trunc)
                buf.rewards[t].copy_(torch.from_numpy(np.asarray(rew, np.float32)))
                buf.dones[t].copy_(torch.from_numpy(done.astype(np.uint8)))
                buf.timeouts[t].copy_(torch.from_numpy(np.asarray(trunc).astype(np.uint8)))
                self._host_episode_infos(done, np.asarray(trunc, bool), infos)
                self._host_obs = np.asarray(next_obs, dtype=self._host_obs.dtype)
        T = self.n_steps
        last_obs = self.env.obs if native else self._obs_dev.copy_(torch.from_numpy(self._host_obs))
        if self.returns_type != "gae:rtg":
            self._compute_mc_targets()          # no value bootstrap, no GAE
        else:
            pm.predict_values(last_obs, out=buf.last_values)
            compute_batched_gae_advantages_and_returns(buf.values, buf.rewards, buf.dones, buf.timeouts,
                                                       buf.last_values, buf.bootstrapped_values, self.gamma,
                                                       self.gae_lambda, adv_out=buf.advantages, ret_out=buf.returns)
        self.rollout_steps, self.rollout_vec_steps = N * T, T
        self.total_steps += N * T
        self.total_vec_steps += T
        self.total_rollouts += 1
        if self.track_stats:
            self._accumulate_stats()
            if native:
                self._episode_records()
        elif native:
            self._episode_window()
        if self.normalize_advantages:
            self._normalize_rollout_advantages()
        if not native:
            self.total_episodes += self.rollout_episodes
        self.rollout_fpss.append(N * T / max(time.time() - t0, 1e-9))
        return DeviceTrajectory(buf)

    @staticmethod
    def _one_launch_supported(env, pm) -> bool:
        """A two-hidden-layer policy on a device env whose rollout_into serves its shape
        (DeviceVecEnv.one_launch_supported)."""
        if getattr(pm, "valid_mask", 0):     # the one-launch rollouts have no masked head: step loop / step graph
            return False
        if not (getattr(env, "device_native", False) and isinstance(env, DeviceVecEnv)):
            return False                     # a host env, or the Atari env (it has no one-launch rollout)
        return env.one_launch_supported(pm.dims)

    @staticmethod
    def _one_launch_mlp1_supported(env, pm) -> bool:
        """A one-hidden-layer policy on a device env whose rollout1_into serves its shape
        (DeviceVecEnv.one_launch_mlp1_supported); never for a masked policy (no masked head there)."""
        if getattr(pm, "valid_mask", 0) or int(getattr(pm.dims, "hidden2", -1)) != 0:
            return False
        if not (getattr(env, "device_native", False) and isinstance(env, DeviceVecEnv)):
            return False                     # a host env, or the Atari env (it has no one-launch rollout)
        return env.one_launch_mlp1_supported(pm.dims)

    def _collect_one_launch(self, mode):
        """The T vector steps as one launch (policy act + env step per step, envs resident in
        LDS): the env's own gs_rollout_* call (rollout_into), gs_rollout1_* (rollout1_into) for a
        one-hidden-layer policy."""
        run = self.env.rollout1_into if self.one_launch_mlp1 else self.env.rollout_into
        run(self.policy_model, self._buffer, mode, self.rng_seed, self.total_vec_steps)

    def _steps_into_buffer(self, mode, clock=None):
        """The rollout's T vector steps on a device env: policy act (writes the step's obs /
        action / log-prob / value rows) then the env step (reward / done / timeout rows)."""
        buf, pm, env = self._buffer, self.policy_model, self.env
        for t in range(self.n_steps):
            pm.act(env.obs, mode=mode, rng_seed=self.rng_seed, rng_counter=t if clock is not None else
                   self.total_vec_steps + t, actions=buf.actions[t], logp=buf.logprobs[t], values=buf.values[t],
                   obs_store=buf.obs[t], clock=clock)
            env.step_into(buf.rewards[t], buf.dones[t], buf.timeouts[t], actions=buf.actions[t], clock=clock,
                          step=t + 1)

    def _collect_steps_graph(self, mode):
        """Replay the captured T-step graph of this sampling mode (captured on the mode's second
        rollout; the first runs eagerly and allocates every scratch buffer the steps use).  The
        clock holds {rng counter, env step count} at the rollout start."""
        env = self.env
        if self._clock is None:
            self._clock = torch.zeros(2, dtype=torch.int64, device=self.device)
        step0 = int(getattr(env, "step_count", 0))
        g = self._graphs.get(mode)
        if g is None and (mode, "warm") not in self._graphs:
            self._graphs[(mode, "warm")] = True
            self._steps_into_buffer(mode)                       # eager, host counters
            return
        self._clock[0:1].fill_(self.total_vec_steps)
        self._clock[1:2].fill_(step0)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._steps_into_buffer(mode, clock=self._clock)
            self._graphs[mode] = g
        g.replay()
        if hasattr(env, "step_count"):
            env.step_count = step0 + self.n_steps

    def _record_episode(self, env: int, ret: float, length: int, timeout: bool) -> None:
        """One finished episode, as _process_done_infos books it (rollout_collector.py:242-294)."""
        self.episode_reward_deque.append(ret)
        self.episode_length_deque.append(length)
        self._last_episode_reward, self._last_episode_length = ret, length
        self._best_episode_reward = max(self._best_episode_reward, ret)
        self._recent_episodes.append((env, ret, length, timeout))

    def _episode_records(self):
        """This rollout's finished episodes in the reference's order (step, then env), one D2H
        of their (return, length, timeout) records."""
        buf, N, T = self._buffer, self.n_envs, self.n_steps
        check(lib.gs_episode_stats(ptr(buf.rewards), ptr(buf.dones), T, N, ptr(self._run_ret), ptr(self._run_len),
                                   ptr(self._ep_ret_rows), ptr(self._ep_len_rows), stream_handle()),
              "gs_episode_stats")
        at = torch.nonzero(buf.dones.reshape(-1)).squeeze(1)        # time-major = (step, env) order
        rec = torch.stack([at.double(), self._ep_ret_rows.reshape(-1)[at].double(),
                           self._ep_len_rows.reshape(-1)[at].double(),
                           buf.timeouts.reshape(-1)[at].double()]).cpu().numpy()
        for pos, r, length, to in rec.T:
            self._record_episode(int(pos) % N, float(np.float32(r)), int(length), bool(to))
        self.rollout_episodes = rec.shape[1]
        self.total_episodes += self.rollout_episodes

    def _episode_window(self):
        """track_stats=False: the reference's rolling window (the last stats_window_size finished
        episodes, rollout_collector.py:242-294, 753-758) kept on the device with no host sync —
        this rollout's episodes in (step, env) order (gs_episode_stats) are merged behind the
        previous window by index arithmetic; best / last episode and the count ride along."""
        buf, N, T = self._buffer, self.n_envs, self.n_steps
        W = int(self.stats_window_size)
        check(lib.gs_episode_stats(ptr(buf.rewards), ptr(buf.dones), T, N, ptr(self._run_ret), ptr(self._run_len),
                                   ptr(self._ep_ret_rows), ptr(self._ep_len_rows), stream_handle()),
              "gs_episode_stats")
        dev = self.device
        if getattr(self, "_win", None) is None:
            self._win = torch.zeros(2, W, dtype=torch.float64, device=dev)        # returns, lengths
            self._win_meta = torch.zeros(3, dtype=torch.float64, device=dev)      # count, best, -
            self._win_meta[1] = -float("inf")
            self.rollout_episodes_dev = torch.zeros((), dtype=torch.int64, device=dev)
        # one launch (gs_episode_window): the block scan numbers this rollout's episodes in (step,
        # env) order, the last W land behind the shifted previous window
        check(lib.gs_episode_window(ptr(buf.dones), ptr(self._ep_ret_rows), ptr(self._ep_len_rows), T, N, W,
                                    ptr(self._win), ptr(self._win_meta), ptr(self.rollout_episodes_dev),
                                    stream_handle()), "gs_episode_window")

    def _window_metrics(self):
        """roll/ep_rew/{mean,best,last} and roll/ep_len/{mean,last} from the device window (one D2H)."""
        if getattr(self, "_win", None) is None:
            return {}
        w, meta = self._win.cpu().numpy(), self._win_meta.cpu().numpy()
        n = int(min(meta[0], w.shape[1]))
        if n <= 0:
            return {}
        r, ln = w[0, -n:], w[1, -n:]
        return {"roll/ep_rew/mean": float(np.float32(r).mean()), "roll/ep_len/mean": int(ln.mean()),
                "roll/ep_rew/best": float(meta[1]), "roll/ep_rew/last": float(np.float32(r[-1])),
                "roll/ep_len/last": int(ln[-1])}

    def _host_episode_infos(self, done, trunc, infos):
        """A host env's RecordEpisodeStatistics infos (rollout_collector.py:210-294)."""
        ep, mask = infos.get("episode"), infos.get("_episode")
        for e in np.nonzero(done)[0]:
            ok = ep is not None and mask is not None and mask[e]
            self._record_episode(int(e), float(ep["r"][e]) if ok else 0.0, int(ep["l"][e]) if ok else 0,
                                 bool(trunc[e]))
        self.rollout_episodes += int(np.count_nonzero(done))

    def baseline_mean(self) -> float:
        b = self._base_stats
        return b["sum"] / b["count"] if b["count"] else 0.0

    def _compute_mc_targets(self):
        """The reference's mc:* branch (utils/rollout_collector.py:385-431) on the device:
        gs_mc_returns_f32 (returns, the index map up to each env's last terminal, the valid returns'
        sums; timeouts count as terminals, the reference's mc_treat_timeouts_as_terminals default),
        the running baseline updated with this rollout's valid returns (one 24-byte read: the
        baseline is host state, Python floats as RunningStats keeps them), advantages = returns -
        f32(baseline mean) when advantages_type is "baseline", then the rollout normalisation of the
        returns (gs_normalize_advantages: its arithmetic is _normalize_returns').  The advantages'
        rollout normalisation follows in collect(), as for GAE.  The running roll/* statistics cover
        every position of the rollout (the reference restricts them to the valid ones)."""
        from ._lib import GS_MC_EPISODE, GS_MC_RTG
        buf, T, N = self._buffer, self.n_steps, self.n_envs
        if self._mc is None:
            self._mc = {"idx_map": torch.zeros(N * T, dtype=torch.int32, device=self.device),
                        "last_terminal": torch.zeros(N, dtype=torch.int32, device=self.device),
                        "valid_sums": torch.zeros(3, dtype=torch.float64, device=self.device)}
        mc = self._mc
        kind = GS_MC_EPISODE if self.returns_type == "mc:episode" else GS_MC_RTG
        check(lib.gs_mc_returns_f32(ptr(buf.rewards), ptr(buf.dones), None, T, N, float(self.gamma), kind,
                                    ptr(buf.returns), ptr(mc["idx_map"]), ptr(mc["last_terminal"]),
                                    ptr(mc["valid_sums"]), stream_handle()), "gs_mc_returns_f32")
        count, total, squares = mc["valid_sums"].cpu().tolist()
        if count > 0:
            b = self._base_stats
            b["count"] += int(count)
            b["sum"] += float(total)
            b["sum_squared"] += float(squares)
            self.idx_map = mc["idx_map"]
        else:
            self.idx_map = None          # nothing valid: the reference keeps no map
        if self.advantages_type == "baseline":
            torch.sub(buf.returns, float(np.float32(self.baseline_mean())), out=buf.advantages)
        else:
            buf.advantages.copy_(buf.returns)
        if self.normalize_returns:
            self._normalize_in_place(buf.returns)

    def _normalize_in_place(self, x, mean_std=None):
        if self._adv_scratch is None:
            nb = int(lib.gs_normalize_advantages_scratch_bytes(x.numel()))
            self._adv_scratch = torch.zeros(max(1, nb // 4), dtype=torch.float32, device=self.device)
            self.adv_mean_std = torch.zeros(2, dtype=torch.float32, device=self.device)
        check(lib.gs_normalize_advantages(ptr(x), x.numel(), 1e-8, ptr(self._adv_scratch), ptr(mean_std),
                                          stream_handle()), "gs_normalize_advantages")

    def _normalize_rollout_advantages(self):
        """adv = (adv - mean) / (std + 1e-8) over the whole rollout in place
        (gs_normalize_advantages; utils/returns_advantages.py:61-64), after the pre-normalisation
        advantage statistics were taken; with track_stats the normalised advantages feed the
        roll/adv_norm/* running statistics (utils/rollout_collector.py:441-448)."""
        buf = self._buffer
        if self._adv_scratch is None:
            nb = int(lib.gs_normalize_advantages_scratch_bytes(buf.advantages.numel()))
            self._adv_scratch = torch.zeros(max(1, nb // 4), dtype=torch.float32, device=self.device)
            self.adv_mean_std = torch.zeros(2, dtype=torch.float32, device=self.device)
        check(lib.gs_normalize_advantages(ptr(buf.advantages), buf.advantages.numel(), 1e-8, ptr(self._adv_scratch),
                                          ptr(self.adv_mean_std), stream_handle()), "gs_normalize_advantages")
        if self.track_stats:
            s = self._stats
            s[10] += buf.advantages.sum(dtype=torch.float64)
            s[11] += (buf.advantages.double() ** 2).sum()
            s[12] += buf.advantages.numel()

    def _accumulate_stats(self):
        """Device-side RunningStats sums (utils/rollout_stats.py:34-67) for get_metrics (slots 10-12:
        the normalised advantages, filled by _normalize_rollout_advantages)."""
        buf = self._buffer
        if self._stats is None:
            self._stats = torch.zeros(13, dtype=torch.float64, device=self.device)
        s = self._stats
        s[0] += buf.obs.numel()
        if buf.obs.dtype == torch.uint8:     # exact, without a float copy of the frames
            cnt = torch.bincount(buf.obs.reshape(-1), minlength=256).double()
            v = torch.arange(256, dtype=torch.float64, device=self.device)
            s[1] += (cnt * v).sum()
            s[2] += (cnt * v * v).sum()
        else:
            s[1] += buf.obs.sum(dtype=torch.float64)
            s[2] += (buf.obs.double() ** 2).sum()
        s[3] += buf.rewards.sum(dtype=torch.float64)
        s[4] += (buf.rewards.double() ** 2).sum()
        s[5] += buf.advantages.sum(dtype=torch.float64)
        s[6] += (buf.advantages.double() ** 2).sum()
        s[7] += buf.returns.sum(dtype=torch.float64)
        s[8] += (buf.returns.double() ** 2).sum()
        s[9] += buf.rewards.numel()
        # action histogram (rollout_collector.py:189-199), on device
        n_act = int(getattr(self.policy_model, "n_actions", 0)) or int(buf.actions.max().item()) + 1
        h = torch.bincount(buf.actions.reshape(-1), minlength=n_act)
        if self._action_counts is None or self._action_counts.numel() < h.numel():
            grown = torch.zeros(h.numel(), dtype=torch.int64, device=self.device)
            if self._action_counts is not None:
                grown[:self._action_counts.numel()] += self._action_counts
            self._action_counts = grown
        self._action_counts[:h.numel()] += h

    # ---- evaluation (utils/rollout_collector.py:570-655) -----------------------------
    def evaluate_episodes(self, *, n_episodes: int, deterministic: bool = True,
                          timeout_seconds: Optional[float] = None) -> dict:
        """The reference's protocol on this collector's env: fresh episodes on every env, whole
        rollouts (deterministic: argmax actions) until every env finished its balanced share of
        n_episodes; means over those episodes only, env steps counted per rollout."""
        N = self.n_envs
        base, rem = divmod(int(n_episodes), N)
        targets = [base + (1 if i < rem else 0) for i in range(N)]
        counts = [0] * N
        rew_sum, len_sum, steps, vec_steps = 0.0, 0, 0, 0
        self._reset_env()
        self._recent_episodes = []
        was_tracking, self.track_stats = self.track_stats, True    # episode records are needed
        t0 = time.time()
        try:
            while any(c < t for c, t in zip(counts, targets)):
                self.collect(deterministic=deterministic)
                steps += N * self.n_steps
                vec_steps += self.rollout_vec_steps
                recent, self._recent_episodes = self._recent_episodes, []
                for env, r, length, _ in recent:
                    if counts[env] >= targets[env]:
                        continue
                    rew_sum += float(r)
                    len_sum += int(length)
                    counts[env] += 1
                if timeout_seconds is not None and time.time() - t0 >= float(timeout_seconds):
                    break
        finally:
            self.track_stats = was_tracking
        total = int(sum(counts))
        m = self.get_metrics()
        m.pop("action_dist", None)
        m.update({"cnt/total_episodes": total, "cnt/total_env_steps": int(steps), "cnt/total_vec_steps": int(vec_steps)})
        if total > 0:
            m["roll/ep_rew/mean"] = float(rew_sum / total)
            m["roll/ep_len/mean"] = float(len_sum / total)
        return m

    # ---- API parity ------------------------------------------------------------------
    def slice_trajectories(self, trajectories, idxs):
        """utils/rollout_collector.py:657-682 — index the env-major views."""
        idx = torch.as_tensor(idxs, dtype=torch.int64, device=self.device)
        if self.idx_map is not None:        # MC targets: every index -> its nearest earlier valid position
            idx = self.idx_map.long()[idx]
        from types import SimpleNamespace
        return SimpleNamespace(**{f: getattr(trajectories, f)[idx] for f in DeviceTrajectory._FIELDS[:-1]})

    def get_metrics(self):
        """utils/rollout_collector.py:686-760: counters, running obs / reward / return /
        advantage statistics, the action histogram and its moments, baseline statistics (PPO's
        GAE targets never update them: zeros), and — once an episode has finished — the rolling
        window means, best and last episode.  In a multi-rank job the additive sums (steps,
        episodes, statistics, action counts) are summed over ranks before the means; the rolling
        window and best/last episode are this rank's."""
        part = [self.rollout_steps, self.total_episodes, self.rollout_episodes]
        n_stats = 0
        if self._stats is not None:
            st = list(self._stats.cpu().numpy().astype(np.float64))
            n_stats = len(st)
            part += st
        counts = self._action_counts.cpu().numpy() if self._action_counts is not None else np.zeros(0, np.int64)
        part += list(counts.astype(np.float64))
        env = self.env
        native = getattr(env, "device_native", False)
        dev_eps = native and not self.track_stats      # episode sums from the env's device counters
        if dev_eps:
            part += [float(env.ep_count.sum().item()), float(env.ep_ret_sum.sum().item()),
                     float(env.ep_len_sum.sum().item())]
        part = allreduce_sum_f64(part)
        scale = part[0] / max(self.rollout_steps, 1)
        m = {"cnt/total_env_steps": int(round(self.total_steps * scale)), "cnt/total_vec_steps": self.total_vec_steps,
             "cnt/total_episodes": int(part[1]), "cnt/total_rollouts": self.total_rollouts,
             "roll/env_steps": int(part[0]), "roll/vec_steps": self.rollout_vec_steps,
             "roll/episodes": int(part[2]), "roll/fps": float(self.rollout_fpss.mean()) if self.rollout_fpss else 0.0}

        def mean_std(sum_, sq, n):      # RunningStats.mean / .std (rollout_stats.py:59-67)
            if n <= 0:
                return 0.0, 0.0
            mean = sum_ / n
            return float(mean), float(np.sqrt(max(0.0, sq / n - mean * mean)))
        zero = (0.0, 0.0)
        if n_stats:
            s = part[3:3 + n_stats]
            obs, rew, adv, ret = (mean_std(s[1], s[2], s[0]), mean_std(s[3], s[4], s[9]), mean_std(s[5], s[6], s[9]),
                                  mean_std(s[7], s[8], s[9]))
        else:
            obs = rew = adv = ret = zero
        m["roll/obs/mean"], m["roll/obs/std"] = obs
        m["roll/reward/mean"], m["roll/reward/std"] = rew
        m["roll/return/mean"], m["roll/return/std"] = ret
        m["roll/adv/mean"], m["roll/adv/std"] = adv
        hist = np.asarray(part[3 + n_stats:3 + n_stats + counts.size], np.int64)
        nz = np.flatnonzero(hist)
        if nz.size:     # the reference's histogram grows to the largest action seen
            hist = hist[:nz[-1] + 1]
            idxs = np.arange(hist.shape[0], dtype=np.float32)
            total = float(hist.sum())
            a_mean = float((idxs * hist).sum() / total)
            a_var = float(((idxs - a_mean) ** 2 * hist).sum() / total)
            m["roll/actions/mean"], m["roll/actions/std"] = a_mean, float(np.sqrt(max(0.0, a_var)))
            m["action_dist"] = hist
        else:
            m["roll/actions/mean"], m["roll/actions/std"], m["action_dist"] = 0.0, 0.0, None
        b = self._base_stats             # the MC baseline (GAE targets never update it: zeros)
        m["roll/baseline/mean"], m["roll/baseline/std"] = mean_std(b["sum"], b["sum_squared"], b["count"])
        if self.normalize_advantages and n_stats and s[12] > 0:      # rollout_collector.py:748-750
            m["roll/adv_norm/mean"], m["roll/adv_norm/std"] = mean_std(s[10], s[11], s[12])
        if dev_eps:
            cnt = part[-3]
            m["cnt/total_episodes"] = int(cnt)
            m.update(self._window_metrics())      # this rank's rolling window, as the reference's deques
        elif self.episode_reward_deque:
            m["roll/ep_rew/mean"] = float(self.episode_reward_deque.mean())
            m["roll/ep_len/mean"] = int(self.episode_length_deque.mean())
            m["roll/ep_rew/best"] = float(self._best_episode_reward)
            m["roll/ep_rew/last"] = float(self._last_episode_reward)
            m["roll/ep_len/last"] = int(self._last_episode_length)
        return m
