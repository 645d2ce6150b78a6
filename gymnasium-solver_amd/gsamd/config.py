"""Config entry point for the device path — same `<env>:<variant>` ids and resolution rules
as the reference's utils/config.py (Config/PPOConfig :17-885, build_from_yaml :363-445,
load_config :887-889), restricted to the fields the rollout + GAE + PPO-update path reads.

Two sources:
  * ``config_dir`` = the reference's ``config/environments`` directory (drop-in mode):
    the YAML files are parsed with the reference's rules (``_base``/anchors, variant
    dicts inheriting file-level fields, ``project_id_variant`` / ``env_id_variant``
    aliases, numeric-string coercion :588-592, fractional batch size :594-607,
    unknown keys dropped :354-357);
  * otherwise the resolved presets of the BASELINE.json configs (gsamd/presets.py).
The BASELINE ids ``LunarLander-v2`` and ``ALE/*:ppo`` are accepted as aliases of
``LunarLander-v3`` and ``ALE-*:rgb_ppo``.
"""
from __future__ import annotations

import dataclasses
import glob
import os
import re
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import yaml

from .presets import MODEL_REGISTRY, PRESETS


# the optimizers of utils/optimizer_factory.py:6-29, each at torch's defaults but lr (include/gsamd.h GS_HP_OPT_*)
OPTIMIZERS = ("adam", "adamw", "sgd")


@dataclass
class PPOConfig:
    env_id: str = ""
    project_id: str = ""
    algo_id: str = "ppo"
    n_envs: int = 8
    n_steps: int = 2048
    batch_size: Any = 64
    n_epochs: int = 10
    max_epochs: Optional[int] = None
    max_env_steps: Optional[float] = None
    seed: int = 42
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    clip_range_vf: float = 0.2
    target_kl: Optional[float] = None
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    policy_lr: float = 3e-4
    optimizer: str = "adam"
    normalize_advantages: str = "batch"
    model_id: str = "mlp_medium"
    obs_type: str = "vector"
    frame_stack: Optional[int] = None
    accelerator: str = "auto"
    spec: Dict[str, Any] = field(default_factory=dict)
    # env construction fields the env choice depends on (utils/config.py:96-151, get_env_args :676-696)
    max_episode_steps: Optional[int] = None
    seed_train: int = 42
    seed_val: int = 1042
    seed_test: int = 2042
    env_wrappers: List[Any] = field(default_factory=list)
    env_kwargs: Dict[str, Any] = field(default_factory=dict)
    normalize_obs: Any = False
    # device-path extras (not reference fields): synthetic env shape for bench / tests
    obs_dim: Optional[int] = None
    n_actions: Optional[int] = None
    episode_len: int = 200
    truncate_every: int = 0
    # which env the agent steps when the caller passes none (device_env_kind):
    #   "auto"      the env_id's own dynamics where the device implements them (CartPole-v1, Acrobot-v1,
    #               MountainCar-v0), otherwise the caller must pass the host VectorEnv (raises if not)
    #   "synthetic" the fixed-length-episode synthetic env of SURVEY §8d (bench / tests), or the
    #               synthetic Atari frame source for rgb configs
    #   "cartpole"  device CartPole-v1 dynamics
    #   "acrobot"   device Acrobot-v1 dynamics
    #   "mountaincar" device MountainCar-v0 dynamics with the config's env_wrappers
    #   "frozenlake" / "taxi" the device tabular env on gsamd.toytext's tables, with the config's
    #               DiscreteEncoder and (FrozenLake) map kwargs
    #   "bandit"    the device Bandit-v0 with the config's env_kwargs (resolve_bandit_env)
    env_dynamics: str = "auto"
    # data-parallel semantics of a multi-rank update:
    #   "local"  every rank takes B-row minibatches of its own samples (weak scaling, global batch G·B)
    #   "global" every rank takes its share of the reference's global minibatches (the single-GPU
    #            math on G GPUs: global sampler, normalisation and KL stop; gs_ppo_update_global)
    dp_mode: str = "local"
    # MFMA operand precision of the NatureCNN update (include/gsamd.h GS_HP_BF16): "fp32" (the
    # parity path, default) or "bf16" (bf16 operands, fp32 accumulation / parameters / Adam)
    precision: str = "fp32"
    # {param: {schedule, start_value, end_value, start, end, warmup}} (gsamd.schedules)
    schedules: Dict[str, Dict[str, Any]] = field(default_factory=dict)

    def __post_init__(self):
        self._resolve_schedules()
        self._resolve_numeric_strings()
        self._resolve_batch_size()
        self.validate()

    # --- reference-equivalent resolution -------------------------------------------
    def _resolve_schedules(self):
        """utils/config.py:626-655: dict-valued policy_lr / ent_coef start at their 'start'."""
        from .schedules import parse_schedule_dict
        self.schedules = dict(self.schedules or {})
        for p in ("policy_lr", "ent_coef"):
            v = getattr(self, p)
            if isinstance(v, dict):
                spec = parse_schedule_dict(v)
                self.schedules[p] = spec
                setattr(self, p, spec["start_value"])

    def _resolve_numeric_strings(self):
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if isinstance(v, str):
                try:
                    setattr(self, f.name, float(v))
                except ValueError:
                    pass

    def _resolve_batch_size(self):
        if self.batch_size is not None and self.batch_size <= 1:
            self.batch_size = max(1, int(self.n_envs * self.n_steps * self.batch_size))
        self.batch_size = int(self.batch_size)

    def validate(self):
        # utils/optimizer_factory.py:6-29: a name or an enum-like with .value, case-insensitive
        opt = str(getattr(self.optimizer, "value", self.optimizer)).lower()
        if opt not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of 'adam', 'adamw' or 'sgd', got {self.optimizer!r}")
        self.optimizer = opt
        for k in ("n_envs", "n_steps", "batch_size", "n_epochs", "policy_lr"):
            if getattr(self, k) is not None and getattr(self, k) <= 0:
                raise ValueError(f"{k} must be positive, got {getattr(self, k)}")
        if not (0 < self.gamma <= 1):
            raise ValueError("gamma must be in (0, 1]")
        rollout = self.n_envs * self.n_steps
        if self.dp_mode == "global":
            pass        # minibatches span every rank's rollout: DevicePPOAgent checks them with the world size
        elif self.batch_size > rollout:
            raise ValueError(f"batch_size ({self.batch_size}) should not exceed n_envs ({self.n_envs}) * "
                             f"n_steps ({self.n_steps}).")
        if self.dp_mode != "global" and rollout % self.batch_size != 0:
            raise ValueError("batch_size must divide (n_envs * n_steps) exactly to yield uniform minibatches: "
                             f"rollout_size={rollout}, batch_size={self.batch_size}.")
        if self.normalize_advantages not in ("batch", "rollout", "off", False, None, ""):
            raise ValueError("normalize_advantages must be 'rollout', 'batch', or 'off'.")
        if self.precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {self.precision!r}")
        if self.precision == "bf16" and self.obs_type != "rgb" and self.target_kl is not None:
            raise ValueError("precision 'bf16' of the MLP update runs on its fused chain, which has no KL early "
                             "stop: unset target_kl or use precision 'fp32'")
        if self.dp_mode not in ("local", "global"):
            raise ValueError(f"dp_mode must be 'local' or 'global', got {self.dp_mode!r}")
        if str(self.env_dynamics or "auto") not in ENV_DYNAMICS:
            raise ValueError(f"env_dynamics must be one of {ENV_DYNAMICS}, got {self.env_dynamics!r}")

    # --- derived -----------------------------------------------------------------------
    @property
    def hidden_dims(self) -> Tuple[int, ...]:
        return tuple(MODEL_REGISTRY[self.model_id]["hidden_dims"])

    @property
    def activation(self) -> str:
        return MODEL_REGISTRY[self.model_id].get("activation", "relu")

    @property
    def valid_actions(self) -> Optional[List[int]]:
        return (self.spec or {}).get("action_space", {}).get("valid")

    def resolved_n_actions(self) -> int:
        if self.n_actions:
            return int(self.n_actions)
        return int((self.spec or {}).get("action_space", {}).get("discrete", 2))

    def resolved_obs_dim(self) -> int:
        if self.obs_dim:
            return int(self.obs_dim)
        bandit = resolve_bandit_env(self)
        if bandit is not None:          # Bandit-v0 observes zeros(n_arms)
            return int(bandit["n_arms"])
        obs = (self.spec or {}).get("observation_space", {})
        variants = obs.get("variants", {})
        default = variants.get(obs.get("default", "state"), {})
        if not default.get("shape") and default.get("n"):
            # a Discrete space (`n` states): the observation is what the config's DiscreteEncoder makes of it
            tab = resolve_tabular_env(self)
            if tab is not None:
                return int(tab["obs_dim"])
            enc = [w for w in (self.env_wrappers or []) if isinstance(w, dict) and w.get("id") == "DiscreteEncoder"]
            if enc and enc[-1].get("encoding", "binary") in DISCRETE_ENCODINGS:
                return discrete_encoding_dim(enc[-1].get("encoding", "binary"), int(default["n"]))
        shape = default.get("shape") or [4]
        if isinstance(shape[0], str):   # a symbolic length (Bandit-v0's [n_arms]): the env kwarg of that name
            return int((self.env_kwargs or {})[shape[0]])
        return int(shape[0])

    def get_rollout_collector_kwargs(self) -> Dict[str, Any]:
        """utils/config.py:698-718."""
        return dict(n_steps=self.n_steps, gamma=self.gamma, gae_lambda=self.gae_lambda,
                    normalize_returns=False, returns_type="gae:rtg", advantages_type="gae",
                    normalize_advantages=self.normalize_advantages == "rollout")


@dataclass
class REINFORCEConfig(PPOConfig):
    """The reference's REINFORCEConfig (utils/config.py:806-820) on the device path: Monte Carlo
    targets, one pass of large minibatches.  Defaults are the reference's; normalize_advantages is a
    field the reference's class lacks (agents/base_agent.py:117 reads it and raises AttributeError on
    the first minibatch): here it exists and defaults to "off".  The PPO-only fields (clip ranges,
    vf_coef, gae_lambda, target_kl) are carried and not read."""
    algo_id: str = "reinforce"
    n_steps: int = 2048
    batch_size: Any = 2048
    n_epochs: int = 1
    policy_lr: float = 1e-2
    gamma: float = 0.99
    ent_coef: float = 0.01
    max_grad_norm: float = 0.5
    normalize_advantages: str = "off"
    returns_type: str = "mc:rtg"            # "mc:rtg" (reward to go) | "mc:episode" (whole-episode return)
    policy_targets: str = "returns"         # what the loss scales the log-probabilities by: "returns" | "advantages"
    normalize_returns: str = "off"          # "off" | "rollout" (the collector) | "batch" (the loss)

    def validate(self):
        super().validate()
        for k in ("returns_type", "policy_targets", "normalize_returns"):    # enums of the reference reduce to values
            setattr(self, k, getattr(getattr(self, k), "value", getattr(self, k)))
        if self.normalize_returns in (None, False, ""):
            self.normalize_returns = "off"
        if self.normalize_advantages in (None, False, ""):
            self.normalize_advantages = "off"
        if self.returns_type not in ("mc:rtg", "mc:episode"):
            raise ValueError(f"returns_type must be 'mc:rtg' or 'mc:episode' for REINFORCE, got {self.returns_type!r}")
        if self.policy_targets not in ("returns", "advantages"):
            raise ValueError("policy_targets must be 'returns' or 'advantages'.")
        if self.normalize_returns not in ("batch", "rollout", "off"):
            raise ValueError("normalize_returns must be 'rollout', 'batch', or 'off'.")
        if self.target_kl is not None:
            raise ValueError("target_kl is a PPO setting: REINFORCE never stops an epoch early")

    def get_rollout_collector_kwargs(self) -> Dict[str, Any]:
        """utils/config.py:698-718: no advantages_type on this class, so the collector infers "baseline"
        (utils/rollout_collector.py:57-63)."""
        return dict(n_steps=self.n_steps, gamma=self.gamma, gae_lambda=self.gae_lambda,
                    normalize_returns=self.normalize_returns == "rollout", returns_type=self.returns_type,
                    advantages_type="baseline", normalize_advantages=self.normalize_advantages == "rollout")


CONFIG_CLASSES = {"ppo": PPOConfig, "reinforce": REINFORCEConfig}
_FIELDS = {f.name for f in dataclasses.fields(PPOConfig)}
_YAML_FIELDS = _FIELDS | {f.name for f in dataclasses.fields(REINFORCEConfig)}


def _config_class(algo_id):
    algo = getattr(algo_id, "value", algo_id) or "ppo"
    if algo not in CONFIG_CLASSES:
        raise ValueError(f"device path implements algo_id 'ppo' and 'reinforce' only, got {algo!r}")
    return CONFIG_CLASSES[algo]


def _fields_of(cls):
    return {f.name for f in dataclasses.fields(cls)}


_ALIASES = {"LunarLander-v2": "LunarLander-v3"}

ENV_DYNAMICS = ("auto", "synthetic", "cartpole", "acrobot", "mountaincar", "frozenlake", "taxi", "bandit")
# env ids whose dynamics the device implements, as BaseAgent.build_env would build them from a
# config without wrappers / env kwargs / observation normalisation; the two
# tabular envs need exactly the DiscreteEncoder wrapper (resolve_tabular_env)
DEVICE_DYNAMICS = {"CartPole-v1": "cartpole", "Acrobot-v1": "acrobot", "MountainCar-v0": "mountaincar",
                   "FrozenLake-v1": "frozenlake", "Taxi-v3": "taxi", "Bandit-v0": "bandit"}
TABULAR_KINDS = ("frozenlake", "taxi")
DISCRETE_ENCODINGS = ("array", "binary", "onehot")      # gym_wrappers/discrete_encoder.py
MAX_POLICY_OBS_DIM = 64                                 # csrc/gs_common.h kMaxObsDim
FROZENLAKE_MAPS = {"4x4": 16, "8x8": 64}                # map_name -> states
TAXI_STATES = 500


def discrete_encoding_dim(encoding: str, n_states: int) -> int:
    """Observation length of the reference's DiscreteEncoder (gym_wrappers/discrete_encoder.py:26-50)."""
    if encoding == "array":
        return 1
    if encoding == "binary":
        return max(1, (int(n_states) - 1).bit_length())     # max(1, ceil(log2 n)) in integers
    if encoding == "onehot":
        return int(n_states)
    raise ValueError(f"encoding must be one of {DISCRETE_ENCODINGS}, got {encoding!r}")


def resolve_tabular_env(cfg) -> Optional[Dict[str, Any]]:
    """What the device tabular env needs from a FrozenLake-v1 / Taxi-v3 config, or None when the
    device does not build that env (the host env then): env_wrappers exactly one
    {"id": "DiscreteEncoder"[, "encoding": array | binary | onehot]} (a missing encoding is the
    class default, binary); for FrozenLake env_kwargs with only is_slippery (bool) and map_name
    ("4x4" | "8x8"), for Taxi none; a onehot of more than 64 states exceeds the policy's obs_dim.
    An unwrapped Discrete env has no float observation, so a config without the encoder is host
    too.  Returns {kind, encoding, n_states, obs_dim, map_name, is_slippery}."""
    kind = DEVICE_DYNAMICS.get(str(getattr(cfg, "env_id", "")))
    if kind not in TABULAR_KINDS:
        return None
    wrappers = getattr(cfg, "env_wrappers", None) or []
    if len(wrappers) != 1 or not isinstance(wrappers[0], dict):
        return None
    w = wrappers[0]
    if w.get("id") != "DiscreteEncoder" or set(w) - {"id", "encoding"}:
        return None
    encoding = w.get("encoding", "binary")
    if encoding not in DISCRETE_ENCODINGS:
        return None
    kwargs = getattr(cfg, "env_kwargs", None) or {}
    map_name, slippery = "4x4", True            # gymnasium's FrozenLake-v1 defaults
    if kind == "frozenlake":
        if set(kwargs) - {"is_slippery", "map_name"}:
            return None
        map_name, slippery = kwargs.get("map_name", map_name), kwargs.get("is_slippery", slippery)
        if map_name not in FROZENLAKE_MAPS or not isinstance(slippery, bool):
            return None
        n_states = FROZENLAKE_MAPS[map_name]
    else:
        if kwargs:
            return None
        n_states = TAXI_STATES
    obs_dim = discrete_encoding_dim(encoding, n_states)
    if obs_dim > MAX_POLICY_OBS_DIM:
        return None
    return dict(kind=kind, encoding=encoding, n_states=n_states, obs_dim=obs_dim, map_name=map_name,
                is_slippery=slippery)

# The env_wrappers the device MountainCar-v0 applies itself (csrc/gs_mountaincar_env.h), with the
# keyword arguments and defaults of the reference's classes
# (gym_wrappers/MountainCarV0/reward_shaper.py:9, state_count_bonus.py:13-21)
MOUNTAINCAR_WRAPPERS = {
    "MountainCarV0_RewardShaper": {"position_reward_scale": 100.0, "velocity_reward_scale": 10.0,
                                   "height_reward_scale": 50.0},
    "MountainCarV0_StateCountBonus": {"position_bins": 50, "velocity_bins": 50, "bonus_scale": 1.0,
                                      "bonus_type": "count", "min_count": 1},
}
MOUNTAINCAR_BONUS_TYPES = ("count", "inverse", "log")
MOUNTAINCAR_MAX_CELLS = 16384      # position_bins * velocity_bins of one env's count table


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == v and abs(v) != float("inf")


def resolve_mountaincar_wrappers(wrappers) -> Optional[List[Tuple[str, Dict[str, Any]]]]:
    """A config's env_wrappers list as [(id, keyword arguments with the reference's defaults
    filled in)], in list order (first entry innermost), when the device MountainCar applies it:
    each entry one of MOUNTAINCAR_WRAPPERS, each id at most once, only the classes' own keyword
    arguments, bonus_type one of count / inverse / log, min_count an integer >= 1, positive
    integer bins with position_bins * velocity_bins <= 16384.  None for any other list (the
    host env then)."""
    out, seen = [], set()
    for w in wrappers or []:
        if not isinstance(w, dict):
            return None
        wid = w.get("id")
        if wid not in MOUNTAINCAR_WRAPPERS or wid in seen:
            return None
        seen.add(wid)
        kw = dict(MOUNTAINCAR_WRAPPERS[wid])
        for k, v in w.items():
            if k == "id":
                continue
            if k not in kw:
                return None
            kw[k] = v
        if wid == "MountainCarV0_RewardShaper":
            if not all(_is_real(v) for v in kw.values()):
                return None
        else:
            pb, vb = kw["position_bins"], kw["velocity_bins"]
            if not (_is_int(pb) and _is_int(vb) and pb > 0 and vb > 0 and pb * vb <= MOUNTAINCAR_MAX_CELLS):
                return None
            if kw["bonus_type"] not in MOUNTAINCAR_BONUS_TYPES or not _is_real(kw["bonus_scale"]):
                return None
            if not (_is_int(kw["min_count"]) and kw["min_count"] >= 1):
                return None
        out.append((wid, kw))
    return out


# The one env_wrapper the device CartPole-v1 applies itself (csrc/gs_cartpole_env.h), with the
# keyword arguments and defaults of the reference's class (gym_wrappers/CartPoleV1/reward_shaper.py:23-29)
CARTPOLE_WRAPPERS = {
    "CartPoleV1_RewardShaper": {"angle_reward_scale": 1.0, "position_reward_scale": 0.25, "clip_potential": True},
}


def resolve_cartpole_wrappers(wrappers) -> Optional[List[Tuple[str, Dict[str, Any]]]]:
    """A config's env_wrappers list as [(id, keyword arguments with the reference's defaults filled
    in)] when the device CartPole applies it: empty, or exactly one CartPoleV1_RewardShaper entry
    carrying only the class's own keyword arguments, finite real scales and a bool clip_potential.
    None for any other list (the host env then)."""
    wrappers = list(wrappers or [])
    if not wrappers:
        return []
    if len(wrappers) != 1 or not isinstance(wrappers[0], dict):
        return None
    w = wrappers[0]
    wid = w.get("id")
    if wid not in CARTPOLE_WRAPPERS:
        return None
    kw = dict(CARTPOLE_WRAPPERS[wid])
    for k, v in w.items():
        if k == "id":
            continue
        if k not in kw:
            return None
        kw[k] = v
    if not (_is_real(kw["angle_reward_scale"]) and _is_real(kw["position_reward_scale"])):
        return None
    if not isinstance(kw["clip_potential"], bool):
        return None
    return [(wid, kw)]


BANDIT_MAX_ARMS = 32               # include/gsamd.h GS_BANDIT_MAX_ARMS (csrc/gs_common.h kMaxActions)
BANDIT_KWARGS = ("n_arms", "means", "stds", "episode_length")


def bandit_arms(n_arms: int, means=None, stds=1.0):
    """(means, stds) as the float32 lists MultiArmedBanditEnv keeps (gym_envs/mab_env.py:179-187):
    means default to linspace(0, n_arms, n_arms) in float32, a scalar std is broadcast."""
    import numpy as np
    n = int(n_arms)
    m = np.linspace(0, n, num=n, dtype=np.float32) if means is None else np.asarray(means, dtype=np.float32)
    s = np.full(n, float(stds), dtype=np.float32) if isinstance(stds, (int, float)) else np.asarray(stds, np.float32)
    return m, s


def resolve_bandit_env(cfg) -> Optional[Dict[str, Any]]:
    """What the device Bandit-v0 needs from a config, or None when the device does not build that
    env (the host env then).  env_kwargs may hold only n_arms (an int in [2, 32] equal to the
    spec's action count; default 10), means (None or n_arms finite reals), stds (a finite real
    >= 0 or n_arms of them; default 1.0) and episode_length (an int >= 1; default 1) — a `seed`
    key means the host env; no env_wrappers, no normalize_obs, no frame_stack.
    Returns {n_arms, means, stds, episode_length} with means / stds float32 arrays."""
    if DEVICE_DYNAMICS.get(str(getattr(cfg, "env_id", ""))) != "bandit":
        return None
    if getattr(cfg, "env_wrappers", None) or getattr(cfg, "normalize_obs", False):
        return None
    if getattr(cfg, "frame_stack", None) not in (None, 0, 1):
        return None
    kwargs = getattr(cfg, "env_kwargs", None) or {}
    if not isinstance(kwargs, dict) or set(kwargs) - set(BANDIT_KWARGS):
        return None
    n_arms, length = kwargs.get("n_arms", 10), kwargs.get("episode_length", 1)
    if not (_is_int(n_arms) and 2 <= n_arms <= BANDIT_MAX_ARMS and _is_int(length) and length >= 1):
        return None
    discrete = ((getattr(cfg, "spec", None) or {}).get("action_space") or {}).get("discrete")
    if discrete is None or not _is_int(discrete) or int(discrete) != n_arms:
        return None
    means, stds = kwargs.get("means"), kwargs.get("stds", 1.0)
    if means is not None:
        if not isinstance(means, (list, tuple)) or len(means) != n_arms or not all(_is_real(v) for v in means):
            return None
    if isinstance(stds, (list, tuple)):
        if len(stds) != n_arms or not all(_is_real(v) and v >= 0 for v in stds):
            return None
    elif not (_is_real(stds) and stds >= 0):
        return None
    m, s = bandit_arms(n_arms, means, stds)
    import numpy as np
    if not (np.isfinite(m).all() and np.isfinite(s).all()):      # finite as float32 too
        return None
    return dict(n_arms=int(n_arms), means=m, stds=s, episode_length=int(length))


def device_env_kind(cfg) -> Optional[str]:
    """The device env a config trains on when the caller passes no env: "synthetic",
    "cartpole", "acrobot", "mountaincar", "frozenlake", "taxi", "bandit", or None when the config
    names an env the device does not simulate — the caller then passes the host VectorEnv the
    reference would build (agents/base_agent.py:129-192 → utils/environment.py:421-425
    build_env_from_config).  MountainCar-v0 and CartPole-v1 may carry the env_wrappers the device
    applies itself (resolve_mountaincar_wrappers, resolve_cartpole_wrappers: CartPole-v1's
    CartPoleV1_RewardShaper), FrozenLake-v1 / Taxi-v3 carry exactly the DiscreteEncoder
    (resolve_tabular_env), Bandit-v0 carries the env_kwargs of its arms (resolve_bandit_env); any
    wrapper on another env means the host env."""
    mode = str(getattr(cfg, "env_dynamics", None) or "auto")
    if mode != "auto":
        return mode
    if str(getattr(cfg, "obs_type", "vector")) == "rgb":
        return None
    kind = DEVICE_DYNAMICS.get(str(getattr(cfg, "env_id", "")))
    wrappers = getattr(cfg, "env_wrappers", None)
    if kind in TABULAR_KINDS:       # FrozenLake-v1 / Taxi-v3: the DiscreteEncoder and the map kwargs are the env's own
        ok = (resolve_tabular_env(cfg) is not None and not getattr(cfg, "normalize_obs", False)
              and getattr(cfg, "frame_stack", None) in (None, 0, 1))
        return kind if ok else None
    if kind == "bandit":            # Bandit-v0: the arms' env_kwargs are the env's own
        return kind if resolve_bandit_env(cfg) is not None else None
    if kind == "mountaincar":
        unwrapped = resolve_mountaincar_wrappers(wrappers) is not None
    elif kind == "cartpole":
        unwrapped = resolve_cartpole_wrappers(wrappers) is not None
    else:
        unwrapped = not wrappers
    plain = (unwrapped and not getattr(cfg, "env_kwargs", None)
             and not getattr(cfg, "normalize_obs", False) and getattr(cfg, "frame_stack", None) in (None, 0, 1))
    return kind if plain else None


def needs_host_env(cfg) -> bool:
    """True when build_agent(cfg) needs env= (a gymnasium VectorEnv built on the host).  False for
    every reference config with vector observations and no Box2D / ALE / VizDoom / Retro
    dependency: CartPole-v1 (ppo, ppo_rewardshaped), Acrobot-v1, MountainCar-v0, FrozenLake-v1,
    Taxi-v3 and Bandit-v0 (device_env_kind)."""
    return device_env_kind(from_reference_config(cfg)) is None


def _sanitize(name: str) -> str:
    return re.sub(r"[^A-Za-z0-9_.-]", "-", name)


def canonical_id(env_id: str, variant: Optional[str]) -> Tuple[str, str]:
    """Map BASELINE.json ids onto the reference's config ids."""
    if variant is None and ":" in env_id:
        env_id, variant = env_id.split(":", 1)
    env_id = _ALIASES.get(env_id, env_id)
    if env_id.startswith("ALE/"):
        env_id = "ALE-" + env_id[4:]
        if variant == "ppo":
            variant = "rgb_ppo"
    return env_id, variant or "ppo"


def _collect_yaml(config_dir: str) -> Dict[str, Dict[str, Any]]:
    out: Dict[str, Dict[str, Any]] = {}
    for path in sorted(glob.glob(os.path.join(config_dir, "*.yaml"))):
        with open(path) as f:
            doc = yaml.safe_load(f) or {}
        base: Dict[str, Any] = {}
        if isinstance(doc.get("_base"), dict):
            base.update({k: v for k, v in doc["_base"].items() if k in _YAML_FIELDS})
        base.update({k: v for k, v in doc.items() if k in _YAML_FIELDS})
        for k, v in doc.items():
            if k in _YAML_FIELDS or not isinstance(v, dict) or str(k).startswith("_"):
                continue
            cfg = dict(base)
            cfg.update(v)
            if not cfg.get("project_id"):
                env = cfg.get("env_id", "")
                cfg["project_id"] = f"{env}_{cfg.get('obs_type', 'rgb')}" if env else os.path.splitext(
                    os.path.basename(path))[0]
            keys = {f"{cfg['project_id']}_{k}", f"{_sanitize(cfg['project_id'])}_{k}"}
            if cfg.get("env_id"):
                keys |= {f"{cfg['env_id']}_{k}", f"{_sanitize(cfg['env_id'])}_{k}"}
            for key in keys:
                out.setdefault(key, cfg)
    return out


def load_config(env_id: str, variant: Optional[str] = None, config_dir: Optional[str] = None,
                overrides: Optional[Dict[str, Any]] = None) -> PPOConfig:
    env_id, variant = canonical_id(env_id, variant)
    if config_dir:
        table = _collect_yaml(config_dir)
        raw = dict(table[f"{env_id}_{variant}"])
    else:
        key = f"{env_id}:{variant}"
        if key not in PRESETS:
            raise KeyError(f"no bundled preset for {key}; pass config_dir=<reference>/config/environments")
        raw = dict(PRESETS[key])
    cls = _config_class(raw.get("algo_id", "ppo"))
    raw = {k: v for k, v in raw.items() if k in _fields_of(cls)}
    if cls is REINFORCEConfig:
        # upstream defects of Bandit-v0.yaml's reinforce variant: no model_id (the reference asserts at
        # utils/config.py:463 and cannot start) -> its ppo sibling's mlp_small; n_envs "auto" -> 32
        if not raw.get("model_id"):
            raw["model_id"] = "mlp_small"
        if raw.get("n_envs") in (None, "auto"):
            raw["n_envs"] = 32
    cfg = cls(**raw)
    if overrides:
        cfg = apply_overrides(cfg, overrides)
    return cfg


def apply_overrides(cfg: PPOConfig, overrides: Dict[str, Any]) -> PPOConfig:
    """`--override K=V` (utils/train_launcher.py:81-98): applied after resolution, like the
    reference, but re-validated here (the reference skips re-validation)."""
    for k, v in overrides.items():
        if k not in _fields_of(type(cfg)):
            raise KeyError(f"unknown config field {k!r}")
        cur = getattr(cfg, k)
        if isinstance(v, str) and isinstance(cur, (int, float)) and not isinstance(cur, bool):
            v = type(cur)(float(v)) if isinstance(cur, int) else float(v)
        setattr(cfg, k, v)
    cfg._resolve_numeric_strings()
    cfg._resolve_batch_size()
    cfg.validate()
    return cfg


def from_reference_config(cfg: Any, **extras) -> PPOConfig:
    """Adapt the reference's own Config/PPOConfig object (utils/config.py:17-885) — whatever
    ``agents.build_agent`` received from ``train.py`` — into a PPOConfig, reading the
    fields this path uses by name (enums are reduced to their ``value``)."""
    if isinstance(cfg, PPOConfig):
        return apply_overrides(cfg, extras) if extras else cfg
    from .schedules import SCHEDULABLE, from_attributes
    kw: Dict[str, Any] = {}
    cls = _config_class(getattr(cfg, "algo_id", "ppo"))
    for name in _fields_of(cls):
        if hasattr(cfg, name) and name != "schedules":
            v = getattr(cfg, name)
            kw[name] = getattr(v, "value", v)
    sched = {p: spec for p in SCHEDULABLE if (spec := from_attributes(cfg, p)) is not None}
    if sched:
        kw["schedules"] = sched
    kw.update(extras)
    if cls is REINFORCEConfig:
        kw = {k: v for k, v in kw.items() if v is not None or k in ("max_epochs", "max_env_steps", "target_kl",
                                                                    "frame_stack", "max_episode_steps")}
    return cls(**kw)
