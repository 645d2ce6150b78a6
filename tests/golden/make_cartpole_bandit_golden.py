"""Generate the CartPole-v1 reward-shaper and Bandit-v0 fixtures FROM THE REFERENCE ITSELF.

Runs ONLY in the build container, where the reference tree is mounted read-only at
/root/reference (like make_golden.py; it never travels to the GPU box).

  cartpole_shaper.npz   the reference's own CartPoleV1_RewardShaper (gym_wrappers/CartPoleV1/
      reward_shaper.py) wrapped around an adapter env that replays steps of oracle/cartpole_ref.py
      (the restated dynamics with the device's reset hash), N = 37 envs, S = 24 steps,
      max_steps = 3.  The run is teacher-forced: before every step each env's float64 state is
      drawn anew, over the whole box and beyond both thresholds, so that clipped potentials,
      terminations, truncations and reset rows all occur (asserted: per parameter set at least 10
      rows with a potential term outside [0, 1] and at least 5 terminations).  NEXT_STEP
      autoreset as gymnasium's SyncVectorEnv applies it: the step after a done calls the wrapped
      reset() and emits reward 0.  Per step: the pre-step state, the action, the reset flag, the
      float32 observation and the done / trunc flags; per parameter set the class's rewards as
      float32.  The adapter carries x_threshold and theta_threshold_radians as gymnasium's
      CartPoleEnv defines them (2.4, 12 * 2 * pi / 360), which the class reads from env.unwrapped.
  bandit_env.npz        from the reference's MultiArmedBanditEnv (gym_envs/mab_env.py): its float32
      means / stds for (n_arms = 10, the yaml's lists) and for (n_arms = 4, defaults), the
      observation's shape and dtype, and the terminated pattern for episode_length 1 and 3 over 7
      steps (reset() after a termination).  Its rewards come from numpy's PCG64 stream and are
      not a target.
  config_cartpole_bandit.json   what the reference's load_config resolves for
      CartPole-v1:ppo_rewardshaped and Bandit-v0:ppo.  The reference leaves Bandit-v0's n_envs at
      "auto" (the host's core count, utils/config.py:482-485); the record keeps "auto",
      gsamd/presets.py takes 32.

Usage: python tests/golden/make_cartpole_bandit_golden.py [shaper] [bandit] [configs]
"""
from __future__ import annotations

import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

N, S, MAX_STEPS, ENV_OFFSET, SEED = 37, 24, 3, 5, 11
PARAMS = {"default": dict(angle_reward_scale=1.0, position_reward_scale=0.25, clip_potential=True),
          "scaled": dict(angle_reward_scale=2.0, position_reward_scale=0.5, clip_potential=True),
          "noclip": dict(angle_reward_scale=1.0, position_reward_scale=0.25, clip_potential=False)}
X_THR, TH_THR = 2.4, 12 * 2 * math.pi / 360
CONFIG_IDS = (("CartPole-v1", "ppo_rewardshaped"), ("Bandit-v0", "ppo"))
BANDIT_YAML = dict(n_arms=10, means=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], stds=1, episode_length=1)   # Bandit-v0.yaml:37-41


def _stub_gymnasium():
    gym = types.ModuleType("gymnasium")
    spaces = types.ModuleType("gymnasium.spaces")

    class Wrapper:
        def __init__(self, env):
            self.env = env

    class Env:
        pass

    class Discrete:
        def __init__(self, n):
            self.n = int(n)

        def contains(self, a):
            return 0 <= int(a) < self.n

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

    gym.Wrapper, gym.Env, gym.spaces = Wrapper, Env, spaces
    spaces.Discrete, spaces.Box = Discrete, Box
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, spaces
    for pkg in ("gym_wrappers", "gym_envs"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, pkg)]      # entered by path: the packages' __init__ import far more
        sys.modules[pkg] = m


def _unstub():
    for name in [m for m in sys.modules if m.split(".")[0] in ("gymnasium", "gym_wrappers", "gym_envs", "PIL")]:
        del sys.modules[name]


# ---------------------------------------------------------------------------- the shaper
def _draw_state(rng, e, t):
    """A pre-step state: most inside the box, the rest beyond the position or the angle threshold
    (on either side), or both."""
    case = (e + 3 * t) % 7
    x = rng.uniform(-2.0, 2.0)
    th = rng.uniform(-0.15, 0.15)
    if case == 0:
        x = rng.choice([-1.0, 1.0]) * rng.uniform(2.42, 3.0)
    elif case == 1:
        th = rng.choice([-1.0, 1.0]) * rng.uniform(0.215, 0.35)
    elif case == 2 and t % 2:
        x, th = rng.choice([-1.0, 1.0]) * rng.uniform(2.42, 2.6), rng.choice([-1.0, 1.0]) * rng.uniform(0.215, 0.3)
    return [x, rng.uniform(-2.0, 2.0), th, rng.uniform(-1.5, 1.5)]


def _trajectory():
    from oracle.cartpole_ref import CartPoleTwin
    rng = np.random.default_rng(SEED)
    twin = CartPoleTwin(N, seed=SEED, env_offset=ENV_OFFSET, max_steps=MAX_STEPS)
    out = dict(obs0=twin.obs(), state=np.zeros((S, N, 4)), action=np.zeros((S, N), np.int64),
               reset=np.zeros((S, N), bool), obs=np.zeros((S, N, 4), np.float32), done=np.zeros((S, N), bool),
               trunc=np.zeros((S, N), bool))
    for t in range(S):
        for e in range(N):
            twin.state[e] = _draw_state(rng, e, t)       # ignored by an env whose reset is pending
        out["state"][t] = np.asarray(twin.state)
        out["action"][t] = rng.integers(0, 2, N)
        out["reset"][t] = twin.pending
        _, done, trunc = twin.step(out["action"][t])
        out["obs"][t], out["done"][t], out["trunc"][t] = twin.obs(), done, trunc
    return out


class _Replay:
    """The adapter env of one env index: reset() / step() hand out the recorded observations."""
    x_threshold, theta_threshold_radians = X_THR, TH_THR

    def __init__(self, traj, e):
        self.traj, self.e, self.t = traj, e, -1
        self.unwrapped = self

    def reset(self, **kwargs):
        o = self.traj["obs0"][self.e] if self.t < 0 else self.traj["obs"][self.t][self.e]
        return o.copy(), {}

    def step(self, action):
        t, e = self.t, self.e
        term = bool(self.traj["done"][t][e] and not self.traj["trunc"][t][e])
        return self.traj["obs"][t][e].copy(), 1.0, term, bool(self.traj["trunc"][t][e]), {}


def make_shaper():
    _stub_gymnasium()
    from gym_wrappers.CartPoleV1.reward_shaper import CartPoleV1_RewardShaper
    traj = _trajectory()
    live = ~traj["reset"]
    term = traj["done"] & ~traj["trunc"] & live
    pos = 1.0 - np.abs(traj["obs"][..., 0].astype(np.float64)) / X_THR
    ang = 1.0 - np.abs(traj["obs"][..., 2].astype(np.float64)) / TH_THR
    clipped = live & ((pos < 0) | (pos > 1) | (ang < 0) | (ang > 1))
    cover = dict(clipped=int(clipped.sum()), terminated=int(term.sum()), truncated=int((traj["trunc"] & live).sum()),
                 reset=int(traj["reset"].sum()), pos_clipped=int((live & (pos < 0)).sum()),
                 ang_clipped=int((live & (ang < 0)).sum()))
    assert cover["clipped"] >= 10 and cover["terminated"] >= 5 and cover["truncated"] >= 1 and cover["reset"] >= 5, cover
    assert cover["pos_clipped"] >= 5 and cover["ang_clipped"] >= 5, cover
    out = dict(seed=np.int64(SEED), env_offset=np.int64(ENV_OFFSET), max_steps=np.int64(MAX_STEPS), obs0=traj["obs0"],
               state=traj["state"], action=traj["action"], reset=traj["reset"], obs=traj["obs"], done=traj["done"],
               trunc=traj["trunc"], coverage=np.array(json.dumps(cover)), params=np.array(json.dumps(PARAMS)))
    for name, kw in PARAMS.items():
        rewards = np.zeros((S, N), np.float32)
        for e in range(N):
            base = _Replay(traj, e)
            env = CartPoleV1_RewardShaper(base, **kw)
            env.reset()
            for t in range(S):
                base.t = t
                if traj["reset"][t][e]:          # SyncVectorEnv, AutoresetMode.NEXT_STEP
                    env.reset()
                    rewards[t][e] = 0.0
                else:
                    rewards[t][e] = np.float32(env.step(int(traj["action"][t][e]))[1])
        out[f"reward_{name}"] = rewards
    np.savez_compressed(os.path.join(HERE, "cartpole_shaper.npz"), **out)
    print("cartpole_shaper.npz written: coverage", cover)
    _unstub()


# ---------------------------------------------------------------------------- the bandit
def make_bandit():
    _stub_gymnasium()
    pil = types.ModuleType("PIL")
    pil.Image = types.ModuleType("PIL.Image")
    sys.modules["PIL"], sys.modules["PIL.Image"] = pil, pil.Image
    sys.path.insert(0, REF)
    try:
        from gym_envs.mab_env import MultiArmedBanditEnv
    finally:
        sys.path.remove(REF)
    out = {}
    for tag, kw in (("yaml10", BANDIT_YAML), ("default4", dict(n_arms=4))):
        env = MultiArmedBanditEnv(**kw, seed=0)
        obs, _ = env.reset()
        assert not obs.any()
        out[f"means_{tag}"], out[f"stds_{tag}"] = env._means.copy(), env._stds.copy()
        out[f"obs_shape_{tag}"] = np.asarray(obs.shape, np.int64)
        out[f"obs_dtype_{tag}"] = np.array(str(obs.dtype))
        out[f"kwargs_{tag}"] = np.array(json.dumps(kw))
    for length in (1, 3):
        env = MultiArmedBanditEnv(n_arms=4, episode_length=length, seed=0)
        env.reset()
        pattern = []
        for _ in range(7):
            obs, _, terminated, truncated, _ = env.step(1)
            assert not obs.any() and truncated is False
            pattern.append(bool(terminated))
            if terminated:
                env.reset()
        out[f"terminated_len{length}"] = np.asarray(pattern)
    np.savez_compressed(os.path.join(HERE, "bandit_env.npz"), **out)
    print("bandit_env.npz written:", {k: (v.shape, str(v.dtype)) for k, v in out.items()})
    _unstub()


# ---------------------------------------------------------------------------- the configs
def make_configs():
    """Every field of the Config object the reference's load_config resolves for the two ids (as
    make_golden.make_configs_full), Bandit-v0's n_envs kept at "auto", plus the derived hidden_dims
    and action count the preset test reads."""
    import dataclasses
    sys.path.insert(0, HERE)
    _unstub()
    import make_golden as G      # its import stubs for the packages the reference's utils need
    out = {}
    for env, var in CONFIG_IDS:
        c = G.load_config(env, var)
        d = {k: getattr(v, "value", v) for k, v in dataclasses.asdict(c).items()}
        d["algo_id"] = c.algo_id
        if env == "Bandit-v0":
            assert d["n_envs"] == (os.cpu_count() or 1)      # "auto" resolved on this host
            d["n_envs"] = "auto"
        # a scheduled hyper-parameter's resolved attributes are set on the object, not dataclass fields
        d.update({k: v for k, v in vars(c).items() if "_schedule" in k and not k.startswith("_")})
        d["_hidden_dims"] = list(c.hidden_dims)
        d["_n_actions"] = c.spec.get("action_space", {}).get("discrete")
        out[f"{env}:{var}"] = json.loads(json.dumps(d, default=lambda o: getattr(o, "value", str(o))))
    with open(os.path.join(HERE, "config_cartpole_bandit.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("config_cartpole_bandit.json written")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["shaper", "bandit", "configs"]):
        globals()[f"make_{name}"]()
