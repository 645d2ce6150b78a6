"""Generate the MountainCar-v0 fixtures FROM THE REFERENCE ITSELF.

Runs ONLY in the build container, where the reference tree is mounted read-only at
/root/reference (like make_golden.py; it never travels to the GPU box).

  mountaincar_wrappers.npz   the reference's own MountainCarV0_RewardShaper and
      MountainCarV0_StateCountBonus classes (gym_wrappers/MountainCarV0/) wrapped around an
      adapter env that replays a trajectory of tests/mountaincar_twin.py (the restated dynamics
      with the device's reset hash), N = 8 envs, S = 240 steps, max_steps = 40.  NEXT_STEP
      autoreset as gymnasium's SyncVectorEnv applies it: the step after a done calls the wrapped
      reset() and emits reward 0.  Every 12 steps the states are re-placed by hand (left wall
      with negative velocity, just below the goal, both speed caps), so that terminations,
      truncations, wall stops, both speed clamps and reset steps all occur (asserted).  Per
      step: the pre-step float64 state, the action, the reset flag and the float32 observation;
      per wrapper config: the reference's rewards and its final count tables.
      The classes only need gymnasium.Wrapper, stubbed here in three lines.  The reference pins
      numpy 1.26.4, where float32 scalar x Python float is float64; this machine's numpy 2
      keeps float32, so the shaper's recorded rewards carry float32 rounding (at most
      (100 + 10 + 50) * 4 * 2^-24 = 3.8e-5).  The bonus' bins must not depend on that: the
      generator asserts that float32 and float64 binning agree on every recorded observation
      and walks the seeds until they do.
  config_mountaincar.json    what the reference's load_config resolves for MountainCar-v0's
      ppo / ppo_rewardshaped / ppo_curiosity.  The reference leaves n_envs at "auto" (the
      host's core count, utils/config.py:482-485); the record keeps "auto", gsamd/presets.py
      takes 32.

Usage: python tests/golden/make_mountaincar_golden.py [wrappers] [configs]
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))

import mountaincar_twin as T  # noqa: E402

N, S, MAX_STEPS, ENV_OFFSET, REPLACE_EVERY = 8, 240, 40, 3, 12
SHAPER = {"id": T.SHAPER, "position_reward_scale": 100.0, "velocity_reward_scale": 10.0, "height_reward_scale": 50.0}
BONUS_A = {"id": T.BONUS, "position_bins": 50, "velocity_bins": 50, "bonus_scale": 0.1, "bonus_type": "count",
           "min_count": 1}
BONUS_B = {"id": T.BONUS, "position_bins": 7, "velocity_bins": 5, "bonus_scale": 1.0, "bonus_type": "inverse",
           "min_count": 2}
BONUS_C = {"id": T.BONUS, "position_bins": 7, "velocity_bins": 5, "bonus_scale": 1.0, "bonus_type": "log",
           "min_count": 1}
CONFIGS = {"shaper": [SHAPER], "bonus_count": [BONUS_A], "bonus_inverse": [BONUS_B], "bonus_log": [BONUS_C],
           "shaper_bonus": [SHAPER, BONUS_A], "bonus_shaper": [BONUS_A, SHAPER]}


def _reference_classes():
    """The two wrapper classes from the reference's files, with gymnasium.Wrapper stubbed and the
    gym_wrappers package entered by path (its __init__ imports every other wrapper's needs)."""
    gym = types.ModuleType("gymnasium")

    class Wrapper:
        def __init__(self, env):
            self.env = env
    gym.Wrapper = Wrapper
    sys.modules["gymnasium"] = gym
    pkg = types.ModuleType("gym_wrappers")
    pkg.__path__ = [os.path.join(REF, "gym_wrappers")]
    sys.modules["gym_wrappers"] = pkg
    from gym_wrappers.MountainCarV0.reward_shaper import MountainCarV0_RewardShaper
    from gym_wrappers.MountainCarV0.state_count_bonus import MountainCarV0_StateCountBonus
    return {T.SHAPER: MountainCarV0_RewardShaper, T.BONUS: MountainCarV0_StateCountBonus}


def _replace(rng, twin, t):
    """Hand-placed states: the cases a free run from the valley does not reach in 240 steps."""
    k = t // REPLACE_EVERY
    for e in range(N):
        case = (e + k) % 8
        if case == 0:
            s = [-1.2 + rng.uniform(0.0, 0.02), -rng.uniform(0.03, 0.07)]      # into the left wall
        elif case == 1:
            s = [0.5 - rng.uniform(0.0, 0.03), rng.uniform(0.035, 0.07)]       # just below the goal, moving right
        elif case == 2:
            s = [rng.uniform(-0.9, -0.3), 0.07]                                  # at the upper speed cap
        elif case == 3:
            s = [rng.uniform(-0.5, 0.2), -0.07]                                  # at the lower speed cap
        elif case == 4:
            s = [rng.uniform(-1.2, 0.6), rng.uniform(-0.07, 0.07)]               # anywhere in the box
        else:
            continue
        twin.state[e] = s


def _trajectory(seed):
    rng = np.random.default_rng(seed)
    twin = T.MountainCarTwin(N, seed=seed, env_offset=ENV_OFFSET, max_steps=MAX_STEPS)
    out = dict(obs0=twin.obs(), state=np.zeros((S, N, 2)), action=np.zeros((S, N), np.int64),
               reset=np.zeros((S, N), bool), obs=np.zeros((S, N, 2), np.float32), done=np.zeros((S, N), bool),
               trunc=np.zeros((S, N), bool))
    cnt = dict(term=0, trunc=0, wall=0, clamp_lo=0, clamp_hi=0, reset=0)
    for t in range(S):
        if t and t % REPLACE_EVERY == 0:
            _replace(rng, twin, t)
        a = rng.integers(0, 3, N)
        # push with the motion most of the time, so that the speed caps are met
        for e in range(N):
            if rng.uniform() < 0.6:
                a[e] = 2 if twin.state[e][1] >= 0 else 0
        out["state"][t] = np.asarray(twin.state)
        out["action"][t] = a
        out["reset"][t] = twin.pending
        _, done, trunc = twin.step(a)
        out["obs"][t] = twin.obs()
        out["done"][t], out["trunc"][t] = done, trunc
        for e in range(N):
            info = twin.infos[e]
            if info == "reset":
                cnt["reset"] += 1
                continue
            for k in ("wall", "clamp_lo", "clamp_hi"):
                cnt[k] += bool(info[k])
            cnt["term"] += bool(done[e] and not trunc[e])
            cnt["trunc"] += bool(trunc[e])
    return out, cnt


def _bins_agree(traj):
    """float32 binning (numpy 2 on the float32 observation) == float64 binning (numpy 1.x, the
    device) on every recorded observation, for every bin shape of CONFIGS."""
    for pb, vb in ((50, 50), (7, 5)):
        kw = {"position_bins": pb, "velocity_bins": vb}
        for o in traj["obs"].reshape(-1, 2):
            p32, v32 = np.float32(o[0]), np.float32(o[1])
            pn = np.clip((p32 - (-1.2)) / (0.6 - (-1.2)), 0.0, 0.999999)
            vn = np.clip((v32 - (-0.07)) / (0.07 - (-0.07)), 0.0, 0.999999)
            if (int(pn * pb), int(vn * vb)) != T.bins_of(kw, float(o[0]), float(o[1])):
                return False
    return True


class _Replay:
    """The adapter env of one env index: reset() / step() hand out the recorded observations."""

    def __init__(self, traj, e):
        self.traj, self.e, self.t = traj, e, -1

    def reset(self, **kwargs):
        o = self.traj["obs0"][self.e] if self.t < 0 else self.traj["obs"][self.t][self.e]
        return o.copy(), {}

    def step(self, action):
        t, e = self.t, self.e
        term = bool(self.traj["done"][t][e] and not self.traj["trunc"][t][e])
        return self.traj["obs"][t][e].copy(), -1.0, term, bool(self.traj["trunc"][t][e]), {}


def _run_reference(classes, traj, wrappers):
    """(rewards [S][N] float32, final tables [N][PB*VB] or None) of the reference's stack."""
    rewards = np.zeros((S, N), np.float32)
    tables = None
    for e in range(N):
        base = env = _Replay(traj, e)
        bonus = None
        for w in wrappers:           # first entry innermost (utils/environment.py applies them in list order)
            env = classes[w["id"]](env, **{k: v for k, v in w.items() if k != "id"})
            if w["id"] == T.BONUS:
                bonus = env
        env.reset()
        for t in range(S):
            base.t = t
            if traj["reset"][t][e]:          # SyncVectorEnv, AutoresetMode.NEXT_STEP
                env.reset()
                rewards[t][e] = 0.0
            else:
                _, r, _, _, _ = env.step(int(traj["action"][t][e]))
                rewards[t][e] = np.float32(r)
        if bonus is not None:
            if tables is None:
                tables = np.zeros((N, bonus.state_counts.size), np.int32)
            tables[e] = bonus.state_counts.reshape(-1)
    return rewards, tables


def make_wrappers():
    classes = _reference_classes()
    for seed in range(1, 200):
        traj, cnt = _trajectory(seed)
        if all(v >= 1 for v in cnt.values()) and _bins_agree(traj):
            break
    else:
        raise SystemExit("no seed with full coverage and agreeing bins")
    assert all(v >= 1 for v in cnt.values()), cnt
    assert _bins_agree(traj)
    out = dict(seed=np.int64(seed), env_offset=np.int64(ENV_OFFSET), max_steps=np.int64(MAX_STEPS),
               obs0=traj["obs0"], state=traj["state"], action=traj["action"], reset=traj["reset"], obs=traj["obs"],
               done=traj["done"], trunc=traj["trunc"], coverage=np.array(json.dumps(cnt)),
               configs=np.array(json.dumps(CONFIGS)))
    for name, wrappers in CONFIGS.items():
        rewards, tables = _run_reference(classes, traj, wrappers)
        out[f"reward_{name}"] = rewards
        if tables is not None:
            out[f"table_{name}"] = tables
    np.savez_compressed(os.path.join(HERE, "mountaincar_wrappers.npz"), **out)
    print("mountaincar_wrappers.npz written: seed", seed, "coverage", cnt)


def make_configs():
    """Every field of the Config object the reference's load_config resolves for the three
    MountainCar-v0 variants (as make_golden.make_configs_full), n_envs kept at "auto"."""
    import dataclasses
    sys.path.insert(0, HERE)
    for name in [m for m in sys.modules if m.split(".")[0] in ("gymnasium", "gym_wrappers")]:
        del sys.modules[name]     # make_wrappers' minimal stubs: make_golden brings its own
    import make_golden as G      # its import stubs for the packages the reference's utils need
    out = {}
    for var in ("ppo", "ppo_rewardshaped", "ppo_curiosity"):
        c = G.load_config("MountainCar-v0", var)
        d = {k: getattr(v, "value", v) for k, v in dataclasses.asdict(c).items()}
        d["algo_id"] = c.algo_id
        assert d["n_envs"] == (os.cpu_count() or 1)      # "auto" resolved on this host
        d["n_envs"] = "auto"
        out[f"MountainCar-v0:{var}"] = json.loads(json.dumps(d, default=lambda o: getattr(o, "value", str(o))))
    with open(os.path.join(HERE, "config_mountaincar.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("config_mountaincar.json written")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["wrappers", "configs"]):
        globals()[f"make_{name}"]()
