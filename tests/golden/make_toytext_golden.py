"""Generate the FrozenLake-v1 / Taxi-v3 fixtures FROM THE REFERENCE ITSELF.

Runs ONLY in the build container, where the reference tree is mounted read-only at
/root/reference (like make_golden.py; it never travels to the GPU box).

  discrete_encoder.npz   the reference's own DiscreteEncoder.observation(s)
      (gym_wrappers/discrete_encoder.py) for every state s of n = 16, 64 and 500 under each of
      its three encodings, as the class returns them: `array_<n>` int64 (n, 1) (the wrapper keeps
      the Discrete space's dtype there), `binary_<n>` float32 (n, n_bits), `onehot_<n>` float32
      (n, n).  The class only needs gymnasium.ObservationWrapper and the two space classes it
      names, stubbed here in a few lines.
  config_toytext.json    what the reference's load_config resolves for FrozenLake-v1's ppo /
      ppo_deterministic and Taxi-v3's ppo.  The reference leaves n_envs at "auto" (the host's
      core count, utils/config.py:482-485); the record keeps "auto", gsamd/presets.py takes 32.

Usage: python tests/golden/make_toytext_golden.py [encoder] [configs]
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

SIZES = (16, 64, 500)
ENCODINGS = ("array", "binary", "onehot")
CONFIG_IDS = (("FrozenLake-v1", "ppo"), ("FrozenLake-v1", "ppo_deterministic"), ("Taxi-v3", "ppo"))


def _reference_encoder():
    """DiscreteEncoder from the reference's file, with gymnasium stubbed and the gym_wrappers
    package entered by path (its __init__ imports every other wrapper's needs)."""
    gym = types.ModuleType("gymnasium")
    spaces = types.ModuleType("gymnasium.spaces")

    class ObservationWrapper:
        def __init__(self, env):
            self.env = env

    class Discrete:
        def __init__(self, n):
            self.n, self.dtype = int(n), np.dtype(np.int64)

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.dtype(dtype)

    gym.ObservationWrapper, gym.spaces = ObservationWrapper, spaces
    spaces.Discrete, spaces.Box = Discrete, Box
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, spaces
    pkg = types.ModuleType("gym_wrappers")
    pkg.__path__ = [os.path.join(REF, "gym_wrappers")]
    sys.modules["gym_wrappers"] = pkg
    from gym_wrappers.discrete_encoder import DiscreteEncoder
    return DiscreteEncoder, Discrete


def make_encoder():
    DiscreteEncoder, Discrete = _reference_encoder()
    out = {}
    for n in SIZES:
        env = types.SimpleNamespace(observation_space=Discrete(n))
        for enc in ENCODINGS:
            w = DiscreteEncoder(env, encoding=enc)
            rows = np.stack([w.observation(s) for s in range(n)])
            assert rows.shape == (n,) + tuple(w.observation_space.shape)
            out[f"{enc}_{n}"] = rows
    # the class default (a config entry without `encoding`) is binary
    assert DiscreteEncoder(types.SimpleNamespace(observation_space=Discrete(16))).encoding == "binary"
    np.savez_compressed(os.path.join(HERE, "discrete_encoder.npz"), **out)
    print("discrete_encoder.npz written:", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


def make_configs():
    """Every field of the Config object the reference's load_config resolves for the three ids
    (as make_golden.make_configs_full), n_envs kept at "auto", plus the derived hidden_dims and
    action count the preset test reads."""
    import dataclasses
    sys.path.insert(0, HERE)
    for name in [m for m in sys.modules if m.split(".")[0] in ("gymnasium", "gym_wrappers")]:
        del sys.modules[name]     # make_encoder's minimal stubs: make_golden brings its own
    import make_golden as G      # its import stubs for the packages the reference's utils need
    out = {}
    for env, var in CONFIG_IDS:
        c = G.load_config(env, var)
        d = {k: getattr(v, "value", v) for k, v in dataclasses.asdict(c).items()}
        d["algo_id"] = c.algo_id
        assert d["n_envs"] == (os.cpu_count() or 1)      # "auto" resolved on this host
        d["n_envs"] = "auto"
        d["_hidden_dims"] = list(c.hidden_dims)
        d["_n_actions"] = c.spec.get("action_space", {}).get("discrete")
        d["_valid_actions"] = c.spec.get("action_space", {}).get("valid")
        out[f"{env}:{var}"] = json.loads(json.dumps(d, default=lambda o: getattr(o, "value", str(o))))
    with open(os.path.join(HERE, "config_toytext.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("config_toytext.json written")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["encoder", "configs"]):
        globals()[f"make_{name}"]()
