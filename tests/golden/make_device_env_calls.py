"""Record what the device env classes hand to the C entries, and what the binding declares.

Writes next to this script:

  device_env_calls.json   per case, every call a device env class of gsamd.rollout makes on
                          reset / step_into / rollout_into / rollout1_into: the entry's name, the
                          name given to `check`, and the argument list.  An integer equal to a known
                          tensor's data_ptr() is written as that tensor's name ("env.state",
                          "buf.rewards", "pm.params", "rewards_row", ...), the stream constant as
                          "stream", a ctypes structure as its type and bytes, None as null.
  lib_argtypes.json       for every entry the binding declares (gsamd._lib.EXPORTED), the names of
                          its restype and argtypes in order.

Nothing here needs a GPU: gsamd.rollout.lib is replaced by a recorder that returns 0,
gsamd.rollout.stream_handle by a constant, and every tensor lives on the CPU.  Only the built
library has to be present (gsamd._lib loads it on import).  tests/test_device_env_calls_cpu.py
regenerates both records in memory and requires equality with the files, so they are written once,
before a change to the host side of the envs, and not again.

Usage: python tests/golden/make_device_env_calls.py
"""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gymnasium-solver_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

N_ENVS, T = 4, 3
STREAM = 0x57EA0000                     # what stream_handle() answers here
MODE, RNG_SEED, COUNTER0 = 1, 99, 21    # rollout_into's mode / rng_seed / counter0
SEED, ENV_OFFSET = 11, 8                # distinct, so a swapped position shows
CP_SHAPER = {"id": "CartPoleV1_RewardShaper"}
MC_SHAPER = {"id": "MountainCarV0_RewardShaper"}
MC_BONUS = {"id": "MountainCarV0_StateCountBonus", "position_bins": 12, "velocity_bins": 10}


# the classes without a gs_rollout_* / gs_rollout1_* entry: that method is not called on them
NO_ROLLOUT, NO_ROLLOUT1 = ("tabular_frozenlake",), ("synthetic",)


class Recorder:
    """Stands in for gsamd.rollout.lib and gsamd.rollout.check: every entry returns 0 and is
    booked with its arguments; check books the name it was given next to the last call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append({"entry": name, "check": None, "args": args})
            return 0
        return entry

    def check(self, rc, what=""):
        assert rc == 0
        self.calls[-1]["check"] = what


def _tensors(prefix, obj):
    return {t.data_ptr(): f"{prefix}.{k}" for k, t in vars(obj).items() if torch.is_tensor(t) and t.numel()}


def encode(arg, names):
    if isinstance(arg, ctypes.Structure):
        return {"struct": type(arg).__name__, "bytes": bytes(arg).hex()}
    if isinstance(arg, int) and not isinstance(arg, bool) and arg in names:
        return names[arg]
    assert arg is None or isinstance(arg, (int, float)), arg
    return arg


def _policy(obs_dim, hidden, n_actions):
    from gsamd._lib import MlpDims
    return SimpleNamespace(params=torch.zeros(8), dims=MlpDims(obs_dim, hidden[0], hidden[1], n_actions))


def _drive(env, case):
    """The calls of one case, in a fixed order; the tensors' names for encode()."""
    synthetic = case == "synthetic"
    from gsamd.rollout import DeviceRolloutBuffer
    buf = DeviceRolloutBuffer(N_ENVS, env.obs_shape, T, "cpu")
    pm, pm1 = _policy(env.obs_dim, (128, 128), env.n_actions), _policy(env.obs_dim, (64, 0), env.n_actions)
    rows = SimpleNamespace(rewards_row=torch.zeros(N_ENVS), dones_row=torch.zeros(N_ENVS, dtype=torch.uint8),
                           timeouts_row=torch.zeros(N_ENVS, dtype=torch.uint8),
                           actions=torch.zeros(N_ENVS, dtype=torch.int64), clock=torch.zeros(2, dtype=torch.int64))
    names = {STREAM: "stream", **_tensors("env", env), **_tensors("buf", buf), **_tensors("pm", pm),
             **_tensors("pm", pm1),
             **{p: k.split(".")[1] for p, k in _tensors("rows", rows).items()}}
    step = (rows.rewards_row, rows.dones_row, rows.timeouts_row)
    env.reset()
    env.step_into(*step, actions=rows.actions)
    if synthetic:
        env.step_into(*step)
        env.step_into(*step, actions=rows.actions, clock=rows.clock, step=2)
    if case not in NO_ROLLOUT:
        for _ in range(2 if synthetic else 1):      # twice: the synthetic env's step_count advances
            env.rollout_into(pm, buf, MODE, RNG_SEED, COUNTER0)
    if case not in NO_ROLLOUT1:
        env.rollout1_into(pm1, buf, MODE, RNG_SEED, COUNTER0)
    return names, (env, buf, pm, pm1, rows)


def cases():
    """name -> a function building the case's env on the CPU."""
    from gsamd import rollout as R
    kw = dict(seed=SEED, env_offset=ENV_OFFSET, device="cpu")
    return {
        "cartpole": lambda: R.DeviceCartPoleVecEnv(N_ENVS, max_steps=7, **kw),
        "cartpole_shaped": lambda: R.DeviceCartPoleVecEnv(N_ENVS, max_steps=7, wrappers=[CP_SHAPER], **kw),
        "acrobot": lambda: R.DeviceAcrobotVecEnv(N_ENVS, max_steps=9, **kw),
        "mountaincar": lambda: R.DeviceMountainCarVecEnv(N_ENVS, max_steps=13, **kw),
        "mountaincar_shaper": lambda: R.DeviceMountainCarVecEnv(N_ENVS, max_steps=13, wrappers=[MC_SHAPER], **kw),
        "mountaincar_bonus_shaper": lambda: R.DeviceMountainCarVecEnv(N_ENVS, max_steps=13,
                                                                      wrappers=[MC_BONUS, MC_SHAPER], **kw),
        "bandit": lambda: R.DeviceBanditVecEnv(N_ENVS, n_arms=4, episode_length=8, max_steps=5, **kw),
        "tabular_frozenlake": lambda: R.DeviceTabularVecEnv(N_ENVS, kind="frozenlake", encoding="binary",
                                                            max_steps=17, **kw),
        "synthetic": lambda: R.DeviceSyntheticVecEnv(N_ENVS, 5, 3, episode_len=6, truncate_every=4, reward=0.5, **kw),
    }


def record_calls():
    """{case: [raw call, ...]} and {case: names}: the raw argument tuples (for the argtype checks)
    and the pointer names that encode() writes in their place."""
    from gsamd import rollout as R
    saved = R.lib, R.stream_handle, R.check
    raw, names, keep = {}, {}, []
    try:
        for case, make in cases().items():
            rec = Recorder()
            R.lib, R.stream_handle, R.check = rec, (lambda stream=None: STREAM), rec.check
            names[case], alive = _drive(make(), case)
            keep.append(alive)           # no tensor of an earlier case is freed and its address reused
            raw[case] = rec.calls
    finally:
        R.lib, R.stream_handle, R.check = saved
    return raw, names


def calls_record():
    """device_env_calls.json's content."""
    raw, names = record_calls()
    return {case: [{"entry": c["entry"], "check": c["check"], "args": [encode(a, names[case]) for a in c["args"]]}
                   for c in calls] for case, calls in raw.items()}


def argtypes_record():
    """lib_argtypes.json's content."""
    from gsamd import _lib
    name = lambda t: None if t is None else t.__name__        # noqa: E731
    return {e: {"restype": name(getattr(_lib.lib, e).restype),
                "argtypes": [name(t) for t in getattr(_lib.lib, e).argtypes]} for e in sorted(_lib.EXPORTED)}


if __name__ == "__main__":
    for fname, content in (("device_env_calls.json", calls_record()), ("lib_argtypes.json", argtypes_record())):
        with open(os.path.join(HERE, fname), "w") as f:
            json.dump(content, f, indent=1)
            f.write("\n")
        print("wrote", fname)
