"""CPU checks of the host side of the device envs (gsamd/rollout.py, gsamd/_lib.py): every C entry an
env class calls gets the arguments recorded in tests/golden/device_env_calls.json, each accepted by
the binding's argtype in that position; the binding declares the restypes and argtypes recorded in
tests/golden/lib_argtypes.json; and the collector's two one-launch predicates answer as recorded
below.  Both records were written by tests/golden/make_device_env_calls.py at commit 22dc494, before
the env classes came to state their argument group once."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


# every env and rollout entry of the binding but the Atari env's two
ENV_ENTRIES = (
    "gs_env_reset", "gs_env_step", "gs_rollout_synth",
    "gs_cartpole_reset", "gs_cartpole_step", "gs_acrobot_reset", "gs_acrobot_step", "gs_rollout_env", "gs_rollout1_env",
    "gs_cartpole_shaped_reset", "gs_cartpole_shaped_step", "gs_rollout_cartpole_shaped", "gs_rollout1_cartpole_shaped",
    "gs_mountaincar_reset", "gs_mountaincar_step", "gs_rollout_mountaincar", "gs_rollout1_mountaincar",
    "gs_bandit_reset", "gs_bandit_step", "gs_rollout_bandit", "gs_rollout1_bandit",
    "gs_tabular_reset", "gs_tabular_step", "gs_rollout1_tabular")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded():
    """make_device_env_calls.record_calls(), once: ({case: raw calls}, {case: pointer names})."""
    import make_device_env_calls as G
    return G.record_calls()


def test_every_entry_call_matches_the_record(recorded):
    import make_device_env_calls as G
    raw, names = recorded
    want = _golden("device_env_calls.json")
    assert list(raw) == list(want)
    for case, calls in raw.items():
        got = [{"entry": c["entry"], "check": c["check"], "args": [G.encode(a, names[case]) for a in c["args"]]}
               for c in calls]
        assert [(c["entry"], c["check"]) for c in got] == [(c["entry"], c["check"]) for c in want[case]], case
        for g, w in zip(got, want[case]):
            assert g["args"] == w["args"], (case, g["entry"])
    # through json and back: what the file holds is what calls_record() writes
    assert json.loads(json.dumps(G.calls_record())) == want


def test_every_recorded_call_fits_the_bound_entry(recorded):
    from gsamd._lib import lib
    raw, _ = recorded
    seen = set()
    for case, calls in raw.items():
        for c in calls:
            argtypes = getattr(lib, c["entry"]).argtypes
            assert len(c["args"]) == len(argtypes), (case, c["entry"])
            for i, (a, t) in enumerate(zip(c["args"], argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ValueError) as e:
                    pytest.fail(f"{case}: {c['entry']} argument {i} ({a!r}) is no {t.__name__}: {e}")
            seen.add(c["entry"])
    assert seen == set(ENV_ENTRIES)


def test_binding_declares_the_recorded_types():
    import make_device_env_calls as G
    from gsamd import _lib
    want = _golden("lib_argtypes.json")
    assert G.argtypes_record() == want
    assert set(_lib.EXPORTED) == set(want) and len(_lib.EXPORTED) == len(want)


# (_one_launch_supported, _one_launch_mlp1_supported) per env case and policy, as commit 22dc494 answers
# with the library's host-only queries (gs_rollout_synth_supported / gs_rollout_env_supported /
# gs_rollout1_supported).  The tabular env has no two-hidden-layer one-launch rollout, the synthetic env
# no one-hidden-layer one.
_REAL = {(128, 128): (True, False), (64, 0): (False, True)}
SUPPORT = {
    "cartpole": _REAL, "cartpole_shaped": _REAL, "acrobot": _REAL, "mountaincar": _REAL, "mountaincar_shaper": _REAL,
    "mountaincar_bonus_shaper": _REAL, "bandit": _REAL,
    "tabular_frozenlake": {(128, 128): (False, False), (64, 0): (False, True)},
    "synthetic": {(128, 128): (True, False), (64, 0): (False, False)},
    "object": {(128, 128): (False, False), (64, 0): (False, False)},
}


@pytest.mark.parametrize("case", list(SUPPORT))
def test_one_launch_support_table(case):
    import make_device_env_calls as G
    from gsamd.rollout import DeviceRolloutCollector as C
    env = object() if case == "object" else G.cases()[case]()
    obs_dim, n_actions = (getattr(env, "obs_dim", 4), getattr(env, "n_actions", 2))
    for hidden, want in SUPPORT[case].items():
        pm = G._policy(obs_dim, hidden, n_actions)
        assert (C._one_launch_supported(env, pm), C._one_launch_mlp1_supported(env, pm)) == want, (case, hidden)
    if case == "acrobot":        # an env's cap on the two-hidden-layer form: past it, the step graph
        env.one_launch_max_envs = env.num_envs - 1
        assert C._one_launch_supported(env, G._policy(obs_dim, (128, 128), n_actions)) is False
        env.one_launch_max_envs = env.num_envs
        assert C._one_launch_supported(env, G._policy(obs_dim, (128, 128), n_actions)) is True


def test_masked_policy_is_refused_before_the_env_is_asked():
    import make_device_env_calls as G
    from gsamd.rollout import DeviceRolloutCollector as C
    for hidden in ((128, 128), (64, 0)):
        pm = G._policy(4, hidden, 2)
        pm.valid_mask = 0b11
        assert C._one_launch_supported(object(), pm) is False
        assert C._one_launch_mlp1_supported(object(), pm) is False
