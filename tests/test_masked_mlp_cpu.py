"""The masked-categorical head of the MLP policies, the part that needs no GPU: the float64 twin
(tests/masked_mlp_twin.py) against the reference's own MLPActorCritic(valid_actions=[0, 3, 4])
(tests/golden/masked_mlp.npz, written by tests/golden/make_masked_mlp_golden.py), the three new C
entries, the host package's argument checks and routing, and the two Pong-objects presets against the
reference's resolved configs (tests/golden/config_pong_objects.json)."""
import dataclasses
import json
import os
import re

import numpy as np
import pytest

import masked_mlp_twin as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = {"gs_policy_act_masked": "gs_policy_act", "gs_ppo_rows_update_masked": "gs_ppo_rows_update",
               "gs_ppo_rows_loss_masked": "gs_ppo_rows_loss"}
PRESET_IDS = ("ALE-Pong-v5:objects_ppo", "ALE-Pong-v5:objects_deterministic_ppo")


@pytest.mark.parametrize("tag", ["small", "tiny"])
def test_twin_reproduces_the_reference_fixture(tag):
    """The float64 twin on the fixture's float32 weights and batch against what the reference computed
    in float32: loss, metrics, per-row log-probs and entropies, the parameter gradient, and
    policy_act(deterministic=True).  The printed deviations are how far the fp32 reference sits from
    the twin; the bars are fp32 rounding of these O(1) quantities over a 64-row mean and a
    128-term dot product (1e-6 relative to the largest entry, ~10 ulp)."""
    f = TW.fixture(tag)
    dims, valid = f["dims"], f["valid"]
    assert valid == (0, 3, 4)
    b = {k[6:]: f[k] for k in f if k.startswith("batch/")}
    assert set(np.unique(b["actions"]).tolist()) == set(valid)
    loss, met, g, lp, H = TW.loss_and_grads(f["p0"], dims, valid, b["observations"], b["actions"], b["logprobs"],
                                            b["values"], b["advantages"], b["returns"], **TW.FIXTURE_HP)
    ref = dict(zip(f["metric_names"].tolist(), f["metric_values"].tolist()))
    gmax = np.abs(f["grads"]).max()
    dev = {"loss rel": abs(loss - float(f["loss"])) / abs(loss),
           "entropy abs": abs(met["opt/policy/entropy"] - ref["opt/policy/entropy"]),
           "logprob abs": np.abs(lp - f["new_logprobs"]).max(),
           "entropy rows abs": np.abs(H - f["entropy_rows"]).max(),
           "grad / max": np.abs(g - f["grads"]).max() / gmax}
    print("MEASURED %s twin - fixture: %s" % (tag, ", ".join("%s %.2e" % kv for kv in dev.items())))
    assert dev["loss rel"] < 1e-6 and dev["entropy abs"] < 1e-6 and dev["logprob abs"] < 2e-6
    assert dev["entropy rows abs"] < 2e-6 and dev["grad / max"] < 1e-6
    for key in ("opt/loss/policy", "opt/loss/value", "opt/ppo/clip_fraction", "opt/ppo/clip_fraction_vf",
                "opt/value/explained_var", "opt/ppo/kl", "opt/ppo/approx_kl"):
        np.testing.assert_allclose(met[key], ref[key], rtol=1e-5, atol=2e-6, err_msg=key)
    assert met["opt/policy/entropy"] <= np.log(3) + 1e-6
    # the invalid actions' rows of the policy head: an exactly zero gradient on both sides
    inv = TW.invalid_slices(dims, valid)
    assert inv.size == 15 * (dims[-2] + 1) and not f["grads"][inv].any() and not g[inv].any()
    # policy_act(deterministic=True): the first maximum among the valid actions, its log-prob, the value
    value, ln, amax = TW.act(f["p0"], dims, valid, b["observations"])
    assert np.array_equal(amax, f["act/actions"]) and set(amax.tolist()) <= set(valid)
    np.testing.assert_allclose(ln[np.arange(64), amax], f["act/logprobs"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(value, f["act/values"], rtol=0, atol=2e-6)
    assert np.isneginf(ln[:, [a for a in range(dims[-1]) if a not in valid]]).all()


def test_twin_entropy_is_the_masked_formula():
    """One valid action: the entropy is -log(1 + 1e-8), no logit moves; all actions valid: the masked
    formula -sum p log(p + 1e-8), which is not Categorical's -sum p log p."""
    c = TW.case((8, 64, 64, 6), (2,), 1, 64, 7)
    r = np.arange(64)
    _, met, g, lp, H = TW.loss_and_grads(c["p0"], c["dims"], c["valid"], c["obs"], c["actions"], c["old_logp"],
                                         c["old_values"], c["adv"], c["ret"], **TW.HP)
    assert not lp.any() and np.allclose(H, -np.log1p(1e-8), rtol=1e-6, atol=0)
    G = __import__("oracle.ppo_ref", fromlist=["x"]).unflatten(g, c["dims"])
    assert not G["policy_head.weight"].any() and not G["policy_head.bias"].any() and G["value_head.weight"].any()
    full = TW.case((8, 64, 64, 6), tuple(range(6)), 1, 64, 7)
    _, _, _, _, H6 = TW.loss_and_grads(full["p0"], full["dims"], full["valid"], full["obs"], full["actions"],
                                       full["old_logp"], full["old_values"], full["adv"], full["ret"], **TW.HP)
    _, ln, _ = TW.act(full["p0"], full["dims"], full["valid"], full["obs"])
    p = np.exp(ln)
    np.testing.assert_allclose(H6, -(p * np.log(p + 1e-8)).sum(1), rtol=1e-12)
    assert (H6[r] < -(p * ln).sum(1)).all()


def test_header_bindings_and_library_export_the_new_entries():
    from gsamd import _lib
    src = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", plain))
    assert declared == set(_lib.EXPORTED)
    args = lambda name: [re.sub(r"\s*\w+$", "", a.strip()) for a in  # noqa: E731  (the C types, names dropped)
                         re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1).split(",")]
    for new, old in NEW_ENTRIES.items():
        assert new in declared and new in _lib.EXPORTED and hasattr(_lib.lib, new), new
        # the unmasked sibling's list and one uint32_t valid_mask behind it
        assert args(new) == args(old) + ["uint32_t"], new
        assert list(getattr(_lib.lib, new).argtypes) == list(getattr(_lib.lib, old).argtypes) + [_lib.ctypes.c_uint32]
    assert _lib.lib.gs_abi_version() == _lib.GS_ABI_VERSION == 7 and re.search(r"#define GS_ABI_VERSION 7\b", src)
    assert _lib.ctypes.sizeof(_lib.MlpDims) == 16 and _lib.ctypes.sizeof(_lib.PPOHparams) == 48


def test_bad_masks_are_refused_before_any_launch():
    """Bits at or beyond n_actions: GS_E_INVALID from the three entries with no device in sight."""
    from gsamd._lib import MlpDims, PPOHparams, RolloutView, check, lib
    hp = PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, 0)
    for dims, mask in ((MlpDims(12, 128, 128, 18), 1 << 18), (MlpDims(12, 64, 0, 18), 0x80000000),
                       (MlpDims(8, 64, 64, 6), 0b1000001)):
        with pytest.raises(ValueError, match="valid_mask 0x[0-9a-f]+ has bits past n_actions"):
            check(lib.gs_policy_act_masked(None, dims, None, 4, 0, 0, 0, None, None, None, None, None, None, None, mask),
                  "gs_policy_act_masked")
        with pytest.raises(ValueError, match="valid_mask 0x[0-9a-f]+ has bits past n_actions"):
            check(lib.gs_ppo_rows_update_masked(None, None, None, None, dims, hp, RolloutView(), None, 64, 1, 0, None, None,
                                                None, 0, None, None, mask), "gs_ppo_rows_update_masked")
        with pytest.raises(ValueError, match="valid_mask 0x[0-9a-f]+ has bits past n_actions"):
            check(lib.gs_ppo_rows_loss_masked(None, None, dims, hp, RolloutView(), None, 64, None, None, 0, None, mask),
                  "gs_ppo_rows_loss_masked")


def test_policy_keeps_and_validates_valid_actions():
    from gsamd.policy import DeviceMLPActorCritic
    pm = DeviceMLPActorCritic(12, (128, 128), 18, device="cpu", init=False, valid_actions=[0, 3, 4])
    assert pm.valid_actions == [0, 3, 4] and pm.valid_mask == 0b11001
    assert DeviceMLPActorCritic(12, (64,), 18, device="cpu", init=False, valid_actions=(17,)).valid_mask == 1 << 17
    plain = DeviceMLPActorCritic(12, (64,), 18, device="cpu", init=False)
    assert plain.valid_actions is None and plain.valid_mask == 0
    for bad in ([0, 18], [-1], [3, 4, 32]):
        with pytest.raises(ValueError, match=r"valid action -?\d+ outside \[0, 18\)"):
            DeviceMLPActorCritic(12, (128, 128), 18, device="cpu", init=False, valid_actions=bad)


def _bare_agent(cfg, cls=None):
    """An agent with only what the routing predicates read (no device buffers: runs on CPU)."""
    from gsamd.ppo_agent import DevicePPOAgent
    a = object.__new__(cls or DevicePPOAgent)
    a.config, a.rank, a.world_size = cfg, 0, 1
    return a


def test_masked_policy_routes_to_the_rows_update_and_away_from_one_launch_rollouts():
    from gsamd.config import load_config
    from gsamd.policy import DeviceMLPActorCritic
    from gsamd.rollout import DeviceRolloutCollector
    spec = {"action_space": {"discrete": 18, "valid": [0, 3, 4]},
            "observation_space": {"default": "state", "variants": {"state": {"shape": [12]}}}}
    over = dict(env_dynamics="synthetic", spec=spec, model_id="mlp_small", n_envs=32, n_steps=64, batch_size=64)
    masked = _bare_agent(load_config("LunarLander-v3", "ppo", overrides=over))
    assert masked._use_rows(64) and masked._use_rows(2) and masked._use_rows(2048)
    plain_spec = {**spec, "action_space": {"discrete": 18}}
    plain = _bare_agent(load_config("LunarLander-v3", "ppo", overrides={**over, "spec": plain_spec}))
    assert not plain._use_rows(64) and not plain._use_rows(1024) and plain._use_rows(1025)
    # the rows update's refusals hold for a masked policy at a small batch
    for kw, msg in ((dict(precision="bf16"), "fp32 only"), (dict(dp_mode="global"), "dp_mode 'global'")):
        a = _bare_agent(load_config("LunarLander-v3", "ppo", overrides={**over, **kw}))
        with pytest.raises(ValueError, match=r"action_space.valid \[0, 3, 4\].*%s" % msg):
            a._check_rows_update()
    a = _bare_agent(load_config("LunarLander-v3", "ppo", overrides=over))
    a.world_size = 2
    with pytest.raises(ValueError, match=r"action_space.valid \[0, 3, 4\].*world_size=2"):
        a._check_rows_update()
    plain._check_rows_update()
    # the one-launch rollouts have no masked head: the predicates answer False before asking the library
    for hidden, fn in (((128, 128), DeviceRolloutCollector._one_launch_supported),
                       ((64,), DeviceRolloutCollector._one_launch_mlp1_supported)):
        pm = DeviceMLPActorCritic(12, hidden, 18, device="cpu", init=False, valid_actions=[0, 3, 4])
        assert fn(object(), pm) is False


def test_reinforce_refuses_a_masked_config():
    from gsamd.config import load_config
    from gsamd.reinforce_agent import DeviceREINFORCEAgent
    cfg = load_config("Bandit-v0", "reinforce")
    DeviceREINFORCEAgent._check_scope(cfg, 1, None)
    spec = {**cfg.spec, "action_space": {"discrete": 10, "valid": [0, 3, 4]}}
    with pytest.raises(ValueError, match=r"action_space\.valid \[0, 3, 4\]"):
        DeviceREINFORCEAgent._check_scope(dataclasses.replace(cfg, spec=spec), 1, None)


def _schedule_of(record, param):
    return {"schedule": record[f"{param}_schedule"], "start_value": record[f"{param}_schedule_start_value"],
            "end_value": record[f"{param}_schedule_end_value"], "start": record[f"{param}_schedule_start"],
            "end": record[f"{param}_schedule_end"], "warmup": 0.0}


@pytest.mark.parametrize("key", PRESET_IDS)
def test_presets_equal_the_reference_record(key):
    """Every field of the preset is what the reference's load_config resolved; nothing the record
    schedules is missing; the resolved config carries the mask and needs a host env."""
    from gsamd.config import device_env_kind, load_config
    from gsamd.presets import MODEL_REGISTRY, PRESETS
    with open(os.path.join(GOLD, "config_pong_objects.json")) as f:
        rec = json.load(f)[key]
    preset = PRESETS[key]
    for k, v in preset.items():
        if k == "spec":
            assert v["action_space"] == {k2: rec["spec"]["action_space"][k2] for k2 in ("discrete", "valid")}
            name = rec["spec"]["observation_space"]["default"]
            got, want = v["observation_space"]["variants"][name], rec["spec"]["observation_space"]["variants"][name]
            assert v["observation_space"]["default"] == name and got == {k2: want[k2] for k2 in ("shape", "dtype")}
        elif k == "schedules":
            assert v == {p: _schedule_of(rec, p) for p in v}
        else:
            assert rec[k] == v, k
    scheduled = {k[:-len("_schedule")] for k in rec if k.endswith("_schedule") and rec[k]}
    assert scheduled == set(preset.get("schedules", {}))
    for k in ("env_kwargs", "env_wrappers"):
        assert (preset.get(k) or type(rec[k])()) == rec[k], k
    c = load_config(*key.split(":"))
    assert c.valid_actions == rec["_valid_actions"] == [0, 3, 4] and c.resolved_n_actions() == rec["_n_actions"] == 18
    assert list(c.hidden_dims) == rec["_hidden_dims"] == list(MODEL_REGISTRY[rec["model_id"]]["hidden_dims"])
    assert c.resolved_obs_dim() == 12 and c.batch_size == 2048 and c.n_envs * c.n_steps % c.batch_size == 0
    assert device_env_kind(c) is None          # no device dynamics: env= / env_factory=
    assert set(c.schedules) == scheduled
