"""CPU: the config plumbing of CartPole-v1:ppo_rewardshaped and Bandit-v0:ppo (presets against the
reference's resolved configs, tests/golden/config_cartpole_bandit.json; which configs the device
takes and which it leaves to the host), the restated reward shaper against the reference's own class
(tests/golden/cartpole_shaper.npz), the Bandit-v0 twin (tests/bandit_twin.py, the twin of
csrc/gs_bandit_env.h) against the reference's class (tests/golden/bandit_env.npz) and its normal
draw, and the new C entries."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import bandit_twin as B
import cartpole_shaper_twin as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SHAPER = {"id": "CartPoleV1_RewardShaper", "angle_reward_scale": 1.0, "position_reward_scale": 0.25,
          "clip_potential": True}
NEW_ENTRIES = ("gs_cartpole_shaped_reset", "gs_cartpole_shaped_step", "gs_rollout_cartpole_shaped",
               "gs_bandit_reset", "gs_bandit_step", "gs_rollout_bandit")


@pytest.fixture(scope="module")
def full():
    with open(os.path.join(GOLD, "config_cartpole_bandit.json")) as f:
        return json.load(f)


def _schedule_of(record, param):
    return {"schedule": record[f"{param}_schedule"], "start_value": record[f"{param}_schedule_start_value"],
            "end_value": record[f"{param}_schedule_end_value"], "start": record[f"{param}_schedule_start"],
            "end": record[f"{param}_schedule_end"], "warmup": 0.0}


@pytest.mark.parametrize("key,obs_dim,n_actions", [("CartPole-v1:ppo_rewardshaped", 4, 2), ("Bandit-v0:ppo", 10, 10)])
def test_presets_equal_the_reference_record(full, key, obs_dim, n_actions):
    from gsamd.config import load_config
    from gsamd.presets import PRESETS
    rec, preset = full[key], PRESETS[key]
    for k, v in preset.items():
        if k == "spec":
            assert v["action_space"]["discrete"] == rec["spec"]["action_space"]["discrete"] == n_actions
            name = rec["spec"]["observation_space"]["default"]
            assert v["observation_space"]["default"] == name
            assert (v["observation_space"]["variants"][name]["shape"]
                    == rec["spec"]["observation_space"]["variants"][name]["shape"])
        elif k == "schedules":
            assert v == {"policy_lr": _schedule_of(rec, "policy_lr")}
        elif k == "n_envs" and rec[k] == "auto":
            assert v == 32                      # the record keeps "auto"; the preset takes 32
        else:
            assert rec[k] == v, k
    # nothing scheduled in the record is missing from the preset
    scheduled = {k[:-len("_schedule")] for k in rec if k.endswith("_schedule") and rec[k]}
    assert scheduled == set(preset.get("schedules", {}))
    cfg = load_config(*key.split(":"))
    assert tuple(cfg.hidden_dims) == tuple(rec["_hidden_dims"])
    assert cfg.resolved_obs_dim() == obs_dim and cfg.resolved_n_actions() == n_actions == rec["_n_actions"]
    assert cfg.env_wrappers == rec["env_wrappers"] and cfg.env_kwargs == rec["env_kwargs"]


def test_bandit_preset_resolves_what_the_issue_names(full):
    from gsamd.config import load_config
    cfg = load_config("Bandit-v0", "ppo")
    assert (cfg.model_id, cfg.n_steps, cfg.batch_size, cfg.n_epochs) == ("mlp_small", 64, 64, 4)
    assert (cfg.gamma, cfg.gae_lambda, cfg.ent_coef, cfg.max_env_steps, cfg.n_envs) == (1.0, 1.0, 0.0, 20000, 32)
    assert cfg.policy_lr == 0.04
    s = cfg.schedules["policy_lr"]
    assert (s["schedule"], s["start_value"], s["end_value"]) == ("linear", 0.04, 0.0)


def test_both_configs_resolve_to_the_device(full):
    from gsamd import needs_host_env
    from gsamd.config import device_env_kind, from_reference_config, load_config
    assert device_env_kind(load_config("CartPole-v1", "ppo_rewardshaped")) == "cartpole"
    assert device_env_kind(load_config("Bandit-v0", "ppo")) == "bandit"
    for key, kind in (("CartPole-v1:ppo_rewardshaped", "cartpole"), ("Bandit-v0:ppo", "bandit")):
        rec = dict(full[key], n_envs=32)
        assert device_env_kind(from_reference_config(SimpleNamespace(**rec))) == kind
        assert needs_host_env(SimpleNamespace(**rec)) is False
        assert needs_host_env(load_config(*key.split(":"))) is False
    # the reference object's schedule attributes arrive as the preset's schedule
    ref = from_reference_config(SimpleNamespace(**dict(full["Bandit-v0:ppo"], n_envs=32)))
    assert ref.schedules == load_config("Bandit-v0", "ppo").schedules


def _cartpole(**over):
    from gsamd.config import load_config
    return load_config("CartPole-v1", "ppo_rewardshaped", overrides=over)


@pytest.mark.parametrize("name,over", [
    ("unknown keyword", dict(env_wrappers=[dict(SHAPER, velocity_reward_scale=1.0)])),
    ("the shaper twice", dict(env_wrappers=[dict(SHAPER), dict(SHAPER)])),
    ("a non-finite scale", dict(env_wrappers=[dict(SHAPER, angle_reward_scale=float("nan"))])),
    ("an infinite scale", dict(env_wrappers=[dict(SHAPER, position_reward_scale=float("inf"))])),
    ("a non-bool clip_potential", dict(env_wrappers=[dict(SHAPER, clip_potential=1)])),
    ("a second wrapper", dict(env_wrappers=[dict(SHAPER), {"id": "X"}])),
    ("another env's shaper", dict(env_wrappers=[{"id": "MountainCarV0_RewardShaper"}])),
    ("normalize_obs", dict(normalize_obs=True)),
    ("env_kwargs", dict(env_kwargs={"render_mode": None})),
])
def test_cartpole_refusals(name, over):
    from gsamd.config import device_env_kind
    assert device_env_kind(_cartpole(**over)) is None, name


def test_cartpole_wrapper_lists_the_device_takes():
    from gsamd.config import CARTPOLE_WRAPPERS, device_env_kind, resolve_cartpole_wrappers
    assert resolve_cartpole_wrappers([]) == [] and resolve_cartpole_wrappers(None) == []
    assert resolve_cartpole_wrappers([{"id": "CartPoleV1_RewardShaper"}]) == [
        ("CartPoleV1_RewardShaper", CARTPOLE_WRAPPERS["CartPoleV1_RewardShaper"])]
    got = resolve_cartpole_wrappers([dict(SHAPER, angle_reward_scale=2, clip_potential=False)])
    assert got[0][1] == {"angle_reward_scale": 2, "position_reward_scale": 0.25, "clip_potential": False}
    assert device_env_kind(_cartpole(env_wrappers=[])) == "cartpole"
    assert device_env_kind(_cartpole(env_wrappers=[{"id": "CartPoleV1_RewardShaper"}])) == "cartpole"


def _bandit(kwargs=None, **over):
    from gsamd.config import load_config
    cfg = load_config("Bandit-v0", "ppo")
    if kwargs is not None:
        over["env_kwargs"] = kwargs
    return load_config("Bandit-v0", "ppo", overrides=over) if over else cfg


def _spec(n):
    return {"action_space": {"discrete": n}, "observation_space": {"default": "z", "variants": {"z": {"shape": ["n_arms"]}}}}


YAML = {"n_arms": 10, "means": list(range(10)), "stds": 1, "episode_length": 1}


@pytest.mark.parametrize("name,over", [
    ("n_arms 1", dict(env_kwargs={"n_arms": 1}, spec=_spec(1))),
    ("n_arms 33", dict(env_kwargs={"n_arms": 33}, spec=_spec(33))),
    ("n_arms != discrete", dict(env_kwargs=dict(YAML, n_arms=8, means=None))),
    ("a bool n_arms", dict(env_kwargs={"n_arms": True})),
    ("means of the wrong length", dict(env_kwargs=dict(YAML, means=[0, 1, 2]))),
    ("a non-finite mean", dict(env_kwargs=dict(YAML, means=[float("nan")] * 10))),
    ("a negative std", dict(env_kwargs=dict(YAML, stds=-0.5))),
    ("a negative std in a list", dict(env_kwargs=dict(YAML, stds=[1.0] * 9 + [-1.0]))),
    ("stds of the wrong length", dict(env_kwargs=dict(YAML, stds=[1.0] * 3))),
    ("episode_length 0", dict(env_kwargs=dict(YAML, episode_length=0))),
    ("a seed key", dict(env_kwargs=dict(YAML, seed=3))),
    ("a wrapper", dict(env_wrappers=[{"id": "X"}])),
    ("normalize_obs", dict(normalize_obs=True)),
    ("frame_stack", dict(frame_stack=4)),
])
def test_bandit_refusals(name, over):
    from gsamd.config import device_env_kind, resolve_bandit_env
    cfg = _bandit(**over)
    assert resolve_bandit_env(cfg) is None, name
    assert device_env_kind(cfg) is None, name


def test_bandit_kwargs_the_device_takes():
    from gsamd.config import device_env_kind, resolve_bandit_env
    b = resolve_bandit_env(_bandit())
    assert b["n_arms"] == 10 and b["episode_length"] == 1
    assert b["means"].dtype == np.float32 and b["means"].tolist() == list(range(10))
    assert b["stds"].dtype == np.float32 and b["stds"].tolist() == [1.0] * 10
    cfg = _bandit(kwargs={"n_arms": 4, "stds": [0, 0.5, 2, 1], "episode_length": 3}, spec=_spec(4))
    b = resolve_bandit_env(cfg)
    assert device_env_kind(cfg) == "bandit" and cfg.resolved_obs_dim() == 4
    assert b["means"].tolist() == B.parse_arms(4)[0].tolist() and b["stds"].tolist() == [0.0, 0.5, 2.0, 1.0]
    # the class defaults: 10 arms, std 1, one step per episode
    b = resolve_bandit_env(_bandit(kwargs={}))
    assert (b["n_arms"], b["episode_length"]) == (10, 1) and b["stds"].tolist() == [1.0] * 10
    assert np.array_equal(b["means"], np.linspace(0, 10, num=10, dtype=np.float32))
    # another env id is not a bandit
    from gsamd.config import load_config
    assert resolve_bandit_env(load_config("CartPole-v1", "ppo")) is None


def test_shaper_restatement_equals_the_reference_class():
    """The Python restatement of the shaper (the twin of csrc/gs_cartpole_env.h cartpole_phi)
    equals the reference's class bit for bit on every row of the fixture, for the three parameter
    sets; the fixture holds clipped rows, terminations, truncations and reset rows."""
    z = np.load(os.path.join(GOLD, "cartpole_shaper.npz"))
    cover, params = json.loads(str(z["coverage"])), json.loads(str(z["params"]))
    assert cover["clipped"] >= 10 and cover["terminated"] >= 5 and cover["truncated"] >= 1 and cover["reset"] >= 5
    assert z["state"].shape == (24, 37, 4) and z["state"].dtype == np.float64
    assert set(params) == {"default", "scaled", "noclip"}
    for name, kw in params.items():
        want = z[f"reward_{name}"]
        got, _ = C.shaped_rewards(z["obs0"], z["obs"], z["reset"], **kw)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        assert (want[z["reset"]] == 0.0).all()
    # clipping matters on this fixture: the unclipped rewards differ from the clipped ones
    assert (z["reward_default"] != z["reward_noclip"]).sum() >= 10


def test_bandit_twin_parser_equals_the_reference_class():
    z = np.load(os.path.join(GOLD, "bandit_env.npz"))
    for tag in ("yaml10", "default4"):
        kw = json.loads(str(z[f"kwargs_{tag}"]))
        m, s = B.parse_arms(kw["n_arms"], kw.get("means"), kw.get("stds", 1.0))
        assert m.dtype == s.dtype == np.float32
        assert np.array_equal(m.view(np.uint32), z[f"means_{tag}"].view(np.uint32))
        assert np.array_equal(s.view(np.uint32), z[f"stds_{tag}"].view(np.uint32))
        tw = B.BanditTwin(3, **kw)
        assert tw.reset().shape == (3,) + tuple(z[f"obs_shape_{tag}"]) and str(z[f"obs_dtype_{tag}"]) == "float32"
        # the product's own parser is the same
        from gsamd.config import bandit_arms
        pm, ps = bandit_arms(kw["n_arms"], kw.get("means"), kw.get("stds", 1.0))
        assert np.array_equal(pm, m) and np.array_equal(ps, s)
    assert z["means_default4"].tolist() == [0.0, np.float32(4 / 3), np.float32(8 / 3), 4.0]
    # the terminated pattern over 7 steps; a reset follows every termination (the twin: a reset row)
    for length in (1, 3):
        tw = B.BanditTwin(1, n_arms=4, episode_length=length)
        tw.reset()
        pattern = []
        while len(pattern) < 7:
            pending = bool(tw.meta[0][2])
            rew, done, trunc = tw.step([1])
            if pending:
                assert rew[0] == 0.0 and not done[0]
                continue
            assert not trunc[0] and not tw.obs().any()
            pattern.append(bool(done[0]))
        assert pattern == z[f"terminated_len{length}"].tolist()


def test_bandit_twin_draw_is_a_standard_normal():
    """32 768 pulls of one arm with mean 3 and std 2: the sample mean within five standard errors
    of 3 (5 * 2 / sqrt(n)), the sample variance within five of 4 (5 * 4 * sqrt(2 / n)).  The hash
    is deterministic, so this holds here or the draw is wrong."""
    n = 32768
    tw = B.BanditTwin(n // 8, n_arms=2, means=[0.0, 3.0], stds=[1.0, 2.0], episode_length=8, seed=7, env_offset=3)
    tw.reset()
    r = np.concatenate([tw.step(np.ones(n // 8, np.int64))[0] for _ in range(8)]).astype(np.float64)
    assert r.size == n
    assert abs(r.mean() - 3.0) <= 5 * 2 / np.sqrt(n)
    assert abs(r.var() - 4.0) <= 5 * 4 * np.sqrt(2 / n)
    # the two uniforms are distinct streams in [0, 1), and the tags stay clear of the reset tags
    u = np.array([[B.unit(7, e, 0, 0, c) for c in (0, 1)] for e in range(64)])
    assert (u >= 0).all() and (u < 1).all() and (u[:, 0] != u[:, 1]).all()
    assert not set(B.NORMAL_TAG + c for c in (0, 1)) & set(0xC0 + c for c in range(16))
    # an arm of std 0 pays exactly its float32 mean
    tw = B.BanditTwin(4, n_arms=3, means=[0.1, 0.2, 0.3], stds=[0, 0.5, 2])
    assert (tw.step([0, 0, 0, 0])[0] == np.float32(0.1)).all()


def test_bandit_twin_time_limit():
    tw = B.BanditTwin(2, n_arms=3, episode_length=3, max_steps=2)
    flags = [tw.step([0, 1])[1:] for _ in range(2)]
    assert flags[0][0].tolist() == [0, 0] and flags[1][0].tolist() == [1, 1] and flags[1][1].tolist() == [1, 1]
    tw = B.BanditTwin(2, n_arms=3, episode_length=2, max_steps=2)
    flags = [tw.step([0, 1])[1:] for _ in range(2)]
    assert flags[1][0].tolist() == [1, 1] and flags[1][1].tolist() == [0, 0]      # a termination, not a timeout
    assert tw.ep_count.tolist() == [1, 1] and tw.ep_len_sum.tolist() == [2.0, 2.0]


def _bare_agent(cfg):
    """A DevicePPOAgent with only what build_env reads (no device buffers: runs on CPU)."""
    import torch
    from gsamd.ppo_agent import DevicePPOAgent
    a = object.__new__(DevicePPOAgent)
    a.config, a.rank, a.device, a._envs, a.env_factory = cfg, 0, torch.device("cpu"), {}, None
    return a


def test_agent_builds_the_envs_per_stage():
    from gsamd.rollout import DeviceBanditVecEnv, DeviceCartPoleVecEnv
    a = _bare_agent(_cartpole(n_envs=8))
    for stage, seed in (("train", 42), ("val", 1042)):
        a.build_env(stage)
        env = a.get_env(stage)
        assert isinstance(env, DeviceCartPoleVecEnv) and env.seed == seed and env.max_steps == 500
        assert env.wrappers == [SHAPER] and env.prev_phi.shape == (8,) and tuple(env.state.shape) == (8, 4)
        assert (env.wrappers_c.shaper, env.wrappers_c.clip_potential) == (1, 1)
        assert (env.wrappers_c.angle_reward_scale, env.wrappers_c.position_reward_scale) == (1.0, 0.25)
    a = _bare_agent(_bandit(n_envs=8, batch_size=64))
    a.build_env("train")
    env = a.get_env("train")
    assert isinstance(env, DeviceBanditVecEnv) and (env.n_arms, env.obs_dim, env.n_actions) == (10, 10, 10)
    assert (env.episode_length, env.max_steps, env.seed) == (1, 1, 42) and tuple(env.obs.shape) == (8, 10)
    assert list(env.spec.means)[:10] == list(range(10)) and list(env.spec.stds)[:10] == [1.0] * 10
    a = _bare_agent(_bandit(n_envs=8, batch_size=64, max_episode_steps=5))
    a.build_env("train")
    assert a.get_env("train").max_steps == 5
    # a wrapper list the device does not apply never reaches the kernels
    with pytest.raises(ValueError, match="resolve_cartpole_wrappers"):
        DeviceCartPoleVecEnv(4, wrappers=[{"id": "X"}], device="cpu")
    with pytest.raises(ValueError, match="n_arms"):
        DeviceBanditVecEnv(4, n_arms=33, device="cpu")
    # the env takes up to 32 arms, the two-hidden-layer update's staging 15: more is refused by name, not trained wrong
    many = _bare_agent(_bandit(kwargs={"n_arms": 16}, spec=_spec(16), n_envs=8, batch_size=64))
    with pytest.raises(ValueError, match="at most 15 arms"):
        many.build_env("train")
    assert DeviceBanditVecEnv(4, n_arms=32, device="cpu").obs.shape == (4, 32)
    # a config the bandit refuses, forced onto the device by name, raises instead of training on something else
    bad = _bare_agent(_bandit(kwargs=dict(YAML, seed=3), n_envs=8, batch_size=64, env_dynamics="bandit"))
    with pytest.raises(ValueError, match="resolve_bandit_env"):
        bad.build_env("train")


def test_header_and_bindings_export_the_new_entries():
    import ctypes
    from gsamd import _lib
    src = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTED and hasattr(_lib.lib, name), name
    assert _lib.lib.gs_abi_version() == _lib.GS_ABI_VERSION == 7
    assert ctypes.sizeof(_lib.CartPoleWrappers) == 24 and ctypes.sizeof(_lib.BanditSpec) == 8 + 2 * 4 * 32
    assert _lib.GS_ENV_BANDIT == 4 and re.search(r"#define GS_ENV_BANDIT 4\b", src)
    # bad specs are refused before any launch (no device needed)
    spec = _lib.BanditSpec()
    spec.n_arms, spec.episode_length = 33, 1
    with pytest.raises(ValueError, match="n_arms"):
        _lib.check(_lib.lib.gs_bandit_reset(1, 1, 1, spec, 4, None), "gs_bandit_reset")
    spec.n_arms, spec.episode_length = 4, 0
    with pytest.raises(ValueError, match="episode_length"):
        _lib.check(_lib.lib.gs_bandit_step(1, 1, 1, spec, 1, 4, 1, 0, 0, 1, 1, 1, None, None, None, None),
                   "gs_bandit_step")
