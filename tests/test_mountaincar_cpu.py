"""CPU: the MountainCar-v0 restatement (tests/mountaincar_twin.py, the twin of
csrc/gs_mountaincar_env.h) — known answers of the dynamics, the twin's wrappers against the
reference's own classes (tests/golden/mountaincar_wrappers.npz) — and the config / agent plumbing
of the device MountainCar env."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mountaincar_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SHAPER_CONFIGS = ("shaper", "shaper_bonus", "bonus_shaper")
BONUS_CONFIGS = ("bonus_count", "bonus_inverse", "bonus_log")


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLD, "mountaincar_wrappers.npz"))
    d = {k: z[k] for k in z.files}
    d["configs"] = json.loads(str(d["configs"]))
    d["coverage"] = json.loads(str(d["coverage"]))
    return d


def test_twin_known_answers():
    # into the left wall: the position stops at -1.2 and the velocity is zeroed
    s, term, info = T.step_state([-1.19, -0.05], 0)
    assert s == [-1.2, 0.0] and info["wall"] and not term
    # at the wall with a positive velocity nothing is zeroed
    s, term, info = T.step_state([-1.2, 0.01], 2)
    assert s[0] > -1.2 and s[1] > 0.0 and not info["wall"]
    # the goal flag needs p >= 0.5 and v >= 0
    s, term, _ = T.step_state([0.49, 0.05], 2)
    assert term and s[0] >= 0.5 and s[1] >= 0.0
    s, term, _ = T.step_state([0.59, -0.01], 1)
    assert not term and s[0] >= 0.5 and s[1] < 0.0
    # both speed caps
    assert T.step_state([-0.5, 0.0699], 2)[2]["clamp_hi"] and T.step_state([-0.5, 0.0699], 2)[0][1] == 0.07
    assert T.step_state([0.0, -0.0699], 0)[2]["clamp_lo"] and T.step_state([0.0, -0.0699], 0)[0][1] == -0.07
    # one plain step, by hand
    s, _, _ = T.step_state([-0.5, 0.0], 2)
    assert s[1] == 0.0 + (1 * 0.001 + np.cos(3.0 * -0.5) * (-0.0025)) and s[0] == -0.5 + s[1]
    # reward -1 on the terminating step too; the step after a done only resets
    tw = T.MountainCarTwin(2, seed=1, max_steps=50)
    tw.state[0] = [0.49, 0.05]
    rew, done, trunc = tw.step([2, 1])
    assert rew.tolist() == [-1.0, -1.0] and done.tolist() == [True, False] and not trunc.any()
    rew, done, trunc = tw.step([2, 1])
    assert rew.tolist() == [0.0, -1.0] and not done.any() and tw.infos[0] == "reset" and tw.steps == [0, 2]
    assert tw.state[0] == T.reset_state(1, 0, 1)
    # truncation at max_steps
    tw = T.MountainCarTwin(1, seed=1, max_steps=3)
    flags = [tw.step([1])[1:] for _ in range(3)]
    assert [bool(d[0]) for d, _ in flags] == [False, False, True] and bool(flags[2][1][0])


def test_reset_draw_range():
    ps = [T.reset_state(seed, env, ep) for seed in (0, 42) for env in range(50) for ep in range(4)]
    assert all(-0.6 <= p < -0.4 and v == 0.0 for p, v in ps)
    assert len({p for p, _ in ps}) == len(ps)
    assert any(p != T.f32(p) for p, _ in ps)        # kept in float64, not rounded to float32


def _twin_rewards(fx, wrappers):
    """The twin's wrappers replayed over the fixture's observations: (rewards, tables)."""
    S, N = fx["action"].shape
    rewards = np.zeros((S, N), np.float32)
    stacks = [T.Wrappers(wrappers) for _ in range(N)]
    for e in range(N):
        stacks[e].reset(fx["obs0"][e])
        for t in range(S):
            if fx["reset"][t][e]:
                stacks[e].reset(fx["obs"][t][e])
            else:
                rewards[t][e] = stacks[e].step(fx["obs"][t][e])
    tables = None if stacks[0].table is None else np.stack([s.table for s in stacks])
    return rewards, tables


def test_fixture_covers_every_branch(fx):
    assert fx["action"].shape == (240, 8) and int(fx["max_steps"]) == 40
    assert all(v >= 1 for v in fx["coverage"].values()), fx["coverage"]
    assert set(fx["coverage"]) == {"term", "trunc", "wall", "clamp_lo", "clamp_hi", "reset"}
    assert set(fx["configs"]) == set(SHAPER_CONFIGS + BONUS_CONFIGS)
    # the recorded trajectory is the twin's own: pre-step state -> observation, reset draws
    seed, off = int(fx["seed"]), int(fx["env_offset"])
    episodes = np.zeros(8, int)
    for t in range(240):
        for e in range(8):
            if fx["reset"][t][e]:
                want = T.reset_state(seed, off + e, int(episodes[e]))
            else:
                want = T.step_state(fx["state"][t][e].tolist(), fx["action"][t][e])[0]
            assert np.array_equal(T.obs_of(want), fx["obs"][t][e]), (t, e)
        episodes += fx["done"][t]


@pytest.mark.parametrize("name", SHAPER_CONFIGS)
def test_twin_shaper_matches_reference_classes(fx, name):
    """The reference's values were computed by numpy 2 in float32 where numpy 1.26 (its pinned
    version) and the twin / device compute in float64: (100 + 10 + 50) * 4 * 2^-24 = 3.8e-5 is the
    bound of that rounding, 5e-5 the bar."""
    rewards, tables = _twin_rewards(fx, fx["configs"][name])
    worst = float(np.abs(rewards.astype(np.float64) - fx[f"reward_{name}"].astype(np.float64)).max())
    print(name, "worst |twin - reference| reward", worst, "max |r|", float(np.abs(fx[f"reward_{name}"]).max()))
    assert worst <= 5e-5
    if tables is not None:
        assert np.array_equal(tables, fx[f"table_{name}"])
    assert np.all(rewards[fx["reset"]] == 0.0) and np.all(fx[f"reward_{name}"][fx["reset"]] == 0.0)


@pytest.mark.parametrize("name", BONUS_CONFIGS)
def test_twin_bonus_matches_reference_classes(fx, name):
    """Bonus-only rewards within two float32 ulps at 1 (2.4e-7), tables exact."""
    rewards, tables = _twin_rewards(fx, fx["configs"][name])
    worst = float(np.abs(rewards.astype(np.float64) - fx[f"reward_{name}"].astype(np.float64)).max())
    print(name, "worst |twin - reference| reward", worst)
    assert worst <= 2.4e-7
    assert np.array_equal(tables, fx[f"table_{name}"])
    assert int(tables.sum()) == int((~fx["reset"]).sum())       # one visit per non-reset step, never cleared


def test_fixture_binning_agrees_in_float32_and_float64(fx):
    """The condition the generator asserted, from the fixture's observations: the bins numpy 2
    forms in float32 are the bins float64 arithmetic forms."""
    obs = np.concatenate([fx["obs0"], fx["obs"].reshape(-1, 2)])
    for pb, vb in ((50, 50), (7, 5)):
        kw = {"position_bins": pb, "velocity_bins": vb}
        for o in obs:
            pn = np.clip((np.float32(o[0]) - (-1.2)) / (0.6 - (-1.2)), 0.0, 0.999999)
            vn = np.clip((np.float32(o[1]) - (-0.07)) / (0.07 - (-0.07)), 0.0, 0.999999)
            assert (int(pn * pb), int(vn * vb)) == T.bins_of(kw, float(o[0]), float(o[1]))


def test_kernel_case_has_no_step_at_a_threshold():
    """The GPU test leaves a step out of its flag comparison when the twin's value lies within
    1e-12 of a threshold; for its seed the twin has no such step."""
    c = T.KERNEL_CASE
    rng = np.random.default_rng(c["rng"])
    tw = T.MountainCarTwin(c["N"], seed=c["seed"], env_offset=c["env_offset"], max_steps=c["max_steps"])
    near = 0
    cnt = dict(term=0, trunc=0, wall=0, clamp_lo=0, clamp_hi=0, reset=0)
    for t in range(c["steps"]):
        if t % c["redraw"] == 0:
            tw.state = T.box_states(rng, c["N"]).tolist()
        a = rng.integers(0, 3, c["N"])
        near += sum(T.threshold_gap(tw.state[e], a[e]) < 1e-12 for e in range(c["N"]) if not tw.pending[e])
        _, done, trunc = tw.step(a)
        for e in range(c["N"]):
            if tw.infos[e] == "reset":
                cnt["reset"] += 1
            else:
                for k in ("wall", "clamp_lo", "clamp_hi"):
                    cnt[k] += bool(tw.infos[e][k])
                cnt["term"] += bool(done[e] and not trunc[e])
                cnt["trunc"] += bool(trunc[e])
    assert near == 0
    assert all(v >= 1 for v in cnt.values()), cnt


def _configs():
    return json.load(open(os.path.join(GOLD, "config_mountaincar.json")))


@pytest.mark.parametrize("variant", ["ppo", "ppo_rewardshaped", "ppo_curiosity"])
def test_presets_equal_the_reference_resolution(variant):
    """The bundled preset is what the reference resolves from its YAML, n_envs excepted: the
    reference leaves it at "auto" (the host's core count), the record keeps "auto", the preset
    takes 32."""
    from gsamd.config import load_config
    from gsamd.presets import PRESETS
    full = _configs()[f"MountainCar-v0:{variant}"]
    preset = PRESETS[f"MountainCar-v0:{variant}"]
    assert full["n_envs"] == "auto" and preset["n_envs"] == 32
    for k, v in preset.items():
        if k == "n_envs":
            continue
        if k == "spec":
            assert v["action_space"]["discrete"] == full["spec"]["action_space"]["discrete"] == 3
            assert (v["observation_space"]["variants"]["state"]["shape"]
                    == full["spec"]["observation_space"]["variants"]["state"]["shape"] == [2])
        else:
            assert full[k] == v, k
    cfg = load_config("MountainCar-v0", variant)
    assert (cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.n_epochs) == (32, 2048, 64, 10)
    assert tuple(cfg.hidden_dims) == tuple(full["_hidden_dims"]) == (256, 256)
    assert cfg.resolved_obs_dim() == 2 and cfg.resolved_n_actions() == 3
    assert cfg.env_wrappers == full["env_wrappers"] and len(cfg.env_wrappers) == 1


SH = {"id": T.SHAPER, "position_reward_scale": 100.0, "velocity_reward_scale": 10.0, "height_reward_scale": 50.0}
BO = {"id": T.BONUS, "position_bins": 50, "velocity_bins": 50, "bonus_scale": 0.1, "bonus_type": "count"}


def test_device_env_kind_for_mountaincar():
    from gsamd import needs_host_env
    from gsamd.config import device_env_kind, from_reference_config, load_config
    for variant in ("ppo", "ppo_rewardshaped", "ppo_curiosity"):
        assert device_env_kind(load_config("MountainCar-v0", variant)) == "mountaincar"
        full = _configs()[f"MountainCar-v0:{variant}"]
        ref = SimpleNamespace(**dict(full, n_envs=32))
        assert device_env_kind(from_reference_config(ref)) == "mountaincar"
        assert needs_host_env(ref) is False

    def kind(wrappers, **over):
        return device_env_kind(load_config("MountainCar-v0", "ppo", overrides=dict(over, env_wrappers=wrappers)))
    assert kind([]) == "mountaincar"
    assert kind([SH, BO]) == "mountaincar" and kind([BO, SH]) == "mountaincar"
    assert kind([{"id": T.SHAPER}]) == "mountaincar" and kind([{"id": T.BONUS}]) == "mountaincar"
    for bt in ("count", "inverse", "log"):
        assert kind([dict(BO, bonus_type=bt, min_count=3)]) == "mountaincar"
    assert kind([dict(BO, position_bins=128, velocity_bins=128)]) == "mountaincar"      # 16384 cells
    # anything else is the host env's
    assert kind([{"id": "DiscreteEncoder"}]) is None                           # an unknown id
    assert kind([SH, {"id": "X"}]) is None
    assert kind([dict(SH, goal_bonus=1.0)]) is None                            # an unknown keyword
    assert kind([dict(BO, min_count=0)]) is None
    assert kind([dict(BO, min_count=1.5)]) is None
    assert kind([dict(BO, position_bins=129, velocity_bins=128)]) is None      # oversized table
    assert kind([dict(BO, position_bins=0)]) is None
    assert kind([dict(BO, bonus_type="sqrt")]) is None
    assert kind([SH, SH]) is None and kind([BO, dict(BO, bonus_scale=1.0)]) is None     # an id twice
    assert kind([SH], env_kwargs={"goal_velocity": 0.01}) is None
    assert kind([SH], normalize_obs=True) is None
    assert kind([SH], frame_stack=4) is None
    # the other envs still take no wrapper
    assert device_env_kind(load_config("CartPole-v1", "ppo", overrides=dict(env_wrappers=[SH]))) is None
    assert device_env_kind(load_config("Acrobot-v1", "ppo", overrides=dict(env_wrappers=[BO]))) is None


def test_c_abi_answers_for_the_mountaincar_kind():
    """gs_rollout_env_supported answers for GS_ENV_MOUNTAINCAR (obs dim 2, 3 actions, policy in
    LDS); gs_rollout_env refuses the kind and names the entry that takes the tables (both checks
    run on the host, before any buffer is read)."""
    import ctypes
    from gsamd._lib import GS_ENV_MOUNTAINCAR, MlpDims, check, lib
    assert GS_ENV_MOUNTAINCAR == 3

    def supported(*dims):
        v = ctypes.c_int(-1)
        check(lib.gs_rollout_env_supported(MlpDims(*dims), GS_ENV_MOUNTAINCAR, ctypes.byref(v)), "supported")
        return v.value
    assert supported(2, 128, 128, 3) == 1
    assert supported(2, 256, 256, 3) == 0            # mlp_medium does not fit in LDS
    assert supported(6, 128, 128, 3) == 0 and supported(2, 128, 128, 2) == 0
    with pytest.raises(ValueError, match="gs_rollout_mountaincar"):
        check(lib.gs_rollout_env(None, MlpDims(2, 128, 128, 3), 16, 4, 0, 0, 0, GS_ENV_MOUNTAINCAR, None, None, None,
                                 None, 200, 0, 0, *([None] * 11)), "gs_rollout_env")


def _bare_agent(cfg):
    """A DevicePPOAgent with only what build_env reads (no device buffers: runs on CPU)."""
    import torch
    from gsamd.ppo_agent import DevicePPOAgent
    a = object.__new__(DevicePPOAgent)
    a.config, a.rank, a.device, a._envs, a.env_factory = cfg, 0, torch.device("cpu"), {}, None
    return a


def test_agent_builds_the_mountaincar_env_per_stage():
    from gsamd._lib import GS_ENV_MOUNTAINCAR
    from gsamd.config import load_config
    from gsamd.rollout import DeviceMountainCarVecEnv
    cfg = load_config("MountainCar-v0", "ppo_curiosity")
    a = _bare_agent(cfg)
    a.build_env("train")
    a.build_env("val")
    tr, va = a.get_env("train"), a.get_env("val")
    assert isinstance(tr, DeviceMountainCarVecEnv) and tr.seed == cfg.seed_train and tr.max_steps == 200
    assert isinstance(va, DeviceMountainCarVecEnv) and va.seed == cfg.seed_val and va.max_steps == 200
    assert tr.wrappers == va.wrappers == cfg.env_wrappers          # every stage from the same list
    assert tr.device_native and tr.env_kind == GS_ENV_MOUNTAINCAR and hasattr(tr, "one_launch_max_envs")
    assert tr.obs_shape == (2,) and tr.n_actions == 3 and tr.num_envs == 32
    assert tuple(tr.state.shape) == (32, 4) and tuple(tr.meta.shape) == (32, 3) and tuple(tr.obs.shape) == (32, 2)
    assert tuple(tr.counts.shape) == (32, 2500) and str(tr.counts.dtype) == "torch.int32"
    w = tr.wrappers_c
    assert list(w.order) == [2, 0] and (w.position_bins, w.velocity_bins, w.bonus_type, w.min_count) == (50, 50, 0, 1)
    assert w.bonus_scale == 0.1
    short = _bare_agent(load_config("MountainCar-v0", "ppo_rewardshaped", overrides=dict(max_episode_steps=50)))
    short.build_env("train")
    env = short.get_env("train")
    assert env.max_steps == 50 and tuple(env.counts.shape) == (32, 0) and list(env.wrappers_c.order) == [1, 0]
    assert (env.wrappers_c.position_reward_scale, env.wrappers_c.velocity_reward_scale,
            env.wrappers_c.height_reward_scale) == (100.0, 10.0, 50.0)
    both = _bare_agent(load_config("MountainCar-v0", "ppo", overrides=dict(env_wrappers=[BO, SH])))
    both.build_env("train")
    assert list(both.get_env("train").wrappers_c.order) == [2, 1]
    # the env itself refuses a list the device does not apply
    with pytest.raises(ValueError, match="env_wrappers"):
        DeviceMountainCarVecEnv(4, wrappers=[dict(BO, min_count=0)], device="cpu")
    # the dynamics need the env's own shapes
    wrong = _bare_agent(load_config("CartPole-v1", "ppo", overrides=dict(env_dynamics="mountaincar")))
    with pytest.raises(ValueError, match="mountaincar"):
        wrong.build_env("train")
