"""CPU tests of the FrozenLake-v1 / Taxi-v3 path: the transition tables against a second, naive
per-state simulator and the envs' published facts, the DiscreteEncoder restatement against the
reference's own outputs, the presets against the reference's resolution, the config plumbing, and
the one-hidden-layer policy's host side."""
import json
import os
import re

import numpy as np
import pytest

import tabular_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

MAPS = {"4x4": "SFFF/FHFH/FFFH/HFFG",
        "8x8": "SFFFFFFF/FFFFFFFF/FFFHFFFF/FFFFFHFF/FFFHFFFF/FHHFFFHF/FHFFHFHF/FFFHFFFG"}
TAXI_ROWS = ["|R: | : :G|", "| : | : : |", "| : : : : |", "| | : | : |", "|Y| : |B: |"]
LOCS = [(0, 0), (0, 4), (4, 0), (4, 3)]


# ---------------------------------------------------------------- naive simulators (the issue's rules)
def _lake_outcomes(grid, s, a, slippery):
    """[(next, reward, terminated)] of one (state, action), straight from the rules."""
    n = len(grid)
    row, col = divmod(s, n)
    if grid[row][col] in "HG":
        return [(s, 0.0, True)] * (3 if slippery else 1)
    out = []
    for b in ([(a - 1) % 4, a, (a + 1) % 4] if slippery else [a]):
        r, c = row, col
        if b == 0:
            c = max(c - 1, 0)
        if b == 1:
            r = min(r + 1, n - 1)
        if b == 2:
            c = min(c + 1, n - 1)
        if b == 3:
            r = max(r - 1, 0)
        ch = grid[r][c]
        out.append((r * n + c, 1.0 if ch == "G" else 0.0, ch in "HG"))
    return out


def _taxi_outcome(s, a):
    dest = s % 4
    p = (s // 4) % 5
    col = (s // 20) % 5
    row = s // 100
    reward, done = -1.0, False
    if a == 0:
        row = min(row + 1, 4)
    elif a == 1:
        row = max(row - 1, 0)
    elif a == 2 and TAXI_ROWS[row][2 * col + 2] == ":":
        col += 1
    elif a == 3 and TAXI_ROWS[row][2 * col] == ":":
        col -= 1
    elif a == 4:
        if p < 4 and (row, col) == LOCS[p]:
            p = 4
        else:
            reward = -10.0
    elif a == 5:
        if p == 4 and (row, col) == LOCS[dest]:
            p, reward, done = dest, 20.0, True
        elif p == 4 and (row, col) in LOCS:
            p = LOCS.index((row, col))
        else:
            reward = -10.0
    return ((row * 5 + col) * 5 + p) * 4 + dest, reward, done


@pytest.mark.parametrize("map_name", ["4x4", "8x8"])
@pytest.mark.parametrize("slippery", [True, False])
def test_frozenlake_table_equals_the_naive_simulator(map_name, slippery):
    from gsamd.toytext import frozenlake_table
    nxt, rew, term, starts, S, A, K = frozenlake_table(map_name, slippery)
    grid = MAPS[map_name].split("/")
    n = len(grid)
    assert (S, A, K) == (n * n, 4, 3 if slippery else 1)
    assert nxt.shape == rew.shape == term.shape == (S, A, K)
    assert (nxt.dtype, rew.dtype, term.dtype, starts.dtype) == (np.int32, np.float32, np.uint8, np.int32)
    assert starts.tolist() == [0]
    for s in range(S):
        for a in range(A):
            want = _lake_outcomes(grid, s, a, slippery)
            got = [(int(nxt[s, a, k]), float(rew[s, a, k]), bool(term[s, a, k])) for k in range(K)]
            assert got == want, (s, a)


def test_frozenlake_facts():
    from gsamd.toytext import MAX_EPISODE_STEPS, frozenlake_table
    for map_name, holes, goal in (("4x4", {5, 7, 11, 12}, 15),
                                  ("8x8", {19, 29, 35, 41, 42, 46, 49, 52, 54, 59}, 63)):
        nxt, rew, term, _, S, A, K = frozenlake_table(map_name, False)
        absorbing = {s for s in range(S) if all(nxt[s, a, 0] == s and term[s, a, 0] for a in range(A))}
        assert absorbing == holes | {goal}
        assert {int(s) for s in nxt[rew > 0]} == {goal}
        assert set(np.unique(rew)) == {0.0, 1.0}
        assert frozenlake_table(map_name, True)[6] == 3 and K == 1
    assert MAX_EPISODE_STEPS == {"frozenlake": 100, "taxi": 200}      # FrozenLake-v1 is 100 for both maps


def test_taxi_table_equals_the_naive_simulator_and_facts():
    from gsamd.toytext import taxi_table
    nxt, rew, term, starts, S, A, K = taxi_table()
    assert (S, A, K) == (500, 6, 1) and nxt.shape == (500, 6, 1)
    for s in range(S):
        for a in range(A):
            assert (int(nxt[s, a, 0]), float(rew[s, a, 0]), bool(term[s, a, 0])) == _taxi_outcome(s, a), (s, a)
    assert len(starts) == 300 and len(set(starts.tolist())) == 300
    assert all((s // 4) % 5 < 4 and (s // 4) % 5 != s % 4 for s in starts.tolist())
    ends = np.argwhere(term[:, :, 0] != 0)
    assert len(ends) == 4 and all(rew[s, a, 0] == 20.0 and a == 5 for s, a in ends)
    assert int((rew[:, 4, 0] == -1.0).sum()) == 16                 # pickup is legal in exactly 16 states
    assert int((rew[:, 5, 0] == -10.0).sum()) == 484               # dropoff is illegal in exactly 484
    pos = lambda s: (s // 100, (s // 20) % 5)                      # noqa: E731
    for a, axis, count in ((2, 1, 14), (3, 1, 14), (0, 0, 20), (1, 0, 20)):
        moved = {pos(s) for s in range(S) if pos(int(nxt[s, a, 0]))[axis] != pos(s)[axis]}
        assert len(moved) == count, (a, len(moved))
    assert set(np.unique(rew)) == {-10.0, -1.0, 20.0}


# ---------------------------------------------------------------- encoder
def test_encoder_twin_equals_the_reference_encoder(golden):
    ref = golden("discrete_encoder.npz")
    from gsamd.config import discrete_encoding_dim
    for n in (16, 64, 500):
        for enc in ("array", "binary", "onehot"):
            want = ref[f"{enc}_{n}"]
            got = np.stack([T.encode(enc, n, s) for s in range(n)])
            assert got.dtype == np.float32 and got.shape == want.shape
            assert want.shape[1] == T.encoding_dim(enc, n) == discrete_encoding_dim(enc, n)
            # array: the reference keeps int64; the policy's input is its float32 value (exact below 2^24)
            assert np.array_equal(got, want.astype(np.float32)), (enc, n)
            if enc == "array":
                assert want.dtype == np.int64 and np.array_equal(want[:, 0], np.arange(n))


# ---------------------------------------------------------------- config
IDS = (("FrozenLake-v1", "ppo", "frozenlake"), ("FrozenLake-v1", "ppo_deterministic", "frozenlake"),
       ("Taxi-v3", "ppo", "taxi"))


def _full():
    return json.load(open(os.path.join(GOLD, "config_toytext.json")))


@pytest.mark.parametrize("env,variant,kind", IDS)
def test_presets_equal_the_reference_resolution(env, variant, kind):
    """The bundled preset is what the reference resolves from its YAML, n_envs excepted: the
    reference leaves it at "auto" (the host's core count), the record keeps "auto", the preset
    takes 32 (as MountainCar-v0 does)."""
    from gsamd.config import load_config
    r = _full()[f"{env}:{variant}"]
    c = load_config(env, variant)
    assert r["n_envs"] == "auto" and c.n_envs == 32
    for f in ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "clip_range_vf", "ent_coef",
              "vf_coef", "policy_lr", "max_grad_norm", "model_id", "seed", "normalize_advantages", "target_kl",
              "env_wrappers", "env_kwargs", "env_id", "project_id", "max_env_steps", "max_episode_steps", "obs_type",
              "seed_train", "seed_val", "normalize_obs", "optimizer", "accelerator"):
        assert getattr(c, f) == r[f], (f, getattr(c, f), r[f])
    assert list(c.hidden_dims) == r["_hidden_dims"] == [64]
    assert c.valid_actions == r["_valid_actions"]
    assert c.resolved_n_actions() == r["_n_actions"]
    assert c.spec["observation_space"] == {k: r["spec"]["observation_space"][k] for k in ("default", "variants")}
    assert c.resolved_obs_dim() == 1          # the `array` encoder, whatever the state count


def _bare_agent(cfg):
    """A DevicePPOAgent with only what build_env reads (no device buffers: runs on CPU)."""
    import torch
    from gsamd.ppo_agent import DevicePPOAgent
    a = object.__new__(DevicePPOAgent)
    a.config, a.rank, a.device, a._envs, a.env_factory = cfg, 0, torch.device("cpu"), {}, None
    return a


@pytest.mark.parametrize("env,variant,kind", IDS)
def test_reference_configs_resolve_to_the_device_env(env, variant, kind):
    from types import SimpleNamespace
    from gsamd import needs_host_env
    from gsamd.config import device_env_kind, from_reference_config, load_config
    from gsamd.rollout import DeviceTabularVecEnv
    ref = SimpleNamespace(**{k: v for k, v in _full()[f"{env}:{variant}"].items() if not k.startswith("_")})
    ref.n_envs = 8
    assert not needs_host_env(ref)
    cfg = from_reference_config(ref)
    assert device_env_kind(cfg) == device_env_kind(load_config(env, variant)) == kind
    a = _bare_agent(cfg)
    a.build_env("train")
    a.build_env("val")
    e = a.get_env("train")
    assert isinstance(e, DeviceTabularVecEnv) and e.kind == kind and e.encoding == "array" and e.obs_dim == 1
    assert (e.seed, a.get_env("val").seed) == (cfg.seed_train, cfg.seed_val)
    if kind == "taxi":
        assert (e.n_states, e.n_actions, e.n_outcomes, e.max_steps, e.starts.numel()) == (500, 6, 1, 200, 300)
    else:
        assert (e.n_states, e.n_actions, e.max_steps) == (16, 4, 100)
        assert e.n_outcomes == (3 if variant == "ppo" else 1)


def test_device_env_kind_accepts_only_what_the_device_builds():
    from gsamd.config import device_env_kind, load_config, resolve_tabular_env
    enc = lambda **kw: [dict({"id": "DiscreteEncoder"}, **kw)]        # noqa: E731
    lake = lambda **ov: load_config("FrozenLake-v1", "ppo", overrides=ov)      # noqa: E731
    taxi = lambda **ov: load_config("Taxi-v3", "ppo", overrides=ov)            # noqa: E731
    big = lake(env_kwargs={"map_name": "8x8"})
    assert device_env_kind(big) == "frozenlake"
    assert resolve_tabular_env(big)["n_states"] == 64 and resolve_tabular_env(big)["is_slippery"] is True
    assert big.resolved_obs_dim() == 1
    # the three encodings, and the class default
    assert lake(env_wrappers=enc()).resolved_obs_dim() == 4 and resolve_tabular_env(lake(env_wrappers=enc()))[
        "encoding"] == "binary"
    assert lake(env_wrappers=enc(encoding="onehot")).resolved_obs_dim() == 16
    assert lake(env_wrappers=enc(encoding="onehot"), env_kwargs={"map_name": "8x8"}).resolved_obs_dim() == 64
    assert taxi(env_wrappers=enc(encoding="binary")).resolved_obs_dim() == 9
    assert device_env_kind(taxi(env_wrappers=enc(encoding="binary"))) == "taxi"
    # everything else is the host env
    assert device_env_kind(lake(env_kwargs={"desc": ["SF", "FG"]})) is None
    assert device_env_kind(lake(env_kwargs={"map_name": "16x16"})) is None
    assert device_env_kind(lake(env_kwargs={"is_slippery": "yes"})) is None
    assert device_env_kind(lake(env_wrappers=enc(encoding="array") + [{"id": "X"}])) is None
    assert device_env_kind(lake(env_wrappers=[])) is None                       # no float observation
    assert device_env_kind(lake(env_wrappers=enc(encoding="gray"))) is None
    assert device_env_kind(lake(env_wrappers=enc(encoding="array", extra=1))) is None
    assert device_env_kind(taxi(env_wrappers=enc(encoding="onehot"))) is None  # 500 > 64 observation values
    assert device_env_kind(taxi(env_kwargs={"is_rainy": True})) is None
    assert device_env_kind(lake(normalize_obs=True)) is None
    with pytest.raises(ValueError, match="no device dynamics"):
        _bare_agent(taxi(env_wrappers=enc(encoding="onehot"))).build_env("train")


# ---------------------------------------------------------------- one-hidden-layer policy, host side
def test_one_layer_param_shapes_and_reference_init():
    import torch
    from gsamd.policy import param_shapes, reference_init
    from oracle import ppo_ref
    keys = ["backbone.0.weight", "backbone.0.bias", "policy_head.weight", "policy_head.bias", "value_head.weight",
            "value_head.bias"]
    for D, H, A in ((1, 64, 4), (1, 64, 6), (9, 64, 6), (64, 64, 32)):
        shapes = param_shapes(D, (H,), A)
        assert [k for k, _ in shapes] == keys
        assert [s for _, s in shapes] == [(H, D), (H,), (A, H), (A,), (1, H), (1,)]
        assert [tuple(s) for _, s in shapes] == [tuple(s) for _, s in ppo_ref.param_shapes((D, H, A))]
        torch.manual_seed(3)
        sd = reference_init(D, (H,), A)
        assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == [s for _, s in shapes]
        assert sum(v.numel() for v in sd.values()) == H * D + H + A * H + A + H + 1
    assert sum(int(np.prod(s)) for _, s in param_shapes(1, (64,), 4)) == 453
    assert sum(int(np.prod(s)) for _, s in param_shapes(1, (64,), 6)) == 583


def test_library_serves_one_hidden_layer_on_the_host_side():
    """hidden2 == 0: the parameter count, the workspace sizes and the shape envelope are host
    computations (no kernel runs)."""
    import ctypes
    from gsamd import _lib
    from gsamd._lib import MlpDims, lib
    assert lib.gs_mlp_param_count(MlpDims(1, 64, 0, 4)) == 453
    assert lib.gs_mlp_param_count(MlpDims(1, 64, 0, 6)) == 583
    assert lib.gs_mlp_param_count(MlpDims(64, 64, 0, 32)) == 6305
    assert lib.gs_mlp_param_count(MlpDims(4, 256, 256, 2)) == 4 * 256 + 256 + 256 * 256 + 256 + 2 * 256 + 2 + 256 + 1
    for d in (MlpDims(1, 64, 0, 4), MlpDims(64, 64, 0, 32)):
        assert lib.gs_ppo_workspace_bytes(d, 64) > 0 and lib.gs_ppo_update_workspace_bytes(d, 64, 8) > 0
        assert lib.gs_policy_scratch_bytes(d, 37) > 0
        v = ctypes.c_int(7)
        _lib.check(lib.gs_rollout_env_supported(d, _lib.GS_ENV_CARTPOLE, ctypes.byref(v)), "supported")
        assert v.value == 0
        v = ctypes.c_int(7)
        _lib.check(lib.gs_rollout_synth_supported(d, ctypes.byref(v)), "supported")
        assert v.value == 0
    # outside the LDS envelope: refused with the byte counts
    assert lib.gs_ppo_update_workspace_bytes(MlpDims(64, 1024, 0, 4), 64, 8) == 0
    v = ctypes.c_int(0)
    with pytest.raises(ValueError, match=r"one hidden layer .*\d+ bytes"):
        _lib.check(lib.gs_rollout_env_supported(MlpDims(64, 1024, 0, 4), _lib.GS_ENV_CARTPOLE, ctypes.byref(v)), "x")
    with pytest.raises(ValueError, match="multiple of 16"):
        _lib.check(lib.gs_rollout_env_supported(MlpDims(4, 40, 0, 4), _lib.GS_ENV_CARTPOLE, ctypes.byref(v)), "x")


def test_agent_rejects_one_layer_policy_with_ranks_or_bf16_before_device_work():
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    cfg = load_config("FrozenLake-v1", "ppo", overrides=dict(n_envs=8, n_steps=16, batch_size=64))
    with pytest.raises(ValueError, match="one hidden layer"):
        DevicePPOAgent(cfg, device="cpu", world_size=2)
    bf = load_config("FrozenLake-v1", "ppo", overrides=dict(n_envs=8, n_steps=16, batch_size=64, precision="bf16"))
    with pytest.raises(ValueError, match="one hidden layer"):
        DevicePPOAgent(bf, device="cpu")


def test_header_and_bindings_export_the_new_symbols():
    from gsamd import _lib
    src = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src))
    for name in ("gs_tabular_reset", "gs_tabular_step"):
        assert name in declared and name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert declared == set(_lib.EXPORTED)
    assert _lib.lib.gs_abi_version() == _lib.GS_ABI_VERSION == 7
    assert ctypes_sizeof_spec() == 24


def ctypes_sizeof_spec():
    import ctypes
    from gsamd._lib import TabularSpec
    return ctypes.sizeof(TabularSpec)
