"""The row-parallel PPO update (csrc/gs_ppo_rows.hip), the host half: the C ABI's three new names,
the workspace query over the envelope, the entries' refusals that need no device, and
DevicePPOAgent's construction-time refusals for batch_size > 1024."""
import ctypes
import dataclasses
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"gs_ppo_rows_workspace_bytes": 2, "gs_ppo_rows_update": 17, "gs_ppo_rows_loss": 11}


def test_header_bindings_and_library_export_the_new_entries():
    from gsamd import _lib
    src = open(os.path.join(ROOT, "include", "gsamd.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", plain))
    assert declared == set(_lib.EXPORTED)
    for name, nargs in NEW_ENTRIES.items():
        assert name in declared and name in _lib.EXPORTED and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs == len(getattr(_lib.lib, name).argtypes), name
    assert _lib.lib.gs_abi_version() == _lib.GS_ABI_VERSION == 7 and re.search(r"#define GS_ABI_VERSION 7\b", src)


def test_workspace_query_over_the_envelope():
    from gsamd._lib import MlpDims, lib
    ws = lambda dims, b: int(lib.gs_ppo_rows_workspace_bytes(MlpDims(*dims), b))  # noqa: E731
    ok = (4, 256, 256, 2)
    for dims, b in (((4, 40, 64, 2), 2048), ((4, 528, 64, 2), 2048), ((4, 64, 40, 2), 2048), ((4, 64, 528, 2), 2048),
                    ((4, 0, 64, 2), 2048), ((0, 64, 64, 2), 2048), ((65, 64, 64, 2), 2048), ((4, 64, 64, 0), 2048),
                    ((4, 64, 64, 33), 2048), (ok, 1), (ok, (1 << 20) + 1), (ok, 0), (ok, -5)):
        assert ws(dims, b) == 0, (dims, b)
    for dims in (ok, (12, 128, 128, 18), (12, 64, 0, 18), (64, 512, 512, 32), (1, 16, 0, 1), (8, 512, 512, 4)):
        for b in (2, 64, 1024, 1025, 2048, 1 << 20):
            assert ws(dims, b) > 0, (dims, b)
    # one partial slot per row workgroup: it grows with min(ceil(batch / 16), 256), never with the
    # batch beyond that
    sizes = [ws(ok, b) for b in (16, 1024, 2048, 4096, 4097, 8192, 1 << 20)]
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] == sizes[4] == sizes[5] == sizes[6]
    P4 = (256 * 4 + 256 + 256 * 256 + 256 + 2 * 256 + 2 + 256 + 1 + 3) & ~3
    assert sizes[3] >= 256 * 4 * P4 and sizes[3] - 256 * 4 * P4 < 1 << 20


def test_c_entries_refuse_by_name_without_a_device():
    from gsamd._lib import GS_HP_BF16, MlpDims, PPOHparams, RolloutView, check, lib
    view = RolloutView(None, None, None, None, None, None, 64, 64)
    hp = lambda flags=0, tkl=0.0: PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, tkl, 1, flags)  # noqa: E731
    ok = MlpDims(4, 128, 128, 2)
    need = int(lib.gs_ppo_rows_workspace_bytes(ok, 2048))

    def update(dims=ok, hp_=None, batch=2048, ws_bytes=need, comm=None, ws=None):
        check(lib.gs_ppo_rows_update(None, None, None, None, dims, hp_ or hp(), view, None, batch, 1, 0, None, None, ws,
                                     ws_bytes, comm, None), "gs_ppo_rows_update")

    def loss(dims=ok, hp_=None, batch=2048, ws_bytes=need):
        check(lib.gs_ppo_rows_loss(None, None, dims, hp_ or hp(), view, None, batch, None, None, ws_bytes, None),
              "gs_ppo_rows_loss")
    with pytest.raises(ValueError, match="communicator"):
        update(comm=ctypes.c_void_p(16))
    for call in (update, loss):
        with pytest.raises(ValueError, match="bf16"):
            call(hp_=hp(flags=GS_HP_BF16))
        with pytest.raises(ValueError, match=r"workspace of %d bytes, gs_ppo_rows_workspace_bytes asks for %d"
                           % (need - 1, need)):
            call(ws_bytes=need - 1)
        with pytest.raises(ValueError, match=r"workspace of 0 bytes"):
            call(ws_bytes=0)
        with pytest.raises(ValueError, match=r"batch 1 outside \[2, 2\^20\]"):
            call(batch=1)
        with pytest.raises(ValueError, match=r"batch 1048577 outside \[2, 2\^20\]"):
            call(batch=(1 << 20) + 1)
        with pytest.raises(ValueError, match="hidden1 40 must be a multiple of 16"):
            call(dims=MlpDims(4, 40, 128, 2))
        with pytest.raises(ValueError, match="hidden1 528 must be a multiple of 16"):
            call(dims=MlpDims(4, 528, 128, 2))
        with pytest.raises(ValueError, match="hidden2 24 must be 0"):
            call(dims=MlpDims(4, 128, 24, 2))
        with pytest.raises(ValueError, match=r"obs_dim 65 outside \[1, 64\]"):
            call(dims=MlpDims(65, 128, 128, 2))
        with pytest.raises(ValueError, match=r"n_actions 33 outside \[1, 32\]"):
            call(dims=MlpDims(4, 128, 128, 33))
        with pytest.raises(ValueError, match="null buffer"):      # everything else in order: the buffers are checked last
            call()
    with pytest.raises(ValueError, match="16-byte aligned"):
        update(ws=ctypes.c_void_p(8))
    big = RolloutView(None, None, None, None, None, None, 1 << 16, 1 << 15)
    with pytest.raises(ValueError, match=r"T\*N < 2\^31"):
        check(lib.gs_ppo_rows_loss(None, None, ok, hp(), big, None, 2048, None, None, need, None), "gs_ppo_rows_loss")


def test_agent_refuses_out_of_scope_configs_before_device_work():
    from gsamd.config import load_config
    from gsamd.ppo_agent import ROWS_UPDATE_ABOVE, DevicePPOAgent
    assert ROWS_UPDATE_ABOVE == 1024
    for env, over in (("CartPole-v1", dict(n_envs=64, n_steps=32)), ("FrozenLake-v1", dict(n_envs=16, n_steps=128))):
        c = load_config(env, "ppo", overrides=dict(over, batch_size=2048, n_epochs=1))
        with pytest.raises(ValueError, match="world_size=2"):
            DevicePPOAgent(c, device="cpu", world_size=2)
        with pytest.raises(ValueError, match="batch_size 2048 > 1024 .* dp_mode 'global'"):
            DevicePPOAgent(dataclasses.replace(c, dp_mode="global"), device="cpu")
        with pytest.raises(ValueError, match="bf16"):
            DevicePPOAgent(dataclasses.replace(c, precision="bf16"), device="cpu")
    # at 1024 rows and below the rows path is not chosen, so its refusals do not apply
    c = load_config("CartPole-v1", "ppo", overrides=dict(n_envs=64, n_steps=32, batch_size=1024, n_epochs=1))
    agent = DevicePPOAgent.__new__(DevicePPOAgent)
    agent.config, agent.world_size = dataclasses.replace(c, dp_mode="global", precision="bf16"), 2
    agent._check_rows_update()
    assert not agent._use_rows(1024) and agent._use_rows(1025)
