"""The single-GPU chain's backward entry k_bwd_chain runs eight waves per workgroup (DESIGN.md §4.1,
round 9): waves 4-7 take the tile loads of roles A and C, dW2 tile 1 of their partner's K range in
role A and the acc1 MFMA chain of their partner's chunks in roles B and C.  How the work is divided
over the waves must not change a bit of the result.  The reference is the same chain with the
four-wave body (GS_BWD_NT=256 in the environment, read per gs_ppo_update call), the body of the k_bwd
entries.  The chain entry exists for the two compile-time shapes only: C2 (CartPole 4-256-256-2,
B = 256, A + 1 = 3, eight role-B slabs) and C3 (LunarLander 8-128-128-4, B = 64, A + 1 = 5, two
role-B slabs), each in fp32 and with bf16 MFMA operands (one accumulator chain per tile: waves 4-7
pass the role-B / role-C loops)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("params", "adam_m", "adam_v", "grads", "metrics")


def _same(name, x, y):
    a, b = np.ascontiguousarray(x), np.ascontiguousarray(y)
    bad = np.flatnonzero(a.view(np.uint8) != b.view(np.uint8)) // a.itemsize
    assert bad.size == 0, f"{name}: {np.unique(bad).size} elements differ, first {np.unique(bad)[:8]}"


def _eight_and_four_waves(cuda, monkeypatch, env, use_graph, track_stats=False, n_take=None, **overrides):
    """One gs_ppo_update of a fresh agent's first rollout with GS_BWD_NT unset (eight waves) and with
    GS_BWD_NT=256: (n, eight-wave arrays, four-wave arrays), arrays in NAMES order."""
    from gsamd._lib import check, lib
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    out = []
    for nt in (None, "256"):
        if nt is None:
            monkeypatch.delenv("GS_BWD_NT", raising=False)
        else:
            monkeypatch.setenv("GS_BWD_NT", nt)
        torch.manual_seed(7)
        cfg = load_config(env, "ppo", overrides=dict(env_dynamics="synthetic", **overrides))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=track_stats)
        coll = agent.get_rollout_collector("train")
        coll.collect()
        idx = agent.prefetcher.upload(0)
        n = agent.n_minibatches if n_take is None else n_take
        assert n <= agent.n_minibatches
        check(lib.gs_ppo_update(agent.policy_model.params.data_ptr(), agent.grads.data_ptr(), agent.adam_m.data_ptr(),
                                agent.adam_v.data_ptr(), agent.policy_model.dims, agent.hparams(), coll.buffer.view(),
                                idx.data_ptr(), agent.batch_size, n, 3, agent.metrics_buf.data_ptr(),
                                agent.stop_flag.data_ptr(), agent.workspace.data_ptr(), agent.workspace.numel(), None,
                                1 if use_graph else 0, torch.cuda.current_stream().cuda_stream), "gs_ppo_update")
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (agent.policy_model.params, agent.adam_m, agent.adam_v, agent.grads,
                                               agent.metrics_buf[:n])])
        del agent
    return n, out[0], out[1]


def _check(n, eight, four, n_expected):
    assert n == n_expected
    assert np.isfinite(eight[0]).all()
    assert np.count_nonzero(eight[1]) > 0 and np.count_nonzero(eight[2]) > 0      # the steps ran
    assert np.count_nonzero(four[1]) > 0 and np.count_nonzero(four[2]) > 0
    for name, x, y in zip(NAMES, eight, four):
        _same(name, x, y)


@pytest.mark.parametrize("use_graph", [False, True])
def test_c2_first_steps(cuda, monkeypatch, use_graph):
    """C2, fp32: the first three minibatches of an update, eager and captured."""
    n, eight, four = _eight_and_four_waves(cuda, monkeypatch, "CartPole-v1", use_graph, n_take=3,
                                           n_envs=512, n_epochs=1)
    _check(n, eight, four, 3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_c2_track_stats(cuda, monkeypatch, use_graph):
    """The same with activation statistics: their records are part of the metric rows."""
    n, eight, four = _eight_and_four_waves(cuda, monkeypatch, "CartPole-v1", use_graph, track_stats=True,
                                           n_take=3, n_envs=512, n_epochs=1)
    _check(n, eight, four, 3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_c2_bf16(cuda, monkeypatch, use_graph):
    """The same with bf16 MFMA operands (the Bf16Shape instantiation)."""
    n, eight, four = _eight_and_four_waves(cuda, monkeypatch, "CartPole-v1", use_graph, n_take=3,
                                           n_envs=512, n_epochs=1, precision="bf16")
    _check(n, eight, four, 3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_c3_two_slabs(cuda, monkeypatch, use_graph):
    """C3, B = 64 (A + 1 = 5, two role-B slabs, one loss wave in roles A and C): 16 envs x 32 steps = 8
    minibatches per epoch, 2 epochs = 16 steps; eager and captured."""
    n, eight, four = _eight_and_four_waves(cuda, monkeypatch, "LunarLander-v3", use_graph,
                                           n_envs=16, n_steps=32, n_epochs=2)
    _check(n, eight, four, 16)
