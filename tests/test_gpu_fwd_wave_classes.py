"""The lagged forward's prologue chooses per wave class which of the norm slots, dW1|db1 partial
quads and W1|b1 quads a wave issues.  Which waves load what must not
change a bit of the result.  The reference is the chain with a separate k_clip_adam launch per
minibatch (GS_LAGGED_ADAM=0), which has no such prologue.  The split is on for C2 (CartPole
4-256-256-2, B = 256: classes wave 0 / waves 1-3 / wave 4 / waves 5-7, every live quad fully
live) and off for C3 (LunarLander 8-128-128-4, B = 64, below the dead-load threshold: one class,
every wave issues every load, the lanes past an array's end or outside the norm discard theirs).
tests/test_gpu_lagged.py covers C2 without statistics, eager and captured, with and without a
communicator.  Here: the unsplit prologue on C3, whose 288 W1|b1 quads leave wave 0's second
partial quad and wave 4's W1|b1 quad half live (the lane clamp), with and without a communicator
(the no-fold path, where the partial slots re-read G); the STATS instantiation of the split
prologue on C2; and C2's first step of an update (no optimizer step in its forward, nothing to
fold).  No instantiated shape both splits and has a partially live wave."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("params", "adam_m", "adam_v", "grads", "metrics")


def _same(name, x, y):
    a, b = np.ascontiguousarray(x), np.ascontiguousarray(y)
    bad = np.flatnonzero(a.view(np.uint8) != b.view(np.uint8)) // a.itemsize
    assert bad.size == 0, f"{name}: {np.unique(bad).size} elements differ, first {np.unique(bad)[:8]}"


def _lagged_and_separate(cuda, monkeypatch, env, use_graph, transport=None, track_stats=False, n_take=None,
                         **overrides):
    """One gs_ppo_update of a fresh agent's first rollout through the lagged chain and through the
    chain with a separate k_clip_adam: (n, lagged arrays, separate arrays), arrays in NAMES order."""
    from gsamd._lib import check, lib
    from gsamd.config import load_config
    from gsamd.distributed import destroy_comm, init_local_comm
    from gsamd.ppo_agent import DevicePPOAgent
    out = []
    for lag in ("1", "0"):
        monkeypatch.setenv("GS_LAGGED_ADAM", lag)
        torch.manual_seed(7)
        cfg = load_config(env, "ppo", overrides=dict(env_dynamics="synthetic", **overrides))
        comm = init_local_comm(transport, 70_000) if transport else None
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=track_stats, comm=comm)
        coll = agent.get_rollout_collector("train")
        coll.collect()
        idx = agent.prefetcher.upload(0)
        n = agent.n_minibatches if n_take is None else n_take
        assert n <= agent.n_minibatches
        check(lib.gs_ppo_update(agent.policy_model.params.data_ptr(), agent.grads.data_ptr(), agent.adam_m.data_ptr(),
                                agent.adam_v.data_ptr(), agent.policy_model.dims, agent.hparams(), coll.buffer.view(),
                                idx.data_ptr(), agent.batch_size, n, 3, agent.metrics_buf.data_ptr(),
                                agent.stop_flag.data_ptr(), agent.workspace.data_ptr(), agent.workspace.numel(), comm,
                                1 if use_graph else 0, torch.cuda.current_stream().cuda_stream), "gs_ppo_update")
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (agent.policy_model.params, agent.adam_m, agent.adam_v, agent.grads,
                                               agent.metrics_buf[:n])])
        del agent
        destroy_comm(comm)
    return n, out[0], out[1]


def _check(n, lagged, separate, n_expected):
    assert n == n_expected
    assert np.isfinite(lagged[0]).all()
    assert np.count_nonzero(lagged[1]) > 0 and np.count_nonzero(lagged[2]) > 0      # the steps ran
    for name, x, y in zip(NAMES, lagged, separate):
        _same(name, x, y)


@pytest.mark.parametrize("use_graph,transport", [(False, None), (True, None), (False, "xgmi"), (True, "xgmi")])
def test_c3_unsplit_partial_lanes(cuda, monkeypatch, use_graph, transport):
    """C3, B = 64 (one wave class, partially live lanes): 16 envs x 32 steps = 8 minibatches per
    epoch, 2 epochs = 16 steps; eager and captured; folding the partials in the forward and behind a
    one-rank communicator (no fold)."""
    n, lagged, separate = _lagged_and_separate(cuda, monkeypatch, "LunarLander-v3", use_graph, transport,
                                               n_envs=16, n_steps=32, n_epochs=2)
    _check(n, lagged, separate, 16)


@pytest.mark.parametrize("use_graph", [False, True])
def test_c2_stats_instantiation(cuda, monkeypatch, use_graph):
    """C2 with activation statistics (the STATS instantiation of the lagged forward): the
    activation records of every step, part of the metric rows, are equal too."""
    from gsamd._lib import ACT_SLOT
    n, lagged, separate = _lagged_and_separate(cuda, monkeypatch, "CartPole-v1", use_graph, track_stats=True,
                                               n_envs=512, n_epochs=1)
    assert n >= 2
    _check(n, lagged, separate, n)
    act_l, act_s = lagged[4][:, ACT_SLOT:ACT_SLOT + 8], separate[4][:, ACT_SLOT:ACT_SLOT + 8]
    assert np.count_nonzero(act_l) > 0                       # the records were written
    _same("activation records", act_l, act_s)


def test_c2_first_steps(cuda, monkeypatch):
    """C2, eager: the first minibatch of an update (its forward applies nothing and folds
    nothing) followed by two more."""
    n, lagged, separate = _lagged_and_separate(cuda, monkeypatch, "CartPole-v1", False, n_take=3,
                                               n_envs=512, n_epochs=1)
    _check(n, lagged, separate, 3)
