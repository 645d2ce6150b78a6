"""The fused update chain's kernel entries (DESIGN.md §4.1 "kernel entries"): k_fwd_chain and
k_bwd_chain take a lean, preload-ordered argument list and come in two instantiations, one for
eager steps and a whole-update capture (absolute step index, no device step base) and one for
the chunked graph replay (step index = k_local + the chunk's device step base).  A captured
update must give bit for bit what the eager launches give, through either instantiation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("params", "adam_m", "adam_v", "grads", "metrics")


def _same(name, x, y):
    a, b = np.ascontiguousarray(x), np.ascontiguousarray(y)
    bad = np.flatnonzero(a.view(np.uint8) != b.view(np.uint8)) // a.itemsize
    assert bad.size == 0, f"{name}: {np.unique(bad).size} elements differ, first {np.unique(bad)[:8]}"


def _update(cuda, env, use_graph, **overrides):
    """One gs_ppo_update of a fresh agent's first rollout: (n_minibatches, [params, adam_m,
    adam_v, last gradients, metric records])."""
    from gsamd._lib import check, lib
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(11)
    cfg = load_config(env, "ppo", overrides=dict(env_dynamics="synthetic", **overrides))
    agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=False)
    coll = agent.get_rollout_collector("train")
    coll.collect()
    idx = agent.prefetcher.upload(0)
    n = agent.n_minibatches
    check(lib.gs_ppo_update(agent.policy_model.params.data_ptr(), agent.grads.data_ptr(), agent.adam_m.data_ptr(),
                            agent.adam_v.data_ptr(), agent.policy_model.dims, agent.hparams(), coll.buffer.view(),
                            idx.data_ptr(), agent.batch_size, n, 0, agent.metrics_buf.data_ptr(),
                            agent.stop_flag.data_ptr(), agent.workspace.data_ptr(), agent.workspace.numel(), None,
                            1 if use_graph else 0, torch.cuda.current_stream().cuda_stream), "gs_ppo_update")
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (agent.policy_model.params, agent.adam_m, agent.adam_v, agent.grads,
                                     agent.metrics_buf[:n])]
    return n, out


def _graph_equals_eager(cuda, env, n_expected, **overrides):
    (n_g, graph), (n_e, eager) = (_update(cuda, env, g, **overrides) for g in (True, False))
    assert n_g == n_e == n_expected
    assert np.isfinite(eager[0]).all() and not np.array_equal(eager[0], np.zeros_like(eager[0]))
    for name, x, y in zip(NAMES, graph, eager):
        _same(name, x, y)


# C2 (CartPole 4-256-256-2, B = 256): 64 envs x 32 steps = 8 minibatches per epoch, 2 epochs.
# C3 (LunarLander 8-128-128-4, B = 64): the smallest rollout with 3 minibatches per epoch, 64
# envs x 3 steps, 2 epochs.  Both run step 0 (no optimizer step in its forward), both parameter
# sets, and the closing k_clip_adam (an even step count: the last step lands in the workspace set
# and is copied back).
@pytest.mark.parametrize("env,overrides,n", [
    ("CartPole-v1", dict(n_envs=64, n_epochs=2), 16),
    ("LunarLander-v3", dict(n_envs=64, n_steps=3, n_epochs=2), 6)])
def test_whole_capture_equals_eager(cuda, env, overrides, n):
    """The whole-update capture (n <= 16 384 steps: no device step base) against eager launches."""
    _graph_equals_eager(cuda, env, n, **overrides)


def test_chunked_replay_equals_eager(cuda):
    """C3 at the config's T = 2048 with 64 envs and 9 epochs: 18 432 steps of B = 64, above the
    whole-capture limit, so the graph is 36 replays of a 512-step chunk reading the device step
    base (the BASE instantiations of both kernels)."""
    _graph_equals_eager(cuda, "LunarLander-v3", 18432, n_envs=64, n_epochs=9)
