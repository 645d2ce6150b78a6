"""The device tabular env (csrc/gs_tabular.hip: FrozenLake-v1, Taxi-v3) against its numpy twin
(tests/tabular_twin.py) — exact — and with the one-hidden-layer policy through the collector and
the public agent entry."""
import numpy as np
import pytest
import torch

import tabular_twin as TW

pytestmark = pytest.mark.gpu

IDS = (("FrozenLake-v1", "ppo"), ("FrozenLake-v1", "ppo_deterministic"), ("Taxi-v3", "ppo"))


def _rows(N, cuda):
    return (torch.zeros(N, device=cuda), torch.zeros(N, dtype=torch.uint8, device=cuda),
            torch.zeros(N, dtype=torch.uint8, device=cuda))


def _taxi_driver(nxt, s):
    """The action of a sensible driver in Taxi state s: pick up / drop off at the right place, else
    the first move of a shortest path (breadth-first over the table's move actions) to it."""
    from gsamd.toytext import TAXI_LOCS
    row, col, p, dest = s // 100, (s // 20) % 5, (s // 4) % 5, s % 4
    goal = TAXI_LOCS[dest if p == 4 else p]
    if (row, col) == goal:
        return 5 if p == 4 else 4
    pos = lambda q: (q // 100, (q // 20) % 5)       # noqa: E731
    frontier, first = [s], {s: None}
    while frontier:
        nxt_frontier = []
        for q in frontier:
            for a in range(4):
                q2 = int(nxt[q, a, 0])
                if q2 not in first:
                    first[q2] = a if first[q] is None else first[q]
                    if pos(q2) == goal:
                        return first[q2]
                    nxt_frontier.append(q2)
        frontier = nxt_frontier
    raise AssertionError("unreachable location")


@pytest.mark.parametrize("kind,map_name,slippery,encoding", [
    ("frozenlake", "4x4", True, "array"), ("frozenlake", "8x8", False, "onehot"), ("taxi", "4x4", True, "binary")])
def test_step_kernel_equals_the_twin_teacher_forced(cuda, kind, map_name, slippery, encoding):
    """120 teacher-forced steps of random actions (Taxi: half the envs mostly driven, or nothing
    would terminate), N = 37 (a ragged block), env_offset 3, max_steps 12: states, meta,
    observations, reward / done / timeout rows and the episode counters are exactly the twin's."""
    from gsamd import toytext
    from gsamd.rollout import DeviceTabularVecEnv
    N, steps, max_steps, off, seed = 37, 120, 12, 3, 5
    tables = toytext.tables_for(kind, map_name, slippery)
    dev = DeviceTabularVecEnv(N, kind=kind, encoding=encoding, map_name=map_name, is_slippery=slippery, seed=seed,
                              env_offset=off, max_steps=max_steps, device=cuda)
    twin = TW.TabularTwin(tables, N, encoding, seed=seed, env_offset=off, max_steps=max_steps)
    assert dev.obs_dim == TW.encoding_dim(encoding, tables[4]) and (dev.n_states, dev.n_actions, dev.n_outcomes) == tables[4:]
    o_d, _ = dev.reset()
    assert np.array_equal(o_d.cpu().numpy(), twin.reset())
    assert np.array_equal(dev.state.cpu().numpy(), twin.state) and not dev.meta.any()
    if kind == "taxi":
        assert len(set(twin.state.tolist())) > 10          # the 300 starts are drawn from
    rng = np.random.default_rng(17)
    rew, dn, to = _rows(N, cuda)
    seen = dict(term=0, trunc=0, reset=0)
    outcomes = set()
    for t in range(steps):
        a = rng.integers(0, tables[5], N)
        if kind == "taxi" and t % 4 != 3:
            # uniformly random actions never deliver a passenger within 12 steps, so no episode would
            # terminate: three steps of four, every second env drives (shortest path on the product's
            # table), picks up and drops off; the others, and every fourth step, stay random
            for e in range(0, N, 2):
                a[e] = _taxi_driver(tables[0], int(twin.state[e]))
        seen["reset"] += int(twin.meta[:, 2].sum())
        r_t, d_t, to_t = twin.step(a)
        dev.step_into(rew, dn, to, actions=torch.as_tensor(a, dtype=torch.int64, device=cuda))
        outcomes |= set(twin.outcomes.tolist())
        seen["term"] += int((d_t & ~to_t.astype(bool)).sum())
        seen["trunc"] += int(to_t.sum())
        assert np.array_equal(dev.state.cpu().numpy(), twin.state), t
        assert np.array_equal(dev.meta.cpu().numpy(), twin.meta), t
        assert np.array_equal(dev.obs.cpu().numpy(), twin.obs()), t
        assert np.array_equal(rew.cpu().numpy(), r_t) and np.array_equal(dn.cpu().numpy(), d_t), t
        assert np.array_equal(to.cpu().numpy(), to_t), t
        assert np.array_equal(dev.ep_ret.cpu().numpy(), twin.ep_ret), t
    assert np.array_equal(dev.ep_count.cpu().numpy(), twin.ep_count)
    assert np.array_equal(dev.ep_ret_sum.cpu().numpy(), twin.ep_ret_sum)
    assert np.array_equal(dev.ep_len_sum.cpu().numpy(), twin.ep_len_sum)
    print(kind, encoding, seen, outcomes)
    assert min(seen.values()) >= 1, seen        # terminations, truncations and reset steps all occurred
    if slippery and kind == "frozenlake":
        assert {0, 1, 2} <= outcomes            # all three slippery outcomes


def test_env_offset_partitions_the_same_trajectories(cuda):
    """Envs 0..15 at env_offset 3 and envs 0..7 at env_offset 11 share global envs 11..18."""
    from gsamd.rollout import DeviceTabularVecEnv
    a_env = DeviceTabularVecEnv(16, kind="frozenlake", encoding="array", seed=9, env_offset=3, max_steps=9, device=cuda)
    b_env = DeviceTabularVecEnv(8, kind="frozenlake", encoding="array", seed=9, env_offset=11, max_steps=9, device=cuda)
    a_env.reset()
    b_env.reset()
    rng = np.random.default_rng(2)
    ra, rb = _rows(16, cuda), _rows(8, cuda)
    for _ in range(40):
        act = torch.as_tensor(rng.integers(0, 4, 16), dtype=torch.int64, device=cuda)
        a_env.step_into(*ra, actions=act)
        b_env.step_into(*rb, actions=act[8:].contiguous())
        assert torch.equal(a_env.state[8:], b_env.state) and torch.equal(a_env.meta[8:], b_env.meta)
        assert all(torch.equal(x[8:], y) for x, y in zip(ra, rb))


def test_slippery_outcomes_are_equiprobable(cuda):
    """3 x 10^4 draws from the interior state 9 of the 8x8 map under RIGHT (every neighbour is
    frozen, so the three outcomes DOWN / RIGHT / UP land on three distinct states): each share
    lies within 4 sigma of 1/3, sigma = sqrt((1/3)(2/3)/n) -> +-0.011."""
    from gsamd import toytext
    from gsamd.rollout import DeviceTabularVecEnv
    n = 30000
    nxt = toytext.frozenlake_table("8x8", True)[0]
    s0, act = 9, 2
    targets = nxt[s0, act].tolist()
    assert len(set(targets)) == 3 and s0 not in targets
    dev = DeviceTabularVecEnv(n, kind="frozenlake", encoding="array", map_name="8x8", is_slippery=True, seed=3,
                              device=cuda)
    dev.reset()
    dev.state.fill_(s0)
    rew, dn, to = _rows(n, cuda)
    dev.step_into(rew, dn, to, actions=torch.full((n,), act, dtype=torch.int64, device=cuda))
    got = dev.state.cpu().numpy()
    shares = np.array([(got == t).mean() for t in targets])
    print("outcome shares", shares)
    assert abs(shares.sum() - 1.0) < 1e-12
    bound = 4.0 * np.sqrt((1 / 3) * (2 / 3) / n)
    assert bound < 0.011 and (np.abs(shares - 1 / 3) <= bound).all(), shares


def test_bad_tables_and_actions_stay_inside_the_tables(cuda):
    """Range checks: actions outside [0, A) are clamped; a next state outside [0, S) ends the
    episode in place; a onehot of more than 64 states is refused."""
    from gsamd import toytext
    from gsamd.rollout import DeviceTabularVecEnv
    nxt, rew, term, starts, S, A, K = toytext.frozenlake_table("4x4", False)
    bad = nxt.copy()
    bad[0, 2, 0] = 1 << 20          # RIGHT from the start: a wild next state
    bad[0, 1, 0] = -5
    dev = DeviceTabularVecEnv(4, kind="frozenlake", encoding="array", tables=(bad, rew, term, starts, S, A, K), seed=1,
                              device=cuda)
    dev.reset()
    r, d, t = _rows(4, cuda)
    dev.step_into(r, d, t, actions=torch.tensor([2, 1, 99, -7], dtype=torch.int64, device=cuda))
    assert dev.state.tolist() == [0, 0, 0, 0]           # 99 -> UP (clamped to 3), -7 -> LEFT: both stay at 0
    assert d.tolist() == [1, 1, 0, 0] and t.tolist() == [0, 0, 0, 0]
    taxi = DeviceTabularVecEnv(4, kind="taxi", encoding="onehot", device=cuda)
    with pytest.raises(ValueError, match="exceed"):
        taxi.reset()


def test_rollout_graph_equals_eager_with_the_tabular_env(cuda):
    """The captured T-step rollout equals the eager per-step launches bit for bit with the tabular
    env and a one-hidden-layer policy (the pattern of test_rollout_graph_equals_eager); the
    collector takes the step-graph path: no one-launch rollout for one hidden layer."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    from gsamd.rollout import DeviceTabularVecEnv
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(42)
        cfg = load_config("FrozenLake-v1", "ppo", overrides=dict(n_envs=24, n_steps=32, batch_size=64, n_epochs=2,
                                                                 max_episode_steps=10))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=True)
        coll = agent.get_rollout_collector("train")
        assert isinstance(coll.env, DeviceTabularVecEnv) and not coll.one_launch
        assert not coll._one_launch_supported(coll.env, agent.policy_model)
        assert agent.policy_model.dims.hidden2 == 0 and agent.policy_model.n_params == 453
        rec = []
        for _ in range(4):
            agent.train_epoch()
            b = coll.buffer
            rec.append([t.clone() for t in (b.obs, b.actions, b.logprobs, b.values, b.rewards, b.dones, b.timeouts,
                                            b.advantages, b.returns)])
        coll.collect(deterministic=True)
        coll.collect(deterministic=True)
        rec.append([coll.buffer.actions.clone(), coll.buffer.values.clone()])
        torch.cuda.synchronize()
        runs.append((rec, coll.get_metrics(), coll.total_vec_steps, agent.policy_model.params.clone()))
        assert (coll._graphs.get(0) is not None) == use_graph
        del agent
    (r0, m0, n0, p0), (r1, m1, n1, p1) = runs
    assert n0 == n1 and torch.equal(p0, p1)
    for k, (a, b) in enumerate(zip(r0, r1)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert m0["cnt/total_episodes"] == m1["cnt/total_episodes"] > 0
    assert m0.get("roll/ep_rew/mean") == m1.get("roll/ep_rew/mean")


@pytest.mark.parametrize("env,variant", IDS)
def test_agent_trains_through_the_public_entry(cuda, env, variant, tmp_path):
    """build_agent on the resolved config with no env=: two epochs train with finite losses and
    moving weights on the device tabular env; the records carry backbone.0's activation
    statistics and the three component norms; the finished episodes obey the env's reward rules;
    the checkpoint round trip speaks the reference's one-hidden-layer keys."""
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.rollout import DeviceTabularVecEnv
    torch.manual_seed(42)
    over = dict(n_envs=8, n_steps=64, batch_size=64, n_epochs=2)
    agent = build_agent(load_config(env, variant, overrides=over), device=cuda)
    e, coll = agent.get_env("train"), agent.get_rollout_collector("train")
    assert isinstance(e, DeviceTabularVecEnv) and not coll.one_launch
    assert agent.policy_model.hidden_dims == (64,) and agent.policy_model.obs_dim == 1
    p0 = agent.policy_model.params.clone()
    for _ in range(2):
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all() and agent.adam_step == 2 * 16
    assert not torch.equal(p0, agent.policy_model.params)
    m = agent.epoch_metrics()
    assert m["opt/grads/norm/all"] > 0 and m["opt/grads/norm/backbone"] > 0
    assert {"opt/activations/backbone.0/mean", "opt/activations/backbone.0/dead_max"} <= set(m)
    assert not any(k.startswith("opt/activations/backbone.2") for k in m)
    obs = coll.buffer.obs.cpu().numpy()
    assert obs.min() >= 0 and obs.max() < e.n_states and np.array_equal(obs, np.round(obs))
    for _, ret, length, timeout in coll._recent_episodes:
        if e.kind == "frozenlake":
            assert ret in (0.0, 1.0) and 1 <= length <= 101
        else:
            assert -10.0 * 201 <= ret <= 20.0 and 1 <= length <= 201
    assert int(e.ep_count.sum()) == len(coll._recent_episodes)
    # checkpoint round trip
    agent.save_checkpoint(tmp_path)
    sd = torch.load(tmp_path / "model.pt", weights_only=True)
    assert list(sd) == ["backbone.0.weight", "backbone.0.bias", "policy_head.weight", "policy_head.bias",
                        "value_head.weight", "value_head.bias"]
    assert tuple(sd["backbone.0.weight"].shape) == (64, 1) and tuple(sd["policy_head.weight"].shape) == (e.n_actions, 64)
    torch.manual_seed(7)
    other = build_agent(load_config(env, variant, overrides=over), device=cuda)
    assert not torch.equal(other.policy_model.params, agent.policy_model.params)
    other.load_checkpoint(tmp_path)
    assert torch.equal(other.policy_model.params, agent.policy_model.params)
    assert torch.equal(other.adam_m, agent.adam_m) and torch.equal(other.adam_v, agent.adam_v)
    assert other.adam_step == agent.adam_step
