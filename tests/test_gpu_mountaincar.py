"""GPU: device MountainCar-v0 with its reward wrappers — the step kernel against the float64 twin
(tests/mountaincar_twin.py) and against the reference's own wrapper classes
(tests/golden/mountaincar_wrappers.npz), the one-launch rollout against the per-step loop, the
captured step graph against eager launches, and training / evaluation through the public entry."""
import json
import os

import numpy as np
import pytest
import torch

import mountaincar_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH = {"id": T.SHAPER, "position_reward_scale": 100.0, "velocity_reward_scale": 10.0, "height_reward_scale": 50.0}
BO = {"id": T.BONUS, "position_bins": 50, "velocity_bins": 50, "bonus_scale": 0.1, "bonus_type": "count"}


@pytest.mark.parametrize("wrappers", [[], [SH, dict(BO, position_bins=12, velocity_bins=9)]], ids=["bare", "both"])
def test_step_kernel_matches_twin_teacher_forced(cuda, wrappers):
    """gs_mountaincar_step against the twin, one step at a time from the device's own state.
    N = 272 (two blocks, ragged), max_steps 25, 120 steps of random actions; every 10 steps the
    states are redrawn over the box (a share at the wall, at the goal, at both speed caps; the
    shaper's prev slots follow the redrawn state), so that terminations, truncations, wall stops,
    both clamps and reset steps all occur (counted on the twin).
    Bars: new p and v 1e-12 absolute (the device cos may differ from the twin's in the last bit,
    ~1e-18 here); flags and meta exact; the state after a reset bit-equal; rewards 2e-6 with the
    twin's wrappers fed the device's own observations; tables and prev slots exact.  A step whose
    twin value lies within 1e-12 of a threshold is left out of the flag comparison (at most one;
    the CPU test shows the twin has none for this seed)."""
    from gsamd.rollout import DeviceMountainCarVecEnv
    c = T.KERNEL_CASE
    N, STEPS, MAXS, SEED, OFF = c["N"], c["steps"], c["max_steps"], c["seed"], c["env_offset"]
    env = DeviceMountainCarVecEnv(N, seed=SEED, env_offset=OFF, max_steps=MAXS, wrappers=wrappers, device=cuda)
    env.counts.fill_(7)                   # reset() zeroes the tables
    env.reset()
    torch.cuda.synchronize()
    st0 = env.state.cpu().numpy()
    want0 = np.array([T.reset_state(SEED, OFF + e, 0) for e in range(N)])
    assert np.array_equal(st0[:, :2], want0) and not env.meta.cpu().numpy().any()
    assert np.array_equal(st0[:, 2:], want0.astype(np.float32).astype(np.float64))
    assert np.array_equal(env.obs.cpu().numpy(), want0.astype(np.float32)) and not env.counts.cpu().numpy().any()
    wraps = [T.Wrappers(wrappers) for _ in range(N)]
    for e in range(N):
        wraps[e].reset(T.obs_of(want0[e]))
    rng = np.random.default_rng(c["rng"])
    r = torch.zeros(N, device=cuda)
    d = torch.zeros(N, dtype=torch.uint8, device=cuda)
    to = torch.zeros(N, dtype=torch.uint8, device=cuda)
    cnt = dict(term=0, trunc=0, wall=0, clamp_lo=0, clamp_hi=0, reset=0)
    skipped, worst_s, worst_r = 0, 0.0, 0.0
    for t in range(STEPS):
        if t % c["redraw"] == 0:
            s = T.box_states(rng, N)
            prev = s.astype(np.float32).astype(np.float64)
            env.state.copy_(torch.as_tensor(np.concatenate([s, prev], axis=1)).to(cuda))
            for e in range(N):
                wraps[e].reset(prev[e])
        a = rng.integers(0, 3, N)
        s_in, m_in = env.state.cpu().numpy(), env.meta.cpu().numpy()
        env.step_into(r, d, to, actions=torch.as_tensor(a).to(cuda))
        torch.cuda.synchronize()
        s_out, m_out, o_out = env.state.cpu().numpy(), env.meta.cpu().numpy(), env.obs.cpu().numpy()
        rr, dd, tt = r.cpu().numpy(), d.cpu().numpy(), to.cpu().numpy()
        assert np.array_equal(o_out, s_out[:, :2].astype(np.float32)), t
        assert np.array_equal(s_out[:, 2:], o_out.astype(np.float64)), t           # the prev slots
        for e in range(N):
            steps, episodes, pending = (int(v) for v in m_in[e])
            if pending:
                cnt["reset"] += 1
                assert s_out[e][:2].tolist() == T.reset_state(SEED, OFF + e, episodes), (t, e)      # bit-equal
                assert (rr[e], dd[e], tt[e]) == (0.0, 0, 0) and m_out[e].tolist() == [0, episodes, 0], (t, e)
                wraps[e].reset(o_out[e])
                continue
            want, term, info = T.step_state(s_in[e][:2].tolist(), a[e])
            trunc = (not term) and steps + 1 >= MAXS
            for k in ("wall", "clamp_lo", "clamp_hi"):
                cnt[k] += bool(info[k])
            cnt["term"] += term
            cnt["trunc"] += trunc
            worst_s = max(worst_s, abs(s_out[e][0] - want[0]), abs(s_out[e][1] - want[1]))
            if T.threshold_gap(s_in[e][:2].tolist(), a[e]) < 1e-12:
                skipped += 1          # the flag may fall either way; meta is re-read from the device
            else:
                done = term or trunc
                assert (dd[e], tt[e]) == (int(done), int(trunc)), (t, e)
                assert m_out[e].tolist() == [steps + 1, episodes + int(done), int(done)], (t, e)
            worst_r = max(worst_r, abs(float(rr[e]) - wraps[e].step(o_out[e])))
            if not wrappers:
                assert rr[e] == -1.0, (t, e)
    print("counts", cnt, "skipped", skipped, "worst state", worst_s, "worst reward", worst_r)
    assert worst_s <= 1e-12 and worst_r <= 2e-6
    assert skipped <= 1
    assert all(v >= 1 for v in cnt.values()), cnt
    if wraps[0].table is not None:
        assert np.array_equal(env.counts.cpu().numpy(), np.stack([w.table for w in wraps]))
    else:
        assert env.counts.numel() == 0


def test_entries_refuse_wrappers_that_could_leave_the_table(cuda):
    """The C entries check the wrapper struct themselves (the Python class already refuses such a
    list): a count bonus without its table, bins past 16384 cells, min_count 0, an id twice."""
    from gsamd.rollout import DeviceMountainCarVecEnv
    env = DeviceMountainCarVecEnv(16, wrappers=[BO], device=cuda)
    env.reset()
    r = torch.zeros(16, device=cuda)
    d = torch.zeros(16, dtype=torch.uint8, device=cuda)
    a = torch.zeros(16, dtype=torch.int64, device=cuda)
    for field, bad in (("min_count", 0), ("position_bins", 400), ("velocity_bins", 0), ("bonus_type", 3)):
        good = getattr(env.wrappers_c, field)
        setattr(env.wrappers_c, field, bad)
        with pytest.raises(ValueError, match="gs_mountaincar_step"):
            env.step_into(r, d, d.clone(), actions=a)
        setattr(env.wrappers_c, field, good)
    env.wrappers_c.order[1] = 2
    with pytest.raises(ValueError, match="twice"):
        env.step_into(r, d, d.clone(), actions=a)
    env.wrappers_c.order[1] = 0
    counts, env.counts = env.counts, env.counts[:, :0]
    with pytest.raises(ValueError, match="table"):
        env.step_into(r, d, d.clone(), actions=a)
    env.counts = counts
    env.step_into(r, d, d.clone(), actions=a)
    torch.cuda.synchronize()
    assert int(env.counts.sum()) == 16


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mountaincar_wrappers.npz"))
    d = {k: z[k] for k in z.files}
    d["configs"] = json.loads(str(d["configs"]))
    return d


@pytest.mark.parametrize("name", ["shaper", "bonus_count", "bonus_inverse", "bonus_log", "shaper_bonus", "bonus_shaper"])
def test_device_wrappers_match_reference_classes(cuda, fx, name):
    """The device against the reference's own wrapper classes: {p, v} is set to the fixture's
    pre-step state before each step and the fixture's actions are replayed.  Observations
    bit-equal in every row; rewards within 5e-5 where a shaper is in the stack (the reference's
    values carry numpy 2's float32 rounding, (100 + 10 + 50) * 4 * 2^-24 = 3.8e-5 at most), within
    2.4e-7 (two float32 ulps at 1) for a bonus alone; final tables exact."""
    from gsamd.rollout import DeviceMountainCarVecEnv
    wrappers = fx["configs"][name]
    S, N = fx["action"].shape
    env = DeviceMountainCarVecEnv(N, seed=int(fx["seed"]), env_offset=int(fx["env_offset"]),
                                  max_steps=int(fx["max_steps"]), wrappers=wrappers, device=cuda)
    env.reset()
    assert np.array_equal(env.obs.cpu().numpy(), fx["obs0"])
    r = torch.zeros(N, device=cuda)
    d = torch.zeros(N, dtype=torch.uint8, device=cuda)
    to = torch.zeros(N, dtype=torch.uint8, device=cuda)
    state, action = torch.as_tensor(fx["state"]).to(cuda), torch.as_tensor(fx["action"]).to(cuda)
    got_r, got_o, got_d, got_reset = [], [], [], []
    for t in range(S):
        env.state[:, :2].copy_(state[t])
        got_reset.append(env.meta[:, 2].clone())
        env.step_into(r, d, to, actions=action[t])
        got_r.append(r.clone())
        got_o.append(env.obs.clone())
        got_d.append(torch.stack([d, to]).clone())
    torch.cuda.synchronize()
    got_r, got_o = torch.stack(got_r).cpu().numpy(), torch.stack(got_o).cpu().numpy()
    got_d, got_reset = torch.stack(got_d).cpu().numpy(), torch.stack(got_reset).cpu().numpy()
    assert np.array_equal(got_reset.astype(bool), fx["reset"])
    assert np.array_equal(got_o, fx["obs"])                                     # bit-equal, every row
    assert np.array_equal(got_d[:, 0].astype(bool), fx["done"]) and np.array_equal(got_d[:, 1].astype(bool), fx["trunc"])
    worst = float(np.abs(got_r.astype(np.float64) - fx[f"reward_{name}"].astype(np.float64)).max())
    print(name, "worst |device - reference| reward", worst)
    assert worst <= (5e-5 if "shaper" in name else 2.4e-7)
    assert np.all(got_r[fx["reset"]] == 0.0)
    if f"table_{name}" in fx:
        assert np.array_equal(env.counts.cpu().numpy(), fx[f"table_{name}"])


def _seed_box(env, seed=11):
    """The same box states into env.state (prev slots and observations following) in every arm."""
    s = T.box_states(np.random.default_rng(seed), env.num_envs)
    o = s.astype(np.float32)
    env.state.copy_(torch.as_tensor(np.concatenate([s, o.astype(np.float64)], axis=1)).to(env.device))
    env.obs.copy_(torch.as_tensor(o).to(env.device))


_ONE = dict(model_id="mlp_small", n_envs=40, n_steps=64, batch_size=64, n_epochs=2, max_episode_steps=20)


@pytest.mark.parametrize("variant,over", [("ppo_curiosity", dict(_ONE)), ("ppo", dict(_ONE, env_wrappers=[SH, BO]))],
                         ids=["curiosity", "both"])
def test_one_launch_rollout_equals_step_loop(cuda, variant, over):
    """gs_rollout_mountaincar (the whole rollout in one launch, the count tables in HBM) writes bit
    for bit the rows of the per-step loop (gs_policy_act + gs_mountaincar_step): sampled,
    deterministic and replayed actions, over rollouts separated by updates, a ragged last
    workgroup (N % 16 != 0), and leaves the same env state, meta, observations, episode counters
    and count tables.  The envs start from states over the whole box, so that terminations and
    reset steps run inside the launch."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for one in (False, True):
        torch.manual_seed(42)
        cfg = load_config("MountainCar-v0", variant, overrides=dict(over))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=True, one_launch=one)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch == one
        coll._prepare()
        _seed_box(coll.env)
        rec = []
        for k in range(3):
            agent.train_epoch()
            b = coll.buffer
            rec.append([t.clone() for t in (b.obs, b.actions, b.logprobs, b.values, b.rewards, b.dones, b.timeouts,
                                            b.advantages, b.returns)])
        coll.collect(deterministic=True)
        rec.append([t.clone() for t in (coll.buffer.actions, coll.buffer.logprobs, coll.buffer.values)])
        replay = torch.randint(0, coll.env.n_actions, coll.buffer.actions.shape, device=coll.buffer.actions.device,
                               generator=torch.Generator(device=coll.buffer.actions.device).manual_seed(7))
        coll.collect(replay_actions=replay)
        rec.append([t.clone() for t in (coll.buffer.actions, coll.buffer.logprobs, coll.buffer.values,
                                        coll.buffer.rewards, coll.buffer.dones, coll.buffer.timeouts)])
        e = coll.env
        rec.append([t.clone() for t in (e.state, e.meta, e.ep_ret, e.obs, e.ep_count, e.ep_ret_sum, e.ep_len_sum,
                                        e.counts)])
        torch.cuda.synchronize()
        runs.append((rec, coll.get_metrics(), coll.total_vec_steps))
        del agent
    (r0, m0, n0), (r1, m1, n1) = runs
    assert n0 == n1
    for k, (a, b) in enumerate(zip(r0, r1)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (k, j)
    assert m0["cnt/total_episodes"] == m1["cnt/total_episodes"] > 0
    first = r1[0]
    assert int(first[5].sum()) > 0                                 # episodes ended inside the first launch
    assert int((first[5].bool() & ~first[6].bool()).sum()) > 0     # by termination, not only the time limit
    counts = r1[-1][-1]
    assert counts.shape == (40, 2500) and int(counts.sum()) > 0


def test_default_policy_does_not_take_the_one_launch_path(cuda):
    """The reference's MountainCar configs use mlp_medium (256, 256), which does not fit in LDS:
    the collector reports the step loop."""
    from gsamd import build_agent
    from gsamd.config import load_config
    agent = build_agent(load_config("MountainCar-v0", "ppo_curiosity", overrides=dict(n_steps=64)), device=cuda)
    assert agent.get_rollout_collector("train").one_launch is False


def test_mountaincar_rollout_graph_equals_eager(cuda):
    """The captured T-step rollout of device MountainCar (policy act + gs_mountaincar_step per
    vector step) writes bit for bit the rollout of the eager per-step launches, count tables
    included — sampled and deterministic actions, over several rollouts, between updates."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(42)
        cfg = load_config("MountainCar-v0", "ppo_curiosity", overrides=dict(
            n_envs=48, n_steps=64, batch_size=64, n_epochs=2, max_episode_steps=20))
        assert cfg.model_id == "mlp_medium"
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=True, one_launch=False)
        coll = agent.get_rollout_collector("train")
        assert not coll.one_launch
        rec = []
        for k in range(4):
            agent.train_epoch()
            b = coll.buffer
            rec.append([t.clone() for t in (b.obs, b.actions, b.logprobs, b.values, b.rewards, b.dones, b.timeouts,
                                            b.advantages, b.returns)])
        coll.collect(deterministic=True)
        coll.collect(deterministic=True)
        rec.append([coll.buffer.actions.clone(), coll.buffer.values.clone()])
        e = coll.env
        rec.append([t.clone() for t in (e.state, e.meta, e.obs, e.counts)])
        torch.cuda.synchronize()
        runs.append((rec, coll.get_metrics(), coll.total_vec_steps))
        assert (coll._graphs.get(0) is not None) == use_graph
        del agent
    (r0, m0, n0), (r1, m1, n1) = runs
    assert n0 == n1
    for k, (a, b) in enumerate(zip(r0, r1)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert m0["cnt/total_episodes"] == m1["cnt/total_episodes"] > 0
    assert m0.get("roll/ep_rew/mean") == m1.get("roll/ep_rew/mean")
    assert int(r1[-1][-1].sum()) > 0


_SMALL = dict(n_envs=32, n_steps=128, batch_size=64, n_epochs=2, max_episode_steps=50)


def _train(cuda, variant, over):
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.rollout import DeviceMountainCarVecEnv
    torch.manual_seed(42)
    agent = build_agent(load_config("MountainCar-v0", variant, overrides=dict(_SMALL, **over)), device=cuda)
    coll = agent.get_rollout_collector("train")
    assert isinstance(agent.get_env("train"), DeviceMountainCarVecEnv)
    for _ in range(3):
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all()
    m = coll.get_metrics()
    assert m["cnt/total_episodes"] > 0 and m["cnt/total_episodes"] == len(coll._recent_episodes)
    return agent, coll


def _episodes(coll):
    """(env steps, return, timeout) per recorded episode.  The collector's recorded length counts
    rollout rows, which for every episode after an env's first include the autoreset transition
    (reward 0, as for CartPole and Acrobot): steps = length - 1 there."""
    seen = set()
    for env, ret, length, timeout in coll._recent_episodes:
        steps = length - (1 if env in seen else 0)
        seen.add(env)
        assert 1 <= steps <= 50 and (not timeout or steps == 50)
        yield steps, ret, timeout


def test_agent_trains_on_bare_mountaincar_through_the_public_entry(cuda):
    """build_agent on MountainCar-v0:ppo with env_wrappers=[] and no env=: three epochs train with
    finite losses and every episode's return is -steps exactly (-1 per step, the terminating one
    included).  The env's own counters add up to the same episodes."""
    agent, coll = _train(cuda, "ppo", dict(env_wrappers=[]))
    steps_sum, ret_sum = 0, 0.0
    for steps, ret, _ in _episodes(coll):
        assert ret == -float(steps)
        steps_sum += steps
        ret_sum += ret
    e = coll.env
    assert e.counts.numel() == 0
    assert int(e.ep_count.sum()) == len(coll._recent_episodes)
    assert float(e.ep_len_sum.sum()) == steps_sum and float(e.ep_ret_sum.sum()) == ret_sum


def test_agent_trains_on_curiosity_mountaincar_through_the_public_entry(cuda):
    """MountainCar-v0:ppo_curiosity as resolved: every step adds a bonus in (0, 0.1], so an
    episode's return lies in (-steps, -steps + 0.1 steps]; the tables hold one visit per
    non-reset env step (every env's resets = its finished episodes minus a pending one)."""
    agent, coll = _train(cuda, "ppo_curiosity", {})
    for steps, ret, _ in _episodes(coll):
        assert -float(steps) < ret <= -float(steps) + 0.1 * steps, (steps, ret)
    e = coll.env
    rows = coll.total_vec_steps * e.num_envs
    resets = int(e.ep_count.sum()) - int(e.meta[:, 2].sum())
    assert int(e.counts.sum()) == rows - resets and resets > 0
    assert int((e.counts.sum(dim=1) > 0).sum()) == e.num_envs


def test_mountaincar_evaluate_episodes_keys_and_counts(cuda):
    from gsamd import build_agent
    from gsamd.config import load_config
    torch.manual_seed(42)
    agent = build_agent(load_config("MountainCar-v0", "ppo_curiosity", overrides=dict(_SMALL, max_episode_steps=30)),
                        device=cuda)
    out = agent.get_rollout_collector("val").evaluate_episodes(n_episodes=8, deterministic=True)
    assert out["cnt/total_episodes"] == 8
    assert {"roll/ep_rew/mean", "roll/ep_len/mean", "cnt/total_env_steps", "cnt/total_vec_steps"} <= set(out)
    assert 1 <= out["roll/ep_len/mean"] <= 30 and -30 <= out["roll/ep_rew/mean"] <= 0
