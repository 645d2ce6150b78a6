"""GPU: device Acrobot-v1 — the step kernel against the float64 twin (tests/acrobot_twin.py),
the one-launch rollout on real dynamics (Acrobot, CartPole) against the per-step loop, the
captured step graph against eager launches, and training / evaluation through the public entry."""
import math

import numpy as np
import pytest
import torch

import acrobot_twin as T

pytestmark = pytest.mark.gpu

PI = math.pi


def _box_states(rng, n):
    """States uniform over the whole box: angles in [-pi, pi], w1 in +-4 pi, w2 in +-9 pi."""
    return np.stack([rng.uniform(-PI, PI, n), rng.uniform(-PI, PI, n), rng.uniform(-T.MAX_VEL_1, T.MAX_VEL_1, n),
                     rng.uniform(-T.MAX_VEL_2, T.MAX_VEL_2, n)], axis=1)


def _ang_diff(a, b):
    return (a - b + PI) % (2.0 * PI) - PI


def test_step_kernel_matches_twin_teacher_forced(cuda):
    """f1: gs_acrobot_step against the twin, one step at a time from the device's own state (the
    system is chaotic: a free run amplifies last-bit sin / cos differences past any useful bar).
    N = 272 (two blocks, ragged), max_steps 25, 120 steps of random actions; every 10 steps the
    states are redrawn over the whole box, so that terminations, truncations, both wraps (multi-
    turn ones too), both velocity clamps and reset steps all occur (counted on the twin).
    Bars: reward / done / timeout rows and meta exact; the state after a reset step bit-equal;
    new angles 1e-9 modulo 2 pi and new velocities 1e-9 absolute (six orders above double
    rounding at |x| <= 30, three below float32 resolution); observations 1e-5 absolute.  An
    env-step whose twin height is within 1e-9 of the line is left out of the flag comparison (at
    most one of the 32 640)."""
    from gsamd.rollout import DeviceAcrobotVecEnv
    N, STEPS, MAXS, SEED, OFF = 272, 120, 25, 3, 5
    env = DeviceAcrobotVecEnv(N, seed=SEED, env_offset=OFF, max_steps=MAXS, device=cuda)
    env.reset()
    torch.cuda.synchronize()
    st0 = env.state.cpu().numpy()
    want0 = np.array([[T.reset_uniform(SEED, OFF + e, 0, c) for c in range(4)] for e in range(N)])
    assert np.array_equal(st0, want0) and not env.meta.cpu().numpy().any()
    np.testing.assert_allclose(env.obs.cpu().numpy(), np.stack([T.obs_of(s) for s in want0]), atol=1e-5, rtol=0)
    rng = np.random.default_rng(0)
    r = torch.zeros(N, device=cuda)
    d = torch.zeros(N, dtype=torch.uint8, device=cuda)
    to = torch.zeros(N, dtype=torch.uint8, device=cuda)
    cnt = dict(term=0, trunc=0, wrap1=0, wrap2=0, clamp1=0, clamp2=0, multi=0, reset=0)
    skipped, worst_ang, worst_vel, worst_obs, min_gap = 0, 0.0, 0.0, 0.0, 1.0
    for t in range(STEPS):
        if t % 10 == 0:
            env.state.copy_(torch.as_tensor(_box_states(rng, N)).to(cuda))
        a = rng.integers(0, 3, N)
        s_in, m_in = env.state.cpu().numpy(), env.meta.cpu().numpy()
        env.step_into(r, d, to, actions=torch.as_tensor(a).to(cuda))
        torch.cuda.synchronize()
        s_out, m_out, o_out = env.state.cpu().numpy(), env.meta.cpu().numpy(), env.obs.cpu().numpy()
        rr, dd, tt = r.cpu().numpy(), d.cpu().numpy(), to.cpu().numpy()
        for e in range(N):
            steps, episodes, pending = (int(v) for v in m_in[e])
            if pending:
                cnt["reset"] += 1
                want = [T.reset_uniform(SEED, OFF + e, episodes, c) for c in range(4)]
                assert s_out[e].tolist() == want, (t, e)                       # bit-equal
                assert (rr[e], dd[e], tt[e]) == (0.0, 0, 0) and m_out[e].tolist() == [0, episodes, 0], (t, e)
            else:
                want, term, info = T.step_state(s_in[e].tolist(), a[e])
                gap = abs(T.height(want) - 1.0)
                min_gap = min(min_gap, gap)
                trunc = (not term) and steps + 1 >= MAXS
                for k in ("wrap1", "wrap2"):
                    cnt[k] += info[k] > 0
                cnt["multi"] += info["wrap1"] > 1 or info["wrap2"] > 1
                cnt["clamp1"] += info["clamp1"]
                cnt["clamp2"] += info["clamp2"]
                cnt["term"] += term
                cnt["trunc"] += trunc
                worst_ang = max(worst_ang, abs(_ang_diff(s_out[e][0], want[0])), abs(_ang_diff(s_out[e][1], want[1])))
                worst_vel = max(worst_vel, abs(s_out[e][2] - want[2]), abs(s_out[e][3] - want[3]))
                if gap < 1e-9:
                    skipped += 1          # the flag may fall either way; meta is re-read from the device
                else:
                    done = term or trunc
                    assert (rr[e], dd[e], tt[e]) == (0.0 if term else -1.0, int(done), int(trunc)), (t, e)
                    assert m_out[e].tolist() == [steps + 1, episodes + int(done), int(done)], (t, e)
            worst_obs = max(worst_obs, float(np.abs(o_out[e] - T.obs_of(want)).max()))
    print("counts", cnt, "skipped", skipped, "worst angle", worst_ang, "velocity", worst_vel, "obs", worst_obs,
          "min |h - 1|", min_gap)
    assert worst_ang <= 1e-9 and worst_vel <= 1e-9 and worst_obs <= 1e-5
    assert skipped <= 1
    assert all(v >= 1 for v in cnt.values()), cnt


def _seed_box(env, seed=11):
    """The same box states into env.state (and their observations into env.obs) in every arm."""
    s = _box_states(np.random.default_rng(seed), env.num_envs)
    env.state.copy_(torch.as_tensor(s).to(env.device))
    o = np.stack([T.obs_of(x) for x in s.tolist()])
    env.obs.copy_(torch.as_tensor(o).to(env.device))


@pytest.mark.parametrize("env,variant,over", [
    ("Acrobot-v1", "ppo", dict(n_envs=40, n_steps=64, batch_size=64, n_epochs=2, max_episode_steps=20)),
    ("CartPole-v1", "ppo", dict(env_dynamics="cartpole", model_id="mlp_small", n_envs=40, n_steps=64, batch_size=64,
                                n_epochs=2, max_episode_steps=20))])
def test_one_launch_rollout_on_real_dynamics_equals_step_loop(cuda, env, variant, over):
    """gs_rollout_env (the whole rollout in one launch, envs resident in registers / LDS) writes
    bit for bit the rows of the per-step loop (gs_policy_act + the env's step kernel): sampled,
    deterministic and replayed actions, over rollouts separated by updates, a ragged last
    workgroup (N % 16 != 0), and leaves the same env state, meta, observations and episode
    counters.  Acrobot starts from states over the whole box, so that terminations and reset
    steps run inside the launch."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for one in (False, True):
        torch.manual_seed(42)
        cfg = load_config(env, variant, overrides=dict(over))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=True, one_launch=one)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch == one
        coll._prepare()
        if env == "Acrobot-v1":
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
        rec.append([t.clone() for t in (e.state, e.meta, e.ep_ret, e.obs, e.ep_count, e.ep_ret_sum, e.ep_len_sum)])
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
    if env == "Acrobot-v1":
        assert int((first[5].bool() & ~first[6].bool()).sum()) > 0     # by termination, not only the time limit


def test_acrobot_rollout_graph_equals_eager(cuda):
    """The captured T-step rollout of device Acrobot (policy act + gs_acrobot_step per vector
    step) writes bit for bit the rollout of the eager per-step launches — sampled and
    deterministic actions, over several rollouts, between updates that move the weights."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(42)
        cfg = load_config("Acrobot-v1", "ppo", overrides=dict(n_envs=48, n_steps=64, batch_size=64, n_epochs=2,
                                                              max_episode_steps=20))
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
        rec.append([t.clone() for t in (e.state, e.meta, e.obs)])
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


_SMALL = dict(n_envs=32, n_steps=128, batch_size=64, n_epochs=2, max_episode_steps=50)


def test_agent_trains_on_device_acrobot_through_the_public_entry(cuda):
    """build_agent on the resolved Acrobot-v1:ppo with no env=: three epochs train with finite
    losses on the one-launch rollout, and every recorded episode's return follows from its
    length: -1 per env step, 0 on a terminating step, so -steps if truncated, else -(steps - 1).
    The collector's recorded length counts rollout rows, which for every episode after an env's
    first include the autoreset transition (reward 0, as for CartPole): steps = length - 1
    there.  The env's own counters must add up to the same episodes."""
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.rollout import DeviceAcrobotVecEnv
    torch.manual_seed(42)
    agent = build_agent(load_config("Acrobot-v1", "ppo", overrides=dict(_SMALL)), device=cuda)
    coll = agent.get_rollout_collector("train")
    assert isinstance(agent.get_env("train"), DeviceAcrobotVecEnv) and coll.one_launch
    for _ in range(3):
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all()
    m = coll.get_metrics()
    assert m["cnt/total_episodes"] > 0 and m["cnt/total_episodes"] == len(coll._recent_episodes)
    seen, steps_sum, ret_sum = set(), 0, 0.0
    for env, ret, length, timeout in coll._recent_episodes:
        steps = length - (1 if env in seen else 0)
        seen.add(env)
        assert 1 <= steps <= 50 and timeout == (steps == 50 and ret == -50.0)
        assert ret == (-float(steps) if timeout else -float(steps - 1)), (env, ret, length, timeout)
        steps_sum += steps
        ret_sum += ret
    e = coll.env
    assert int(e.ep_count.sum()) == len(coll._recent_episodes)
    assert float(e.ep_len_sum.sum()) == steps_sum and float(e.ep_ret_sum.sum()) == ret_sum


def test_acrobot_evaluate_episodes_keys_and_counts(cuda):
    from gsamd import build_agent
    from gsamd.config import load_config
    torch.manual_seed(42)
    agent = build_agent(load_config("Acrobot-v1", "ppo", overrides=dict(_SMALL, max_episode_steps=30)), device=cuda)
    out = agent.get_rollout_collector("val").evaluate_episodes(n_episodes=8, deterministic=True)
    assert out["cnt/total_episodes"] == 8
    assert {"roll/ep_rew/mean", "roll/ep_len/mean", "cnt/total_env_steps", "cnt/total_vec_steps"} <= set(out)
    assert 1 <= out["roll/ep_len/mean"] <= 30 and -30 <= out["roll/ep_rew/mean"] <= 0
