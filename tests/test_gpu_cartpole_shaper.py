"""GPU: device CartPole-v1 under the reference's CartPoleV1_RewardShaper — the step kernel against
the reference's own class (tests/golden/cartpole_shaper.npz), the one-launch rollout against the
per-step loop, the captured step graph against eager launches, training through the public entry,
and the unshaped env left as it was."""
import json
import os

import numpy as np
import pytest
import torch

import cartpole_shaper_twin as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPER_ID = "CartPoleV1_RewardShaper"


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "cartpole_shaper.npz"))
    d = {k: z[k] for k in z.files}
    d["params"] = json.loads(str(d["params"]))
    return d


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("N", [37, 300])
@pytest.mark.parametrize("name", ["default", "scaled", "noclip"])
def test_step_kernel_matches_reference_class(cuda, fx, name, N):
    """gs_cartpole_shaped_step against the reference's own class, teacher-forced: the device state
    is set to the fixture's pre-step state before each step and the fixture's actions are replayed.
    Observations, flags and rewards are bit-equal (the shaper is the same double sequence on both
    sides), reset rows are exactly 0, prev_phi ends where the wrapper's does.

    N = 300 tiles the fixture's 37 envs over two workgroups.  Env e >= 37 has another global index
    than the fixture's env e % 37, so its reset observations (the counter hash) differ, and with
    them the potential the next reward is measured from.  Those envs are held to the Python
    restatement of the shaper (cartpole_shaper_twin, pinned bit for bit to the class on the same
    fixture, re-checked here) fed the device's own observations; their reset observations are
    held to the reset hash (oracle/cartpole_ref.py) and every other row to the fixture."""
    from gsamd.rollout import DeviceCartPoleVecEnv
    from oracle.cartpole_ref import reset_uniform
    kw = fx["params"][name]
    S, N0 = fx["action"].shape
    reps = -(-N // N0)
    tile = lambda a: np.concatenate([a] * reps, axis=1)[:, :N]           # noqa: E731
    seed, off, max_steps = int(fx["seed"]), int(fx["env_offset"]), int(fx["max_steps"])
    env = DeviceCartPoleVecEnv(N, seed=seed, env_offset=off, max_steps=max_steps,
                               wrappers=[dict(kw, id=SHAPER_ID)], device=cuda)
    env.reset()
    obs0 = env.obs.cpu().numpy()
    assert np.array_equal(obs0[:N0], fx["obs0"])
    want0 = np.array([[reset_uniform(seed, off + e, 0, c) for c in range(4)] for e in range(N)]).astype(np.float32)
    assert np.array_equal(_bits(obs0), _bits(want0))
    assert np.array_equal(env.prev_phi.cpu().numpy(), np.array([C.phi(o, **kw) for o in obs0]))
    r = torch.zeros(N, device=cuda)
    d = torch.zeros(N, dtype=torch.uint8, device=cuda)
    to = torch.zeros(N, dtype=torch.uint8, device=cuda)
    state, action = torch.as_tensor(tile(fx["state"])).to(cuda), torch.as_tensor(tile(fx["action"])).to(cuda)
    got_r, got_o, got_d, got_reset, got_meta = [], [], [], [], []
    for t in range(S):
        env.state.copy_(state[t])
        got_reset.append(env.meta[:, 2].clone())
        got_meta.append(env.meta.clone())
        env.step_into(r, d, to, actions=action[t])
        got_r.append(r.clone())
        got_o.append(env.obs.clone())
        got_d.append(torch.stack([d, to]).clone())
    torch.cuda.synchronize()
    got_r, got_o = torch.stack(got_r).cpu().numpy(), torch.stack(got_o).cpu().numpy()
    got_d, got_reset = torch.stack(got_d).cpu().numpy(), torch.stack(got_reset).cpu().numpy().astype(bool)
    got_meta = torch.stack(got_meta).cpu().numpy()
    reset = tile(fx["reset"])
    assert np.array_equal(got_reset, reset)
    assert np.array_equal(got_d[:, 0].astype(bool), tile(fx["done"]))
    assert np.array_equal(got_d[:, 1].astype(bool), tile(fx["trunc"]))
    # observations: the fixture's, bit for bit — on reset rows of the tiled copies, the reset hash
    want_o = tile(fx["obs"]).copy()
    for t, e in zip(*np.nonzero(reset)):
        if e >= N0:
            want_o[t, e] = [reset_uniform(seed, off + int(e), int(got_meta[t, e, 1]), c) for c in range(4)]
    assert np.array_equal(_bits(got_o), _bits(want_o))
    # rewards: the reference class's, bit for bit
    want_r = fx[f"reward_{name}"]
    assert np.array_equal(_bits(got_r[:, :N0]), _bits(want_r))
    assert np.all(got_r[reset] == 0.0)
    twin_r, twin_prev = C.shaped_rewards(obs0, got_o, reset, **kw)
    assert np.array_equal(_bits(twin_r[:, :N0]), _bits(want_r))         # the restatement is the class
    assert np.array_equal(_bits(got_r), _bits(twin_r))
    assert np.array_equal(env.prev_phi.cpu().numpy(), twin_prev)
    assert int(tile(fx["done"]).sum()) >= 5 and int(reset.sum()) >= 5


_ONE = dict(model_id="mlp_small", n_envs=40, n_steps=64, batch_size=64, n_epochs=2, max_episode_steps=20)


def test_one_launch_rollout_equals_step_loop(cuda):
    """gs_rollout_cartpole_shaped (the whole rollout in one launch) writes bit for bit the rows of
    the per-step loop (gs_policy_act + gs_cartpole_shaped_step): sampled, deterministic and
    replayed actions, over rollouts separated by updates, a ragged last workgroup (40 % 16 != 0),
    and leaves the same env state, prev_phi, meta, observations and episode counters."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for one in (False, True):
        torch.manual_seed(42)
        cfg = load_config("CartPole-v1", "ppo_rewardshaped", overrides=dict(_ONE))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=True, one_launch=one)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch == one and coll.env.prev_phi is not None
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
        rec.append([t.clone() for t in (e.state, e.prev_phi, e.meta, e.ep_ret, e.obs, e.ep_count, e.ep_ret_sum,
                                        e.ep_len_sum)])
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
    done, timeout = first[5].bool(), first[6].bool()
    assert int((done & ~timeout).sum()) > 0         # episodes ended inside the first launch by termination
    assert int((done & timeout).sum()) > 0          # and by the time limit
    assert int((first[4] != 1.0).sum()) > 0 and bool((first[4][0] != 1.0).any())      # the rewards are shaped


def test_resolved_config_takes_the_step_graph_and_it_equals_eager(cuda):
    """CartPole-v1:ppo_rewardshaped as resolved uses mlp_medium (256, 256), which does not fit in
    LDS: the collector reports the step loop, and its captured T-step graph (policy act +
    gs_cartpole_shaped_step per vector step) writes bit for bit the rollouts of eager launches."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(42)
        cfg = load_config("CartPole-v1", "ppo_rewardshaped")
        assert cfg.model_id == "mlp_medium"
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=use_graph, track_stats=True)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch is False
        rec = []
        for k in range(3):
            agent.train_epoch()
            b = coll.buffer
            rec.append([t.clone() for t in (b.obs, b.actions, b.logprobs, b.values, b.rewards, b.dones, b.timeouts,
                                            b.advantages, b.returns)])
        e = coll.env
        rec.append([t.clone() for t in (e.state, e.prev_phi, e.meta, e.obs, e.ep_ret)])
        torch.cuda.synchronize()
        runs.append((rec, coll.total_vec_steps))
        assert (coll._graphs.get(0) is not None) == use_graph
        del agent
    (r0, n0), (r1, n1) = runs
    assert n0 == n1 == 96
    for k, (a, b) in enumerate(zip(r0, r1)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
    assert int((r1[1][4] != 1.0).sum()) > 0


def test_agent_trains_on_shaped_cartpole_through_the_public_entry(cuda):
    """build_agent on CartPole-v1:ppo_rewardshaped with no env=: three epochs train with finite
    losses.  Potential-based shaping telescopes: an episode's return is steps + phi_last - phi_0
    with both potentials in [0, angle_reward_scale + position_reward_scale], so
    |return - steps| <= 1.25 + 1e-3; the 1e-3 covers the float32 accumulation of at most 50 rewards
    of magnitude at most 2.25 (50 * 50 * 2.25 * 2^-24 < 1e-3).
    A terminated episode ends beyond a threshold, where that term's potential is clipped to 0 (or,
    where the float32 observation rounds onto the threshold, is below 1e-7): phi_last <= max(1.0,
    0.25) + 1e-7, while phi_0 is the potential of a reset observation, |x|, |theta| < 0.05:
    phi_0 >= (1 - 0.05 / 0.2095) + 0.25 (1 - 0.05 / 2.4) > 1.006.  So its return is <= steps + 1e-3."""
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.rollout import DeviceCartPoleVecEnv
    torch.manual_seed(42)
    cfg = load_config("CartPole-v1", "ppo_rewardshaped", overrides=dict(n_envs=32, n_steps=128, batch_size=64,
                                                                        n_epochs=2, max_episode_steps=50))
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    env = agent.get_env("train")
    assert isinstance(env, DeviceCartPoleVecEnv) and env.wrappers_c is not None and env.max_steps == 50
    for _ in range(3):
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all()
    m = coll.get_metrics()
    assert m["cnt/total_episodes"] > 0 and m["cnt/total_episodes"] == len(coll._recent_episodes)
    seen, terminated, worst = set(), 0, 0.0
    for e, ret, length, timeout in coll._recent_episodes:
        steps = length - (1 if e in seen else 0)        # later episodes count their autoreset row
        seen.add(e)
        assert 1 <= steps <= 50 and (not timeout or steps == 50)
        worst = max(worst, abs(ret - steps))
        assert abs(ret - steps) <= 1.0 + 0.25 + 1e-3, (e, ret, steps)
        if not timeout:
            terminated += 1
            assert ret <= steps + 1e-3, (e, ret, steps)
    print("episodes", len(coll._recent_episodes), "terminated", terminated, "worst |return - steps|", worst)
    assert terminated > 0 and worst > 0.0       # the returns are the shaped ones
    # the env's own counters add up the same shaped returns
    assert int(env.ep_count.sum()) == len(coll._recent_episodes)
    want = sum(r for _, r, _, _ in coll._recent_episodes)
    assert abs(float(env.ep_ret_sum.sum()) - want) <= 1e-3 * len(coll._recent_episodes)


def test_unshaped_env_is_unchanged(cuda, monkeypatch):
    """Without wrappers DeviceCartPoleVecEnv still calls gs_cartpole_reset / gs_cartpole_step, has
    no prev_phi, keeps its (N, 4) state, and pays reward 1 on every live row."""
    from gsamd import rollout
    from gsamd.rollout import DeviceCartPoleVecEnv
    called, real = [], rollout.lib

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(rollout, "lib", Spy())
    env = DeviceCartPoleVecEnv(40, seed=3, max_steps=7, device=cuda)
    assert env.wrappers_c is None and env.prev_phi is None and tuple(env.state.shape) == (40, 4)
    env.reset()
    r = torch.zeros(40, device=cuda)
    d = torch.zeros(40, dtype=torch.uint8, device=cuda)
    to = torch.zeros(40, dtype=torch.uint8, device=cuda)
    a = torch.ones(40, dtype=torch.int64, device=cuda)
    for _ in range(9):
        pending = env.meta[:, 2].clone().bool()
        env.step_into(r, d, to, actions=a)
        torch.cuda.synchronize()
        assert torch.equal(r, (~pending).float())
    assert set(called) == {"gs_cartpole_reset", "gs_cartpole_step"}
    # and with the shaper, the shaped entries
    called.clear()
    env = DeviceCartPoleVecEnv(40, seed=3, max_steps=7, wrappers=[{"id": SHAPER_ID}], device=cuda)
    env.reset()
    env.step_into(r, d, to, actions=a)
    torch.cuda.synchronize()
    assert set(called) == {"gs_cartpole_shaped_reset", "gs_cartpole_shaped_step"} and tuple(env.state.shape) == (40, 4)
