"""GPU: device Bandit-v0 — the step kernel against the numpy twin (tests/bandit_twin.py), the
one-launch rollout against the per-step loop, the one-launch probe and its bound on the arm count,
and training / evaluation of the resolved Bandit-v0:ppo (with its scheduled policy_lr) through the
public entry."""
import ctypes

import numpy as np
import pytest
import torch

import bandit_twin as B

pytestmark = pytest.mark.gpu

YAML = dict(n_arms=10, means=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], stds=1, episode_length=1)


def _spec(n):
    return {"action_space": {"discrete": n},
            "observation_space": {"default": "z", "variants": {"z": {"shape": ["n_arms"]}}}}


@pytest.mark.parametrize("kw,max_steps", [(YAML, None), (dict(n_arms=3, stds=[0, 0.5, 2], episode_length=3), 2)],
                         ids=["yaml10", "timeout3"])
def test_step_kernel_matches_twin(cuda, kw, max_steps):
    """gs_bandit_step against the twin over 12 steps of random actions on 40 envs.  Flags, meta,
    episode counts and lengths and the all-zero observations are exact.  Every reward is within one
    float32 spacing of the twin's: the device's double log / sqrt / cos may differ from numpy's by
    a few double ulps, which moves the float32 rounding by at most one step, near ties only.  The
    running returns and their sums are exact float32 sums of the device's own rewards.  An arm of
    std 0 pays exactly float32(mean).  With max_steps == episode_length the done is a termination
    (timeout 0); with max_episode_steps 2 < episode_length 3 it is a timeout."""
    from gsamd.rollout import DeviceBanditVecEnv
    N, STEPS, SEED, OFF = 40, 12, 9, 6
    env = DeviceBanditVecEnv(N, seed=SEED, env_offset=OFF, max_steps=max_steps, device=cuda, **kw)
    tw = B.BanditTwin(N, seed=SEED, env_offset=OFF, max_steps=max_steps, **kw)
    env.obs.fill_(5.0)
    env.meta.fill_(3)
    env.reset()
    tw.reset()
    assert not env.obs.cpu().numpy().any() and not env.meta.cpu().numpy().any()
    assert env.max_steps == tw.max_steps == (max_steps or kw["episode_length"])
    rng = np.random.default_rng(1)
    r = torch.zeros(N, device=cuda)
    d = torch.zeros(N, dtype=torch.uint8, device=cuda)
    to = torch.zeros(N, dtype=torch.uint8, device=cuda)
    er, ers = np.zeros(N, np.float32), np.zeros(N, np.float32)
    differ, rows, dones, timeouts, zero_std = 0, 0, 0, 0, 0
    for t in range(STEPS):
        a = rng.integers(0, kw["n_arms"], N)
        pending = tw.meta[:, 2].astype(bool)
        want_r, want_d, want_t = tw.step(a)
        env.obs.fill_(5.0)                                   # the step rewrites the zeros
        env.step_into(r, d, to, actions=torch.as_tensor(a).to(cuda))
        torch.cuda.synchronize()
        rr, dd, tt = r.cpu().numpy(), d.cpu().numpy(), to.cpu().numpy()
        assert not env.obs.cpu().numpy().any()
        assert np.array_equal(dd, want_d) and np.array_equal(tt, want_t), t
        assert np.array_equal(env.meta.cpu().numpy(), tw.meta), t
        assert np.all(rr[pending] == 0.0) and np.all(dd[pending] == 0)
        assert np.all(np.abs(rr.astype(np.float64) - want_r.astype(np.float64)) <= np.spacing(np.abs(want_r))), t
        differ += int((rr != want_r).sum())
        rows += int((~pending).sum())
        live0 = ~pending & (tw.stds[np.clip(a, 0, kw["n_arms"] - 1)] == 0)
        assert np.array_equal(rr[live0], tw.means[a[live0]])
        zero_std += int(live0.sum())
        er = np.where(pending, np.float32(0), (er + rr).astype(np.float32))
        ers = np.where(dd.astype(bool), (ers + er).astype(np.float32), ers)
        assert np.array_equal(env.ep_ret.cpu().numpy(), er), t
        dones += int(dd.sum())
        timeouts += int(tt.sum())
    print("rewards differing from the twin at all:", differ, "of", rows, "live rows")
    assert np.array_equal(env.ep_count.cpu().numpy(), tw.ep_count)
    assert np.array_equal(env.ep_len_sum.cpu().numpy(), tw.ep_len_sum)
    assert np.array_equal(env.ep_ret_sum.cpu().numpy(), ers)
    assert dones > 0 and rows > 0
    if max_steps is None:
        assert timeouts == 0 and dones == N * STEPS // 2         # every live step ends its one-step episode
    else:
        assert timeouts == dones and zero_std > 0                 # the time limit of 2 comes before the 3rd step


def test_entries_refuse_a_spec_that_could_leave_the_arrays(cuda):
    from gsamd.rollout import DeviceBanditVecEnv
    env = DeviceBanditVecEnv(16, device=cuda, **YAML)
    env.reset()
    r = torch.zeros(16, device=cuda)
    d = torch.zeros(16, dtype=torch.uint8, device=cuda)
    a = torch.zeros(16, dtype=torch.int64, device=cuda)
    for field, bad in (("n_arms", 33), ("n_arms", 1), ("episode_length", 0)):
        good = getattr(env.spec, field)
        setattr(env.spec, field, bad)
        with pytest.raises(ValueError, match="gs_bandit_step"):
            env.step_into(r, d, d.clone(), actions=a)
        setattr(env.spec, field, good)
    # an action outside [0, n_arms) is clamped, not read past the arrays
    a[:8], a[8:] = -4, 99
    env.step_into(r, d, d.clone(), actions=a)
    torch.cuda.synchronize()
    rr = r.cpu().numpy()
    z = np.array([B.normal(env.seed, e, 0, 0) for e in range(16)])
    want = np.where(np.arange(16) < 8, 0.0 + z, 9.0 + z).astype(np.float32)
    assert np.all(np.abs(rr.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))


_ONE = dict(n_envs=40, n_steps=64, n_epochs=2)


def test_one_launch_rollout_equals_step_loop(cuda):
    """gs_rollout_bandit (the whole rollout in one launch, on its own 10-action
    shape) writes bit for bit the rows of the per-step loop (gs_policy_act on its 32-action shape +
    gs_bandit_step): sampled, deterministic and replayed actions, over rollouts separated by
    updates, a ragged last workgroup (40 % 16 != 0), and leaves the same meta, running returns,
    observations and episode counters.  The initial policy is near-uniform over 1 280 pulls: fewer
    than 8 of the 10 arms in the first rollout would mean the head's upper actions are broken."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    runs = []
    for one in (False, True):
        torch.manual_seed(42)
        cfg = load_config("Bandit-v0", "ppo", overrides=dict(_ONE))
        agent = DevicePPOAgent(cfg, device=cuda, use_graph=False, track_stats=True, one_launch=one)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch == one
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
        rec.append([t.clone() for t in (e.meta, e.ep_ret, e.obs, e.ep_count, e.ep_ret_sum, e.ep_len_sum)])
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
    assert not first[0].any()                                   # the observations are zeros
    assert int(first[5].sum()) == 40 * 32 and int(first[6].sum()) == 0
    pulled = torch.unique(first[1][~_reset_rows(first[5])])
    assert pulled.numel() >= 8 and int(pulled.max()) <= 9, pulled.tolist()
    assert torch.equal(torch.unique(r1[4][0]).cpu(), torch.arange(10))       # the replayed actions reach every arm


def _reset_rows(dones):
    """(T, N) bool: the rows after a done, whose action is ignored."""
    out = torch.zeros_like(dones, dtype=torch.bool)
    out[1:] = dones[:-1].bool()
    return out


def _supported(dims):
    from gsamd._lib import GS_ENV_BANDIT, MlpDims, check, lib
    v = ctypes.c_int(-1)
    check(lib.gs_rollout_env_supported(MlpDims(*dims), GS_ENV_BANDIT, ctypes.byref(v)), "gs_rollout_env_supported")
    return v.value


def test_one_launch_probe_and_the_arm_bound(cuda):
    """gs_rollout_env_supported(kind GS_ENV_BANDIT): the reference's 10 arms under mlp_small take
    one launch; mlp_medium does not fit in LDS; more than GS_BANDIT_ROLLOUT_MAX_ARMS arms, or an
    obs dim that is not the arm count, do not — and such a config (12 arms) still trains, on the
    step loop and its captured graph."""
    from gsamd import build_agent
    from gsamd._lib import GS_BANDIT_ROLLOUT_MAX_ARMS
    from gsamd.config import load_config
    assert GS_BANDIT_ROLLOUT_MAX_ARMS == 10
    assert _supported((10, 128, 128, 10)) == 1 and _supported((2, 128, 128, 2)) == 1
    assert _supported((10, 256, 256, 10)) == 0
    assert _supported((11, 128, 128, 11)) == 0 and _supported((16, 128, 128, 16)) == 0
    assert _supported((32, 128, 128, 32)) == 0
    assert _supported((10, 128, 128, 4)) == 0 and _supported((4, 128, 128, 2)) == 0
    torch.manual_seed(42)
    cfg = load_config("Bandit-v0", "ppo", overrides=dict(n_envs=16, n_steps=32, n_epochs=2, spec=_spec(12),
                                                         env_kwargs=dict(n_arms=12, stds=0.5)))
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    assert coll.one_launch is False and coll.env.n_arms == 12 and agent.policy_model.n_actions == 12
    for _ in range(3):          # eager warm-up, then the captured step graph
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all()
    assert not coll.buffer.obs.any() and coll._graphs.get(0) is not None
    acts = coll.buffer.actions
    assert int(acts.min()) >= 0 and int(acts.max()) == 11
    assert build_agent(load_config("Bandit-v0", "ppo", overrides=dict(model_id="mlp_medium")), device=cuda) \
        .get_rollout_collector("train").one_launch is False


def test_agent_trains_on_the_resolved_config_through_the_public_entry(cuda):
    """build_agent on Bandit-v0:ppo as resolved, no env=: four epochs with finite losses; each
    epoch's hp/policy_lr is the linear 0.04 -> 0 schedule (gsamd.schedules, pinned by
    schedules.npz) at the vector steps taken before that epoch; every episode is one pull (its
    recorded length counts the autoreset row of every episode after an env's first, as
    test_gpu_mountaincar._episodes); evaluate_episodes returns the usual keys.  No learning outcome
    is asserted."""
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.rollout import DeviceBanditVecEnv
    from gsamd.schedules import build_schedulers
    torch.manual_seed(42)
    cfg = load_config("Bandit-v0", "ppo")
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    assert isinstance(agent.get_env("train"), DeviceBanditVecEnv) and coll.one_launch is True
    (sched,) = build_schedulers(cfg.schedules, cfg.max_env_steps, cfg.n_envs)
    assert (sched.parameter, sched.start_step, sched.end_step) == ("policy_lr", 0.0, 20000 / 32)
    lrs = []
    for k in range(4):
        before = coll.total_vec_steps
        agent.train_epoch()
        m = agent.epoch_metrics()
        assert before == 64 * k and coll.total_vec_steps == 64 * (k + 1)
        assert m["hp/policy_lr"] == pytest.approx(sched.value(before), rel=1e-6)
        assert agent.policy_lr == pytest.approx(sched.value(coll.total_vec_steps), rel=1e-12)
        lrs.append(m["hp/policy_lr"])
    torch.cuda.synchronize()
    assert lrs[0] == pytest.approx(0.04) and all(a > b > 0 for a, b in zip(lrs, lrs[1:]))
    assert np.isfinite(agent.minibatch_losses()).all()
    met = coll.get_metrics()
    assert met["cnt/total_episodes"] == len(coll._recent_episodes) == 4 * 32 * 32
    seen = set()
    for e, ret, length, timeout in coll._recent_episodes:
        assert length - (1 if e in seen else 0) == 1 and not timeout and np.isfinite(ret)
        seen.add(e)
    out = agent.get_rollout_collector("val").evaluate_episodes(n_episodes=8, deterministic=True)
    assert out["cnt/total_episodes"] == 8
    assert {"roll/ep_rew/mean", "roll/ep_len/mean", "cnt/total_env_steps", "cnt/total_vec_steps"} <= set(out)
    assert out["roll/ep_len/mean"] == 1 and np.isfinite(out["roll/ep_rew/mean"])
