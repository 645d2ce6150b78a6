"""The one-launch rollout of the one-hidden-layer policy (csrc/gs_mlp1.hip k_rollout1, the
gs_rollout1_* entries, DeviceRolloutCollector(one_launch_mlp1=True)) against the step loop it
replaces — bit for bit, on every device env — against the tabular twin, across workgroups and
env_offset, and the entries' argument contract."""
import ctypes

import numpy as np
import pytest
import torch

import tabular_twin as TW

pytestmark = pytest.mark.gpu

SH = {"id": "MountainCarV0_RewardShaper", "position_reward_scale": 100.0, "velocity_reward_scale": 10.0,
      "height_reward_scale": 50.0}
BO = {"id": "MountainCarV0_StateCountBonus", "position_bins": 12, "velocity_bins": 9, "bonus_scale": 0.1,
      "bonus_type": "count"}
ENC = lambda e: [{"id": "DiscreteEncoder", "encoding": e}]      # noqa: E731
TINY = dict(model_id="mlp_tiny")
# n_envs 70 is no multiple of a workgroup's 64 envs; max_episode_steps 10 (the bandit: episode_length 4)
# ends and autoresets every env several times within the 40 steps
SHAPE = dict(n_envs=70, n_steps=40, batch_size=100, n_epochs=2, max_episode_steps=10)
CASES = {
    "frozenlake-4x4-array": ("FrozenLake-v1", "ppo", dict(SHAPE), (1, 4)),
    "frozenlake-8x8-onehot": ("FrozenLake-v1", "ppo", dict(SHAPE, env_kwargs={"is_slippery": True, "map_name": "8x8"},
                                                         env_wrappers=ENC("onehot")), (64, 4)),
    "taxi-binary": ("Taxi-v3", "ppo", dict(SHAPE, env_wrappers=ENC("binary")), (9, 6)),
    "cartpole": ("CartPole-v1", "ppo", dict(SHAPE, **TINY), (4, 2)),
    "cartpole-shaped": ("CartPole-v1", "ppo_rewardshaped", dict(SHAPE, **TINY), (4, 2)),
    "acrobot": ("Acrobot-v1", "ppo", dict(SHAPE, **TINY), (6, 3)),
    "mountaincar-both": ("MountainCar-v0", "ppo", dict(SHAPE, env_wrappers=[SH, BO], **TINY), (2, 3)),
    "bandit-10": ("Bandit-v0", "ppo", dict({k: v for k, v in SHAPE.items() if k != "max_episode_steps"},
                                           env_kwargs={"n_arms": 10, "means": list(range(10)), "stds": 1,
                                                       "episode_length": 4}, **TINY), (10, 10)),
}
BUFFER_FIELDS = ("obs", "actions", "logprobs", "values", "rewards", "dones", "timeouts", "advantages", "returns")
ENV_FIELDS = ("state", "meta", "ep_ret", "obs", "ep_count", "ep_ret_sum", "ep_len_sum", "counts", "prev_phi")


def _buffer(coll):
    return {f: getattr(coll.buffer, f).clone() for f in BUFFER_FIELDS}


def _env_tensors(env):
    return {f: getattr(env, f).clone() for f in ENV_FIELDS if isinstance(getattr(env, f, None), torch.Tensor)}


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("case", list(CASES))
def test_one_launch_rollout_equals_the_step_loop(cuda, case):
    """Two agents from one seed, the eager step loop and one_launch_mlp1=True: after three training
    epochs and two deterministic rollouts every buffer tensor, the env's own tensors, the
    parameters, the step count and the episode metrics are equal bit for bit."""
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    env_id, variant, over, (D, A) = CASES[case]
    runs = []
    for kw in (dict(one_launch_mlp1=False, use_graph=False), dict(one_launch_mlp1=True)):
        torch.manual_seed(42)
        agent = DevicePPOAgent(load_config(env_id, variant, overrides=over), device=cuda, **kw)
        coll = agent.get_rollout_collector("train")
        assert coll.one_launch_mlp1 == kw["one_launch_mlp1"] and not coll.one_launch
        pm = agent.policy_model
        assert pm.dims.hidden2 == 0 and (pm.dims.obs_dim, pm.dims.n_actions) == (D, A)
        rec = []
        for _ in range(3):
            agent.train_epoch()
            rec.append(_buffer(coll))
        for _ in range(2):
            coll.collect(deterministic=True)
            rec.append(_buffer(coll))
        torch.cuda.synchronize()
        m = coll.get_metrics()
        runs.append((rec, _env_tensors(coll.env), pm.params.clone(), coll.total_vec_steps,
                     m["cnt/total_episodes"], m.get("roll/ep_rew/mean")))
        del agent
    (r0, e0, p0, n0, ep0, rew0), (r1, e1, p1, n1, ep1, rew1) = runs
    for k, (a, b) in enumerate(zip(r0, r1)):
        _assert_same(a, b, f"rollout {k}")
    assert {"meta", "ep_ret", "obs", "ep_count"} <= set(e0)
    _assert_same(e0, e1, "env")
    assert torch.equal(p0, p1) and n0 == n1 == 5 * 40
    # every env finished several episodes inside one rollout: dones in the last training rollout
    assert int(r0[2]["dones"].sum(0).min()) >= 2 and int(r0[2]["timeouts"].sum()) >= (0 if "bandit" in case else 1)
    assert ep0 == ep1 > 0 and rew0 == rew1 and rew0 is not None


def _tabular(cuda, N, T, off=0, seed=5, max_steps=7, kind="frozenlake", encoding="array", one_launch_mlp1=True, pm=None):
    from gsamd.policy import DeviceMLPActorCritic
    from gsamd.rollout import DeviceRolloutCollector, DeviceTabularVecEnv
    env = DeviceTabularVecEnv(N, kind=kind, encoding=encoding, seed=seed, env_offset=off, max_steps=max_steps, device=cuda)
    if pm is None:
        torch.manual_seed(3)
        pm = DeviceMLPActorCritic(env.obs_dim, (64,), env.n_actions, device=cuda)
    coll = DeviceRolloutCollector(env, pm, T, use_graph=False, one_launch_mlp1=one_launch_mlp1)
    assert coll.one_launch_mlp1 == one_launch_mlp1 and not coll.one_launch
    return env, pm, coll


def test_replay_mode_equals_the_step_loop_and_the_twin(cuda):
    """collect(replay_actions=A) through the one-launch path equals the step path on the same A,
    and its reward / done / timeout / observation rows are the twin's teacher-forced with A
    (N = 37, env_offset 3, max_steps 7, two rollouts so the second starts mid-episode)."""
    from gsamd import toytext
    N, T, off, seed, max_steps = 37, 30, 3, 5, 7
    rng = np.random.default_rng(11)
    env1, pm, c1 = _tabular(cuda, N, T, off, seed, max_steps)
    env0, _, c0 = _tabular(cuda, N, T, off, seed, max_steps, one_launch_mlp1=False, pm=pm)
    twin = TW.TabularTwin(toytext.tables_for("frozenlake", "4x4", True), N, "array", seed=seed, env_offset=off,
                          max_steps=max_steps)
    obs = twin.reset()
    for _ in range(2):
        A = rng.integers(0, 4, (T, N))
        A_dev = torch.as_tensor(A, dtype=torch.int64, device=cuda)
        c1.collect(replay_actions=A_dev)
        c0.collect(replay_actions=A_dev)
        _assert_same(_buffer(c1), _buffer(c0), "replay")
        _assert_same(_env_tensors(env1), _env_tensors(env0), "env")
        assert torch.equal(c1.buffer.actions, A_dev)
        b = {f: getattr(c1.buffer, f).cpu().numpy() for f in ("obs", "rewards", "dones", "timeouts")}
        for t in range(T):
            assert np.array_equal(b["obs"][t], obs), t
            r_t, d_t, to_t = twin.step(A[t])
            obs = twin.obs()
            assert np.array_equal(b["rewards"][t], r_t) and np.array_equal(b["dones"][t], d_t), t
            assert np.array_equal(b["timeouts"][t], to_t), t
        assert np.array_equal(env1.state.cpu().numpy(), twin.state) and np.array_equal(env1.meta.cpu().numpy(), twin.meta)
        assert np.array_equal(env1.obs.cpu().numpy(), obs)
        assert np.array_equal(env1.ep_count.cpu().numpy(), twin.ep_count)
        assert np.array_equal(env1.ep_ret_sum.cpu().numpy(), twin.ep_ret_sum)
    assert twin.ep_count.min() >= 2


def test_many_workgroups_and_env_offset(cuda):
    """300 envs (five workgroups, the last ragged) equal the step loop in sampling mode; two
    collectors of 150 envs at env_offset 0 and 150 reproduce the halves of the 300-env rollout's
    rows on the same replayed actions (the sampling draw is keyed by the local row, the env by the
    global one)."""
    N, T = 300, 8
    env1, pm, c1 = _tabular(cuda, N, T, max_steps=3)
    env0, _, c0 = _tabular(cuda, N, T, max_steps=3, one_launch_mlp1=False, pm=pm)
    for _ in range(2):
        c1.collect()
        c0.collect()
        _assert_same(_buffer(c1), _buffer(c0), "sampled")
        _assert_same(_env_tensors(env1), _env_tensors(env0), "env")
    assert len(set(c1.buffer.actions.reshape(-1).tolist())) == 4
    A = torch.as_tensor(np.random.default_rng(4).integers(0, 4, (T, N)), dtype=torch.int64, device=cuda)
    envw, _, cw = _tabular(cuda, N, T, max_steps=3, pm=pm)
    cw.collect(replay_actions=A)
    whole, whole_env = _buffer(cw), _env_tensors(envw)
    for off in (0, 150):
        envh, _, ch = _tabular(cuda, 150, T, off=off, max_steps=3, pm=pm)
        ch.collect(replay_actions=A[:, off:off + 150].contiguous())
        for f, x in _buffer(ch).items():
            assert torch.equal(x, whole[f][:, off:off + 150]), (off, f)
        for f, x in _env_tensors(envh).items():
            assert torch.equal(x, whole_env[f][off:off + 150]), (off, f)
    assert int(whole["dones"].sum()) > N


def _supported(dims):
    from gsamd._lib import MlpDims, check, lib
    v = ctypes.c_int(7)
    check(lib.gs_rollout1_supported(MlpDims(*dims), ctypes.byref(v)), "gs_rollout1_supported")
    return v.value


def test_supported_query_follows_the_lds_rule(cuda):
    """gs_rollout1_supported: 1 for the preset shape, an error for two hidden layers, and for every
    shape of the one-hidden-layer envelope the answer is (4 (round4(P) + 64 (D | 1)) <= 160 KiB),
    the bytes computed here.  The envelope is swept (D, A at their ends, every hidden1 up to 1040):
    the update's own LDS rule (four parameter-sized vectors) keeps P below 6.5 k parameters, so the
    largest accepted shape needs about 42 KiB and no shape of the envelope reaches the 0 answer —
    it is asserted as that equivalence.  gs_rollout_env_supported still answers 0 for one layer."""
    from gsamd._lib import GS_ENV_CARTPOLE, MlpDims, check, lib
    assert _supported((1, 64, 0, 4)) == 1
    with pytest.raises(ValueError, match="one hidden layer"):
        _supported((4, 256, 256, 2))
    accepted, worst = 0, 0
    for D in (1, 4, 64):
        for A in (1, 4, 32):
            for H in range(16, 1041, 16):
                try:
                    got = _supported((D, H, 0, A))
                except ValueError:
                    continue
                P = int(lib.gs_mlp_param_count(MlpDims(D, H, 0, A)))
                nbytes = 4 * (((P + 3) & ~3) + 64 * (D | 1))
                assert got == (1 if nbytes <= 160 * 1024 else 0), (D, H, A, nbytes)
                accepted, worst = accepted + 1, max(worst, nbytes)
    print("accepted shapes", accepted, "largest rollout LDS", worst)
    assert accepted >= 9 and _supported((64, 64, 0, 32)) == 1 and 4 * (6308 + 64 * 65) <= worst <= 160 * 1024
    v = ctypes.c_int(7)
    check(lib.gs_rollout_env_supported(MlpDims(4, 64, 0, 2), GS_ENV_CARTPOLE, ctypes.byref(v)), "gs_rollout_env_supported")
    assert v.value == 0


def test_tabular_entry_refuses_bad_arguments_before_any_launch(cuda):
    """gs_rollout1_tabular with two-layer dims, a null row pointer, mode 3 or an oversized spec is
    a ValueError that leaves the buffers and the env untouched; T = 0 is OK and writes nothing;
    the unchanged call then runs."""
    from gsamd._lib import MlpDims, TabularSpec, check, lib, ptr, stream_handle
    env, pm, coll = _tabular(cuda, 20, 6)
    buf = coll.buffer           # resets the env
    for f in BUFFER_FIELDS:
        getattr(buf, f).fill_(7)
    before = (_buffer(coll), _env_tensors(env))

    def call(dims=None, T=buf.T, mode=0, spec=None, rows=None):
        rows = rows if rows is not None else [ptr(buf.obs), ptr(buf.actions), ptr(buf.logprobs), ptr(buf.values),
                                             ptr(buf.rewards), ptr(buf.dones), ptr(buf.timeouts)]
        check(lib.gs_rollout1_tabular(ptr(pm.params), dims or pm.dims, env.num_envs, T, mode, 1, 0, ptr(env.state),
                                      ptr(env.meta), ptr(env.ep_ret), ptr(env.obs), spec or env.spec,
                                      ptr(env.next_table), ptr(env.reward_table), ptr(env.term_table), ptr(env.starts),
                                      env.max_steps, env.seed, env.env_offset, ptr(env.ep_count), ptr(env.ep_ret_sum),
                                      ptr(env.ep_len_sum), *rows, stream_handle()), "gs_rollout1_tabular")

    def untouched():
        torch.cuda.synchronize()
        _assert_same(_buffer(coll), before[0], "buffer")
        _assert_same(_env_tensors(env), before[1], "env")

    with pytest.raises(ValueError, match="one hidden layer"):
        call(dims=MlpDims(1, 64, 64, 4))
    rows = [ptr(buf.obs), ptr(buf.actions), ptr(buf.logprobs), None, ptr(buf.rewards), ptr(buf.dones), ptr(buf.timeouts)]
    with pytest.raises(ValueError, match="null buffer"):
        call(rows=rows)
    with pytest.raises(ValueError, match="mode 3"):
        call(mode=3)
    with pytest.raises(ValueError, match="tables too large"):
        call(spec=TabularSpec(1 << 20, 64, 64, 1, 0, 1))
    with pytest.raises(ValueError, match="not the env's"):
        call(dims=MlpDims(1, 64, 0, 6))
    untouched()
    call(T=0)
    untouched()
    call()
    torch.cuda.synchronize()
    assert not torch.equal(buf.values, before[0]["values"]) and int(buf.actions.max()) <= 3
