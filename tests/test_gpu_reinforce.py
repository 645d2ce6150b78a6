"""GPU: device REINFORCE — gs_mc_returns_f32 against the reference's recorded returns and index maps,
gs_pg_loss / gs_pg_update against the reference's loss fixture (and, entry for entry, the torch-CPU
twin, a restatement in the reference's own torch ops that the CPU tests pin to that fixture), the
update's invariants, and
DeviceREINFORCEAgent on Bandit-v0:reinforce and on device CartPole."""
import os

import numpy as np
import pytest
import torch

import reinforce_twin as tw
from test_reinforce_cpu import GAMMAS, RETURN_SHAPES, _pool, check_against_fixture, ill_conditioned

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "reinforce.npz"))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _mc(cuda, rew, dones, timeouts, gamma, kind, with_map=True):
    from gsamd._lib import check, lib, ptr, stream_handle
    T, N = rew.shape
    r, d = _dev(rew, cuda), _dev(dones, cuda)
    to = None if timeouts is None else _dev(timeouts, cuda)
    ret = torch.full((T, N), float("nan"), device=cuda)
    im = torch.full((N * T,), -7, dtype=torch.int32, device=cuda) if with_map else None
    lt = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=cuda)
    check(lib.gs_mc_returns_f32(ptr(r), ptr(d), ptr(to), T, N, float(gamma), kind, ptr(ret), ptr(im), ptr(lt), ptr(sums),
                                stream_handle()), "gs_mc_returns_f32")
    torch.cuda.synchronize()
    return ret.cpu().numpy(), (im.cpu().numpy() if with_map else None), lt.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("T,N", RETURN_SHAPES)
def test_mc_returns_match_the_reference(cuda, gold, T, N):
    """Returns bit-exact, idx_map / last_terminal exact, the valid sums within the float32
    pairwise-sum bound 1e-6 sum|x| of the reference's own sums (2^-24 ceil(log2 n) sum|x|, n <= 2^16)."""
    tag = f"ret/{T}x{N}"
    rew, dones, mask = gold[f"{tag}/rewards"], gold[f"{tag}/dones"], gold[f"{tag}/timeouts"]
    for to_name, to in (("default", None), ("mask", mask)):
        valid = gold[f"{tag}/{to_name}/valid"]
        for g in GAMMAS:
            for kind, name in ((0, "rtg"), (1, "episode")):
                want = gold[f"{tag}/{to_name}/g{g}/{name}"]
                ret, im, lt, sums = _mc(cuda, rew, dones, to, g, kind)
                assert np.array_equal(ret, want), (to_name, g, name)
                assert np.array_equal(im, gold[f"{tag}/{to_name}/idx_map"])
                assert np.array_equal(lt, gold[f"{tag}/{to_name}/last_terminal"])
                v = want.T.reshape(-1)[valid]
                assert sums[0] == v.size
                ref_sum, ref_sq = float(v.sum(dtype=np.float32)), float((v * v).sum(dtype=np.float32))
                assert abs(sums[1] - ref_sum) <= 1e-6 * float(np.abs(v).sum(dtype=np.float64)) + 0.0
                assert abs(sums[2] - ref_sq) <= 1e-6 * float((v.astype(np.float64) ** 2).sum())
    # the map is optional
    ret, im, lt, _ = _mc(cuda, rew, dones, None, 0.99, 0, with_map=False)
    assert im is None and np.array_equal(ret, gold[f"{tag}/default/g0.99/rtg"])


def test_mc_returns_with_nothing_valid(cuda, gold):
    rew = gold["ret/64x37/rewards"]
    ret, im, lt, sums = _mc(cuda, rew, np.zeros_like(gold["ret/64x37/dones"]), None, 0.98, 1)
    assert np.array_equal(im, np.arange(64 * 37)) and (lt == -1).all() and not sums.any()
    assert np.array_equal(ret, np.broadcast_to(tw.mc_returns(rew, np.zeros((64, 37), bool), None, 0.98)[0], (64, 37)))
    # more envs than one scan chunk of 256, one terminal each side of the chunk boundary
    T, N = 3, 600
    d = np.zeros((T, N), np.uint8)
    d[1, 5] = d[2, 300] = d[0, 599] = 1
    r = np.random.default_rng(3).normal(size=(T, N)).astype(np.float32)
    ret, im, lt, sums = _mc(cuda, r, d, None, 0.99, 0)
    last, want_map, valid = tw.valid_index_map(d, None)
    assert np.array_equal(ret, tw.mc_returns(r, d, None, 0.99)) and np.array_equal(im, want_map) and np.array_equal(lt, last)
    assert sums[0] == valid.sum() == 6


# ---- loss, gradient, steps -----------------------------------------------------------------------
class _Case:
    """One loss case on the device: the pool as the rollout, three minibatches perms[k][:B]."""

    def __init__(self, cuda, gold, case):
        from gsamd._lib import GS_NUM_METRICS, MlpDims, PGHparams, RolloutView, lib, ptr
        self.tag, shape, self.B, self.norm, self.ent = case
        self.dims = tw.LOSS_SHAPES[shape]
        self.pool = _pool(gold, tw.POOLS[shape])
        self.P = tw.n_params(*self.dims)
        self.flat = tw.hash_params(self.P)
        self.t = {k: _dev(self.pool[k], cuda) for k in ("obs", "actions", "logprobs", "returns")}
        self.idx = _dev(np.concatenate([self.pool["perms"][k][:self.B] for k in range(3)]).astype(np.int32), cuda)
        self.md = MlpDims(*self.dims)
        self.hp = PGHparams(self.ent, 0.5, 1e-3, 0.9, 0.999, 1e-8, 1 if self.norm else 0, 0)
        self.view = RolloutView(ptr(self.t["obs"]), ptr(self.t["actions"]), ptr(self.t["logprobs"]), None,
                                ptr(self.t["returns"]), None, tw.POOL_T, tw.POOL_N)
        self.wsb = int(lib.gs_pg_update_workspace_bytes(self.md, self.B))
        self.ws = torch.zeros(self.wsb, dtype=torch.uint8, device=cuda)
        self.cuda, self.nm = cuda, GS_NUM_METRICS

    def state(self, m0=0.0, v0=0.0):
        z = dict(dtype=torch.float32, device=self.cuda)
        return (_dev(self.flat, self.cuda), torch.zeros(self.P, **z), torch.full((self.P,), m0, **z),
                torch.full((self.P,), v0, **z))

    def loss(self, params, grads):
        from gsamd._lib import check, lib, ptr, stream_handle
        met = torch.full((self.nm,), float("nan"), device=self.cuda)
        check(lib.gs_pg_loss(ptr(params), ptr(grads), self.md, self.hp, self.view, ptr(self.idx), self.B, ptr(met),
                             ptr(self.ws), self.wsb, stream_handle()), "gs_pg_loss")
        torch.cuda.synchronize()
        return met.cpu().numpy()

    def update(self, st, n, step0=0, first=0):
        from gsamd._lib import check, lib, ptr, stream_handle
        p, g, m, v = st
        met = torch.full((n, self.nm), float("nan"), device=self.cuda)
        check(lib.gs_pg_update(ptr(p), ptr(g), ptr(m), ptr(v), self.md, self.hp, self.view,
                               ptr(self.idx[first * self.B:]), self.B, n, step0, ptr(met), ptr(self.ws), self.wsb, None,
                               stream_handle()), "gs_pg_update")
        torch.cuda.synchronize()
        return met.cpu().numpy()


def _record(row):
    from gsamd._lib import M
    rec = dict(loss=row[M["loss"]], policy_loss=row[M["policy_loss"]], entropy=row[M["entropy"]], kl=row[M["kl"]],
               approx_kl=row[M["approx_kl"]], target_mean=row[M["pg_target_mean"]], target_std=row[M["pg_target_std"]],
               grad_norm=row[M["grad_norm"]], gn_backbone=row[M["gn_backbone"]], gn_policy_head=row[M["gn_policy_head"]])
    return {k: float(v) for k, v in rec.items()}


@pytest.mark.parametrize("case", tw.loss_cases(), ids=lambda c: c[0])
def test_loss_gradient_and_steps_match_the_reference(cuda, gold, case):
    """gs_pg_loss's record, norms and gradient and gs_pg_update's parameters after three steps at
    the project's tolerances (check_against_fixture) against the reference's fixture; the whole
    gradient, not only the fixture's sampled entries, against the torch-CPU twin at the same
    tolerance; and the invariants: the value head's parameters and both moments untouched (moments
    starting non-zero), its gradient zero, every slot the entry does not serve zero.


    The parameters after three steps are held to 5e-6 at every sampled entry.  One entry
    (small1010_B2_norm_ent0, flat 6181) is held to the double evaluation of the same inputs instead of
    the fixture, at the same 5e-6: its reference gradient is the size of Adam's eps and the fixture
    itself is 7.08e-6 from the double value (test_reinforce_cpu.ill_conditioned finds it on the CPU,
    from the fixture alone)."""
    from gsamd._lib import M
    c = _Case(cuda, gold, case)
    p, g, m, v = c.state(m0=0.01, v0=0.02)
    row = c.loss(p, g)
    rec = _record(row)
    if c.norm:
        rec["norm_mean"], rec["norm_std"] = float(row[M["adv_norm_mean"]]), float(row[M["adv_norm_std"]])
    else:
        assert row[M["adv_norm_mean"]] == 0 and row[M["adv_norm_std"]] == 0
    served = {M[k] for k in ("loss", "policy_loss", "entropy", "kl", "approx_kl", "adv_norm_mean", "adv_norm_std",
                             "grad_norm", "gn_backbone", "gn_policy_head", "pg_target_mean", "pg_target_std")}
    assert np.isfinite(row).all() and not row[[j for j in range(c.nm) if j not in served]].any()
    gd = g.cpu().numpy()
    assert np.array_equal(p.cpu().numpy(), c.flat)                      # the loss entry takes no step
    _, g_twin = tw.loss_and_grads(c.flat, c.dims, *tw.batch_rows(c.pool, c.pool["perms"][0], c.B), c.ent, c.norm)
    np.testing.assert_allclose(gd, g_twin, rtol=0, atol=2e-6 * max(1.0, float(np.abs(g_twin).max())))
    nv = c.dims[2] + 1
    assert not gd[-nv:].any()
    # three steps from zero moments (the fixture's), then the value-head invariant from non-zero ones
    st = c.state()
    recs = c.update(st, 3)
    check_against_fixture(gold, c.tag, rec, gd, st[0].cpu().numpy(), ill=ill_conditioned(gold, case))
    np.testing.assert_array_equal(recs[0][:c.nm], row)                  # the update's first record is the loss entry's
    for t, start in ((st, 0.0), ((p, g, m, v), None)):
        if start is None:
            c.update(t, 3)
        assert np.array_equal(t[0].cpu().numpy()[-nv:], c.flat[-nv:])
    assert torch.equal(m[-nv:], torch.full((nv,), 0.01, device=cuda)) and torch.equal(v[-nv:], torch.full((nv,), 0.02, device=cuda))
    assert not torch.equal(m[:-nv], torch.full((c.P - nv,), 0.01, device=cuda))
    assert not st[2][-nv:].any() and not st[3][-nv:].any() and st[2][:-nv].any()


@pytest.mark.parametrize("case", [c for c in tw.loss_cases() if c[0] in (
    "small1010_B48_norm_ent0.01", "small42_B2048_raw_ent0", "medium42_B2048_norm_ent0.01")], ids=lambda c: c[0])
def test_update_is_deterministic_and_splits_over_calls(cuda, gold, case):
    """Two runs of the same update give the same bytes; n_minibatches = 3 in one call equals three
    calls of 1 (parameters, moments, gradient, records)."""
    c = _Case(cuda, gold, case)
    a, b, s = c.state(), c.state(), c.state()
    ra, rb = c.update(a, 3), c.update(b, 3)
    rs = np.concatenate([c.update(s, 1, step0=k, first=k) for k in range(3)])
    for x, y, z in zip(a, b, s):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert ra.tobytes() == rb.tobytes() == rs.tobytes()


def test_update_loops_over_more_tiles_than_workgroups(cuda):
    """B = 16 x 300 + 5 rows: 301 tiles on 256 workgroups (some own two tiles, the last tile is ragged),
    against the twin at the gradient tolerance."""
    from gsamd._lib import GS_NUM_METRICS, M, MlpDims, PGHparams, RolloutView, check, lib, ptr, stream_handle
    dims, T, N = (6, 32, 48, 3), 61, 80
    B = 16 * 300 + 5
    rng = np.random.default_rng(11)
    P = tw.n_params(*dims)
    flat = tw.hash_params(P, salt=5)
    pool = dict(obs=rng.normal(size=(T, N, 6)).astype(np.float32), actions=rng.integers(0, 3, size=(T, N)).astype(np.int64),
                logprobs=(-1.1 + 0.1 * rng.normal(size=(T, N))).astype(np.float32),
                returns=rng.normal(size=(T, N)).astype(np.float32) * 2 + 1)
    perm = rng.permutation(T * N).astype(np.int32)
    rec, g_twin = tw.loss_and_grads(flat, dims, *tw.batch_rows(pool, perm, B), 0.01, True)
    t = {k: _dev(v, cuda) for k, v in pool.items()}
    md, hp = MlpDims(*dims), PGHparams(0.01, 0.5, 1e-3, 0.9, 0.999, 1e-8, 1, 0)
    view = RolloutView(ptr(t["obs"]), ptr(t["actions"]), ptr(t["logprobs"]), None, ptr(t["returns"]), None, T, N)
    wsb = int(lib.gs_pg_update_workspace_bytes(md, B))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=cuda)
    p, g, idx = _dev(flat, cuda), torch.zeros(P, device=cuda), _dev(perm, cuda)
    met = torch.zeros(GS_NUM_METRICS, device=cuda)
    check(lib.gs_pg_loss(ptr(p), ptr(g), md, hp, view, ptr(idx), B, ptr(met), ptr(ws), wsb, stream_handle()), "gs_pg_loss")
    torch.cuda.synchronize()
    row = met.cpu().numpy()
    np.testing.assert_allclose(row[M["loss"]], rec["loss"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(row[M["grad_norm"]], rec["grad_norm"], rtol=2e-5)
    np.testing.assert_allclose(g.cpu().numpy(), g_twin, rtol=0, atol=2e-6 * max(1.0, float(np.abs(g_twin).max())))


# ---- the agent -----------------------------------------------------------------------------------
def test_agent_learns_the_bandit_through_the_public_entry(cuda, tmp_path):
    """build_agent(load_config("Bandit-v0", "reinforce")), no env=: the 9 rollouts of its 20 000-step
    budget.  Finite records, adam_step 9, the 0.04 -> 0 schedule, the one-launch bandit rollout.  With
    zero observations the only live gradient is -p_a (mu_a - mu_bar) on the head biases: the three
    best arms' biases end positive, the three worst negative, and the mean reward of the last
    rollout's pulls (the rows that pulled an arm: every other row is the autoreset row, reward 0)
    exceeds the first's by more than 0.2 — both checked through the twin first
    (test_reinforce_cpu.test_twin_learns_the_bandit: rises of 0.36 .. 0.57).  Then a checkpoint
    round trip: the value head's moments are written as zeros."""
    from gsamd import build_agent
    from gsamd.config import load_config
    from gsamd.reinforce_agent import DeviceREINFORCEAgent
    from gsamd.rollout import DeviceBanditVecEnv
    from gsamd.schedules import build_schedulers
    torch.manual_seed(42)
    cfg = load_config("Bandit-v0", "reinforce")
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    assert isinstance(agent, DeviceREINFORCEAgent) and isinstance(agent.get_env("train"), DeviceBanditVecEnv)
    assert coll.one_launch is True and agent.n_minibatches == 1 and coll.returns_type == "mc:rtg"
    (sched,) = build_schedulers(cfg.schedules, cfg.max_env_steps, cfg.n_envs)
    pulls, logged = [], []
    v0 = agent.policy_model.state_dict()["value_head.weight"].clone()

    def log(m):
        b = coll.buffer
        pulls.append(float(b.rewards[b.dones.bool()].mean()))
        logged.append(m)
    agent.learn(log=log)
    torch.cuda.synchronize()
    assert agent.adam_step == 9 == agent.current_epoch == len(logged) and coll.total_steps == 9 * 2048
    for k, m in enumerate(logged):
        assert all(np.isfinite(v) for v in m.values() if isinstance(v, float)), m
        assert m["hp/policy_lr"] == pytest.approx(sched.value(64 * k), rel=1e-6)
        assert m["opt/loss/entropy"] == pytest.approx(-m["opt/policy/entropy"])
        assert m["opt/grads/norm/value_head"] == 0.0 and m["opt/grads/norm/all"] > 0
        assert "roll/baseline/mean" in m and "policy_targets_std" in m and "opt/ppo/approx_kl" in m
    assert logged[0]["hp/policy_lr"] == pytest.approx(0.04) and agent.policy_lr == pytest.approx(sched.value(64 * 9))
    sd = agent.policy_model.state_dict()
    bias = sd["policy_head.bias"].cpu().numpy()
    assert (bias[7:10] > 0).all() and (bias[0:3] < 0).all(), bias
    assert pulls[-1] - pulls[0] > 0.2, pulls
    assert torch.equal(sd["value_head.weight"], v0)
    # the index map: the rollout ends on an autoreset row, which maps to the pull before it
    im = coll.idx_map.cpu().numpy().reshape(32, 64)
    assert (im[:, :63] == np.arange(32)[:, None] * 64 + np.arange(63)).all() and (im[:, 63] == im[:, 62]).all()
    # checkpoint round trip
    agent.save_checkpoint(tmp_path)
    opt = torch.load(tmp_path / "optimizer.pt", weights_only=True)[0]["state"]
    assert not opt[6]["exp_avg"].any() and not opt[7]["exp_avg_sq"].any() and opt[5]["exp_avg"].any()
    other = build_agent(cfg, device=cuda)
    other.load_checkpoint(tmp_path)
    assert torch.equal(other.policy_model.params, agent.policy_model.params)
    assert torch.equal(other.adam_m, agent.adam_m) and torch.equal(other.adam_v, agent.adam_v)
    assert other.adam_step == 9 and other.current_epoch == 9
    assert other.get_rollout_collector("train")._base_stats == coll._base_stats and coll._base_stats["count"] == 9 * 32 * 63
    assert other.policy_lr == pytest.approx(agent.policy_lr)


def test_episode_returns_and_baseline_on_device_cartpole(cuda):
    """mc:episode returns with policy_targets "advantages" on device CartPole (8 envs x 64 steps, four
    128-row minibatches per rollout): the collector's targets equal the twin's on the device's own
    rewards and dones (returns bit-exact, the running baseline, advantages = returns - f32(baseline)),
    the update's index stream is the sampler's mapped through the idx_map, and
    slice_trajectories applies the same map."""
    from gsamd import build_agent
    from gsamd.config import REINFORCEConfig
    torch.manual_seed(7)
    spec = {"action_space": {"discrete": 2}, "observation_space": {"default": "state", "variants": {"state": {"shape": [4]}}}}
    cfg = REINFORCEConfig(env_id="CartPole-v1", project_id="CartPole-v1", n_envs=8, n_steps=64, batch_size=128,
                          model_id="mlp_small", returns_type="mc:episode", policy_targets="advantages", policy_lr=1e-3,
                          gamma=0.98, spec=spec, max_env_steps=None)
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    assert agent.n_minibatches == 4 and agent.targets_field == "advantages" and not agent.normalize_targets
    base = tw.BaseStats()
    for k in range(3):
        agent.train_epoch()
        torch.cuda.synchronize()
        b = coll.buffer
        adv, ret, idx_map, last = tw.targets(b.rewards.cpu().numpy(), b.dones.cpu().numpy(), None, 0.98, "mc:episode", base)
        assert (last >= 0).any() and (last < 63).any()          # CartPole episodes end inside the rollout
        assert np.array_equal(b.returns.cpu().numpy(), ret)
        assert coll._base_stats["count"] == base.count
        assert coll.baseline_mean() == pytest.approx(base.mean(), rel=1e-12)
        assert np.array_equal(b.advantages.cpu().numpy(), (ret - np.float32(coll.baseline_mean())).astype(np.float32))
        assert np.array_equal(coll.idx_map.cpu().numpy(), idx_map)
        fed = agent._mapped(agent.prefetcher.device_buf).cpu().numpy()
        assert np.array_equal(fed, idx_map[agent.prefetcher.device_buf.cpu().numpy()])
        valid = np.arange(64)[None, :] <= last[:, None]
        assert valid.reshape(-1)[fed].all() and not valid.all()
        m = {**coll.get_metrics(), **agent.epoch_metrics()}
        assert m["roll/baseline/mean"] == pytest.approx(base.mean()) and m["roll/baseline/std"] == pytest.approx(base.std())
        assert np.isfinite(agent.minibatch_losses()).all() and agent.adam_step == 4 * (k + 1)
    sl = coll.slice_trajectories(agent._trajectories, [0, 63, 64 * 7 + 63])
    want = torch.as_tensor(idx_map[[0, 63, 64 * 7 + 63]].astype(np.int64), device=cuda)
    assert torch.equal(sl.returns, agent._trajectories.returns[want])
    # losses_for_batch on a tensor batch: the reference's return shape, no step
    before = agent.policy_model.params.clone()
    out = agent.losses_for_batch(coll.slice_trajectories(agent._trajectories, np.arange(96)), 0)
    assert out["early_stop_epoch"] is False and np.isfinite(float(out["loss"]))
    assert torch.equal(agent.policy_model.params, before)


def test_rollout_normalisations_on_the_mc_path(cuda):
    """normalize_returns and normalize_advantages "rollout" with mc:rtg targets on device CartPole:
    the collector's returns and advantages are the twin's _normalize_returns / _normalize_advantages
    of the raw targets (values of a few units in float32: 1e-6 covers the last-place differences of
    the mean and std), and the statistics taken after them cover every position of the rollout."""
    from gsamd import build_agent
    from gsamd.config import REINFORCEConfig
    torch.manual_seed(3)
    spec = {"action_space": {"discrete": 2}, "observation_space": {"default": "state", "variants": {"state": {"shape": [4]}}}}
    cfg = REINFORCEConfig(env_id="CartPole-v1", project_id="CartPole-v1", n_envs=8, n_steps=64, batch_size=512,
                          model_id="mlp_small", normalize_returns="rollout", normalize_advantages="rollout",
                          policy_targets="advantages", policy_lr=1e-3, gamma=0.98, spec=spec, max_env_steps=None)
    agent = build_agent(cfg, device=cuda)
    coll = agent.get_rollout_collector("train")
    assert coll.normalize_returns and coll.normalize_advantages and not agent.normalize_targets
    sums = np.zeros(3)
    for k in range(2):
        agent.train_epoch()
        torch.cuda.synchronize()
        b = coll.buffer
        raw = tw.mc_returns(b.rewards.cpu().numpy(), b.dones.cpu().numpy(), None, 0.98)
        adv = (raw - np.float32(coll.baseline_mean())).astype(np.float32)
        ret = b.returns.cpu().numpy()
        np.testing.assert_allclose(ret, tw.normalize_rollout(raw), rtol=0, atol=1e-6)
        np.testing.assert_allclose(b.advantages.cpu().numpy(), tw.normalize_rollout(adv), rtol=0, atol=1e-6)
        assert abs(float(ret.mean())) < 1e-6 and float(ret.std()) == pytest.approx(1.0, abs=1e-5)
        sums += [ret.size, ret.astype(np.float64).sum(), (ret.astype(np.float64) ** 2).sum()]
        m = coll.get_metrics()
        # roll/return/* are taken after the rollout normalisation, over all 512 positions (valid or not)
        assert m["roll/return/mean"] == pytest.approx(sums[1] / sums[0], abs=1e-6)
        assert m["roll/return/std"] == pytest.approx(np.sqrt(sums[2] / sums[0] - (sums[1] / sums[0]) ** 2), abs=1e-6)
        assert m["roll/adv_norm/std"] == pytest.approx(1.0, abs=1e-4)
        assert np.isfinite(agent.minibatch_losses()).all()
