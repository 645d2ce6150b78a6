"""The masked-categorical head of the MLP policies on the device (gs_policy_act_masked,
gs_ppo_rows_update_masked / gs_ppo_rows_loss_masked, DeviceMLPActorCritic(valid_actions=...) and
DevicePPOAgent on top) against the float64 twin (tests/masked_mlp_twin.py).

Cases are built as tests/test_gpu_ppo_rows.py builds them (one minibatch: T = 3, N = max(40, ceil(B/3) + 5),
idx = default_rng(B + D).permutation(T N)[:B]; four minibatches: N = ceil(4 B / 3) + 5, idx =
default_rng(seed).permutation(T N)[:4 B]) with the recorded actions drawn from the valid set
(masked_mlp_twin.case), and the bars are that module's: loss 1e-5 relative, metrics 1e-5 relative +
2e-6, clipped gradient 1e-6 of its largest entry, parameters after one Adam step 5e-6, after four steps
1e-5 relative L2.  No bar is widened: the twin sits within 3e-7 of the reference's own float32 step
(tests/test_masked_mlp_cpu.py prints it), far inside every bar.  A case's seed is the first from B + 100
on whose five twin steps all meet the input conditions (both clip fractions strictly inside (0, 1), no
pre-activation within 1e-6 of a ReLU flip, every recorded action valid): first_seed below."""
import functools
import types

import numpy as np
import pytest
import torch

import masked_mlp_twin as TW
import mlp_cases as C
import test_gpu_ppo_rows as RW
from mlp_cases import HP, LR, MAX_NORM

pytestmark = pytest.mark.gpu

# (dims, valid, B, seed)
CASES = [
    ((12, 128, 128, 18), (0, 3, 4), 1043, 1161),       # Pong-objects (mlp_small): AMAX 32, a ragged last tile
    ((12, 64, 18), (0, 3, 4), 1030, 1133),             # one hidden layer (mlp_tiny)
    ((8, 64, 64, 6), (1, 4, 5), 64, 164),              # AMAX 8; action 0 invalid, the last valid; a batch the chain also serves
    ((64, 16, 32, 32), (0, 31), 1025, 1125),           # mask bit 31
    ((8, 64, 64, 6), (2,), 64, 164),                   # one valid action: entropy ~ 0, no policy-logit gradient
    ((8, 64, 64, 6), (0, 1, 2, 3, 4, 5), 64, 164),     # the masked entropy formula with no action excluded
]
_id = lambda s: "%s-valid%s-B%d" % ("-".join(map(str, s[0])), "".join("_%d" % a for a in s[1]), s[2])  # noqa: E731


def _one(dims, valid, B, seed):
    T, N = 3, max(40, -(-B // 3) + 5)
    case = TW.case(dims, valid, T, N, seed)
    idx = np.random.default_rng(B + dims[0]).permutation(T * N)[:B]
    rows = C.rows(idx, T, N)
    zeros = np.zeros_like(case["p0"])
    loss, met, g, gc, total, p1, m1, v1 = TW.step(case, case["p0"], zeros, zeros, rows, 1)
    return dict(case=case, idx=idx, rows=rows, loss=loss, met=met, g=g, gc=gc, total=total, p1=p1,
                ok=TW.conditions_met(case, case["p0"], rows, met))


def _four(dims, valid, B, seed):
    n, T = 4, 3
    N = -(-n * B // T) + 5
    case = TW.case(dims, valid, T, N, seed)
    idx = np.random.default_rng(seed).permutation(T * N)[:n * B]
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    losses, ok = [], True
    for k in range(n):
        rows = C.rows(idx[k * B:(k + 1) * B], T, N)
        loss, met, _, _, _, p1, m, v = TW.step(case, p, m, v, rows, k + 1)
        ok = ok and TW.conditions_met(case, p, rows, met)
        p = p1
        losses.append(loss)
    return dict(case=case, idx=idx, losses=losses, p=p, ok=ok)


def first_seed(dims, valid, B):
    """How CASES' seeds were found (twin only; not run by the tests)."""
    seed = B + 100
    while not (_one(dims, valid, B, seed)["ok"] and _four(dims, valid, B, seed)["ok"]):
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def _ref(shape):
    """One case's twin steps (shared by the tests; never written to)."""
    return _one(*shape), _four(*shape)


class _Run(RW._Run):
    """test_gpu_ppo_rows._Run with the masked entries"""

    def __init__(self, case, cuda, mask):
        super().__init__(case, cuda)
        self.mask = mask

    def loss(self, idx, B, **hp):
        from gsamd._lib import GS_NUM_METRICS, check, lib
        ws, idx_d = self._ws(B), RW._dev(idx, self.cuda, torch.int32)
        rec = torch.full((GS_NUM_METRICS,), -3.0, device=self.cuda)
        g = torch.full((self.P,), -3.0, device=self.cuda)
        check(lib.gs_ppo_rows_loss_masked(self.params.data_ptr(), g.data_ptr(), self.dims, self.hp(**hp), self.view,
                                          idx_d.data_ptr(), B, rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream, self.mask), "gs_ppo_rows_loss_masked")
        torch.cuda.synchronize()
        return rec.cpu().numpy(), g.cpu().numpy()

    def update(self, idx, B, n, step0=0, **hp):
        from gsamd._lib import GS_NUM_METRICS, check, lib
        ws, idx_d = self._ws(B), RW._dev(idx, self.cuda, torch.int32)
        met = torch.full((n, GS_NUM_METRICS), -3.0, device=self.cuda)
        check(lib.gs_ppo_rows_update_masked(self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                            self.v.data_ptr(), self.dims, self.hp(**hp), self.view, idx_d.data_ptr(), B, n,
                                            step0, met.data_ptr(), self.stop.data_ptr(), ws.data_ptr(), ws.numel(), None,
                                            torch.cuda.current_stream().cuda_stream, self.mask),
              "gs_ppo_rows_update_masked")
        torch.cuda.synchronize()
        return met.cpu().numpy()


def _invalid_rows_untouched(run, case, grads=True):
    """The invalid actions' policy-head rows: parameters byte-identical to the start, both Adam moments
    and the gradient exactly 0."""
    inv = TW.invalid_slices(case["dims"], case["valid"])
    p, m, v, g = run.state()
    assert np.array_equal(p[inv].view(np.uint32), case["p0"][inv].view(np.uint32))
    assert not m[inv].any() and not v[inv].any() and not (grads and g[inv].any())
    return inv


# ------------------------------------------------------------------------------- one and four minibatches
@pytest.mark.parametrize("shape", CASES, ids=_id)
def test_one_and_four_minibatches_vs_twin(cuda, shape):
    from gsamd._lib import M
    dims, valid, B, _ = shape
    one, four = _ref(shape)
    assert one["ok"] and four["ok"]                      # the input conditions, from the twin alone
    case, idx, met, g, gc, p1 = one["case"], one["idx"], one["met"], one["g"], one["gc"], one["p1"]
    mask = TW.mask_of(valid)
    run = _Run(case, cuda, mask)
    rec0, g0 = run.loss(idx, B)
    assert np.array_equal(run.params.cpu().numpy(), case["p0"]) and not run.grads.any()
    rec = run.update(idx, B, 1)[0]
    pd, _, _, gd = run.state()
    print("MEASURED %s loss rel %.2e (bar 1e-05) entropy %.3e (twin %.3e) raw grad %.2e (bar %.2e) clipped grad %.2e "
          "(bar %.2e) params %.2e (bar 5e-06) norm rel %.2e (bar 1e-05)"
          % (_id(shape), abs(float(rec0[M["loss"]]) - one["loss"]) / abs(one["loss"]), rec0[M["entropy"]],
             met["opt/policy/entropy"], np.abs(g0 - g).max(), 1e-6 * max(1, np.abs(g).max()), np.abs(gd - gc).max(),
             1e-6 * max(1, np.abs(gc).max()), np.abs(pd - p1).max(), abs(float(rec[M["grad_norm"]]) - one["total"]) / one["total"]))
    for which in (rec0, rec):
        np.testing.assert_allclose(which[M["loss"]], one["loss"], rtol=1e-5, atol=0)
        for key, slot in RW.METRICS + [("roll/adv/norm/std", "adv_norm_std")]:
            np.testing.assert_allclose(which[M[slot]], met[key], atol=2e-6, rtol=1e-5, err_msg=key)
        assert which[M["kl_stop"]] == which[M["skipped"]] == which[M["unevaluated"]] == 0
        np.testing.assert_allclose(which[M["grad_norm"]], one["total"], rtol=1e-5)
        assert which[M["entropy"]] <= np.log(len(valid)) + 1e-6
    assert np.array_equal(rec0.view(np.uint32), rec.view(np.uint32))
    np.testing.assert_allclose(g0, g, atol=1e-6 * max(1, np.abs(g).max()), rtol=0)
    np.testing.assert_allclose(gd, gc, atol=1e-6 * max(1, np.abs(gc).max()), rtol=0)
    np.testing.assert_allclose(pd, p1, atol=5e-6, rtol=0)
    inv = _invalid_rows_untouched(run, case)
    assert not g0[inv].any() and inv.size == (dims[-1] - len(valid)) * (dims[-2] + 1)
    if len(valid) == 1:                                  # nothing moves a lone valid logit either
        from oracle import ppo_ref as R
        G = R.unflatten(g0, dims)
        assert not G["policy_head.weight"].any() and not G["policy_head.bias"].any() and rec0[M["gn_policy_head"]] == 0
        assert abs(rec0[M["entropy"]]) <= 2e-6
    # four minibatches in one call
    case4 = four["case"]
    run4 = _Run(case4, cuda, mask)
    rec4 = run4.update(four["idx"], B, 4)
    p4, pr = run4.state()[0].astype(np.float64), four["p"].astype(np.float64)
    print("MEASURED %s four steps: losses rel %.2e (bar 1e-05) params rel L2 %.2e (bar 1e-05)"
          % (_id(shape), np.abs(rec4[:, 0] / np.asarray(four["losses"]) - 1).max(),
             np.linalg.norm(p4 - pr) / np.linalg.norm(pr)))
    np.testing.assert_allclose(rec4[:, M["loss"]], four["losses"], rtol=1e-5, atol=0)
    assert np.linalg.norm(p4 - pr) / np.linalg.norm(pr) < 1e-5
    assert not rec4[:, [M["kl_stop"], M["skipped"], M["unevaluated"]]].any() and run4.stop.item() == 0
    _invalid_rows_untouched(run4, case4)
    assert not np.array_equal(run4.state()[0], case4["p0"])


# ------------------------------------------------------------------------------- mask 0, determinism
ZERO = [((12, 128, 128, 18), 1043, 1143), ((12, 64, 18), 1043, 1143)]


@pytest.mark.parametrize("shape", ZERO, ids=RW._id)
def test_mask_zero_gives_the_unmasked_entries_bytes(cuda, shape):
    """valid_mask == 0: *_masked against the unmasked entries byte for byte, the update (three
    minibatches, activation statistics on) and the act in its three modes."""
    from gsamd._lib import GS_HP_ACT_STATS, check, lib
    dims, B, seed = shape
    n, T = 3, 3
    N = -(-n * B // T) + 5
    case = C.case(dims, T, N, seed)
    idx = np.random.default_rng(seed).permutation(T * N)[:n * B]
    a, b = RW._Run(case, cuda), _Run(case, cuda, 0)
    rec_a, rec_b = a.update(idx, B, n, flags=GS_HP_ACT_STATS), b.update(idx, B, n, flags=GS_HP_ACT_STATS)
    assert np.isfinite(rec_a).all() and RW._same_bytes(a.state() + [rec_a], b.state() + [rec_b])
    la, lb = RW._Run(case, cuda).loss(idx[:B], B), _Run(case, cuda, 0).loss(idx[:B], B)
    assert RW._same_bytes(la, lb)
    # act
    rows = 1000
    obs = RW._dev(case["obs"][:rows], cuda)
    scratch = torch.zeros(int(lib.gs_policy_scratch_bytes(a.dims, rows)), dtype=torch.uint8, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    outs = {}
    for masked in (False, True):
        for mode in (0, 1, 2):
            act = RW._dev(case["actions"][:rows], cuda, torch.int64)
            lp, val = torch.full((rows,), -3.0, device=cuda), torch.full((rows,), -3.0, device=cuda)
            args = (a.params.data_ptr(), a.dims, obs.data_ptr(), rows, mode, 11, 5, act.data_ptr(), lp.data_ptr(),
                    val.data_ptr(), None, scratch.data_ptr(), None, s)
            check(lib.gs_policy_act_masked(*args, 0) if masked else lib.gs_policy_act(*args), "act")
            torch.cuda.synchronize()
            outs[masked, mode] = [act.cpu().numpy().astype(np.float32), lp.cpu().numpy(), val.cpu().numpy()]
    for mode in (0, 1, 2):
        assert RW._same_bytes(outs[False, mode], outs[True, mode]), mode
    assert len(set(outs[True, 0][0].tolist())) > 3          # unmasked: more than three actions drawn


@pytest.mark.parametrize("shape", [CASES[0], CASES[1]], ids=_id)
def test_two_runs_and_split_calls_give_the_same_bytes(cuda, shape):
    """With a mask: two runs of a three-minibatch update are byte-identical, and one call with
    n_minibatches = 3 equals three calls of 1."""
    from gsamd._lib import GS_HP_ACT_STATS
    dims, valid, B, seed = shape
    n = 3
    four = _ref(shape)[1]
    case, idx, mask = four["case"], four["idx"][:n * B], TW.mask_of(valid)
    a, b, c = _Run(case, cuda, mask), _Run(case, cuda, mask), _Run(case, cuda, mask)
    rec_a = a.update(idx, B, n, flags=GS_HP_ACT_STATS)
    rec_b = b.update(idx, B, n, flags=GS_HP_ACT_STATS)
    rec_c = np.concatenate([c.update(idx[k * B:(k + 1) * B], B, 1, step0=k, flags=GS_HP_ACT_STATS) for k in range(n)])
    assert np.isfinite(rec_a).all() and not np.array_equal(a.state()[0], case["p0"])
    assert RW._same_bytes(a.state() + [rec_a], b.state() + [rec_b])
    assert RW._same_bytes(a.state() + [rec_a], c.state() + [rec_c])


# ------------------------------------------------------------------------------- act
ACT_SEED = 11      # the first rng_seed from 11 on at which at most 8 of the 4096 rows lie within 2e-5 of a CDF boundary


@pytest.mark.parametrize("tag", ["small", "tiny"])
def test_act_on_the_fixture_weights(cuda, tag):
    """gs_policy_act_masked, N = 4096, on the reference fixture's weights: values, mode-1 actions and
    log-probs and mode-2 log-probs against the twin; mode 0 draws valid actions only, equal to the
    twin's inverse CDF at the host-recomputed uniforms outside 2e-5 of a CDF boundary."""
    from gsamd.policy import DeviceMLPActorCritic
    f = TW.fixture(tag)
    dims, valid = f["dims"], f["valid"]
    N, ctr = 4096, 3
    obs = np.random.default_rng(4096).standard_normal((N, dims[0])).astype(np.float32)
    value, ln, amax = TW.act(f["p0"], dims, valid, obs)
    top2 = np.sort(ln[:, list(valid)], axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 1e-5            # no argmax within rounding of a tie (twin alone)
    u = C.uniforms(ACT_SEED, ctr, N)
    want0, dist = TW.sample(ln, valid, u)
    near = dist < 2e-5
    assert near.sum() <= 8
    pm = DeviceMLPActorCritic(dims[0], dims[1:-1], dims[-1], device=cuda, init=False, valid_actions=list(valid))
    pm.load_flat(f["p0"])
    obs_d = RW._dev(obs, cuda)
    a1, lp1, v1 = (t.cpu().numpy() for t in pm.act(obs_d, mode=1))
    assert np.array_equal(a1, amax)
    print("MEASURED %s act: value %.2e logp(mode 1) %.2e (bars 2e-06)"
          % (tag, np.abs(v1 - value).max(), np.abs(lp1 - ln[np.arange(N), amax]).max()))
    np.testing.assert_allclose(v1, value, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(lp1, ln[np.arange(N), amax], rtol=1e-5, atol=2e-6)
    rec = np.asarray(valid)[np.random.default_rng(5).integers(0, len(valid), N)]
    a2, lp2, v2 = (t.cpu().numpy() for t in pm.act(obs_d, mode=2, actions=RW._dev(rec, cuda, torch.int64)))
    assert np.array_equal(a2, rec) and np.array_equal(v2.view(np.uint32), v1.view(np.uint32))
    np.testing.assert_allclose(lp2, ln[np.arange(N), rec], rtol=1e-5, atol=2e-6)
    a0, lp0, _ = (t.cpu().numpy() for t in pm.act(obs_d, mode=0, rng_seed=ACT_SEED, rng_counter=ctr))
    assert np.isin(a0, valid).all()                          # with no exception
    assert np.array_equal(a0[~near], want0[~near])
    np.testing.assert_allclose(lp0, ln[np.arange(N), a0], rtol=1e-5, atol=2e-6)
    assert len(set(a0.tolist())) == len(valid)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- refusals
def test_refusals_with_a_mask(cuda):
    """Mask bits at or beyond n_actions, and the rows entries' own refusals under a mask; no buffer
    changes."""
    from gsamd._lib import GS_HP_BF16, GS_NUM_METRICS, MlpDims, PPOHparams, RolloutView, check, lib
    T, N = 3, 800
    ok, mask = MlpDims(12, 128, 128, 18), 0b11001
    P = int(lib.gs_mlp_param_count(ok))
    rng = np.random.default_rng(3)
    bufs = [RW._dev(rng.standard_normal(P).astype(np.float32), cuda) for _ in range(4)]
    met = torch.full((2, GS_NUM_METRICS), -3.0, device=cuda)
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    f = lambda *shp: torch.ones(*shp, device=cuda)  # noqa: E731
    keep = [f(T, N, 65), torch.zeros(T, N, dtype=torch.int64, device=cuda), f(T, N), f(T, N), f(T, N), f(T, N)]
    view = RolloutView(*(t.data_ptr() for t in keep), T, N)
    need = int(lib.gs_ppo_rows_workspace_bytes(ok, 2048))
    ws = torch.full((need + 64,), 7, dtype=torch.uint8, device=cuda)
    idx = torch.arange(T * N, dtype=torch.int32, device=cuda)
    hp = lambda flags=0, tkl=0.0: PPOHparams(HP["clip"], HP["clip_vf"], HP["vf_coef"], HP["ent_coef"], MAX_NORM, LR,  # noqa: E731
                                             0.9, 0.999, 1e-8, tkl, 1, flags)
    s = torch.cuda.current_stream().cuda_stream
    before = [t.clone() for t in bufs + [met, stop, ws]]
    p, g, m, v = (t.data_ptr() for t in bufs)

    def update(dims=ok, B=2048, hp_=None, wsp=ws.data_ptr(), nbytes=need, comm=None, stop_p=stop.data_ptr(), mask_=mask):
        check(lib.gs_ppo_rows_update_masked(p, g, m, v, dims, hp_ or hp(), view, idx.data_ptr(), B, 1, 0, met.data_ptr(),
                                            stop_p, wsp, nbytes, comm, s, mask_), "gs_ppo_rows_update_masked")

    def loss(dims=ok, B=2048, hp_=None, wsp=ws.data_ptr(), nbytes=need, mask_=mask, **_):
        check(lib.gs_ppo_rows_loss_masked(p, g, dims, hp_ or hp(), view, idx.data_ptr(), B, met.data_ptr(), wsp, nbytes, s,
                                          mask_), "gs_ppo_rows_loss_masked")
    cases = [(dict(mask_=1 << 18), "valid_mask 0x40000 has bits past n_actions 18"),
             (dict(mask_=0x80000001), "has bits past n_actions 18"),
             (dict(dims=MlpDims(12, 40, 128, 18)), "hidden1 40 must be a multiple of 16"),
             (dict(dims=MlpDims(12, 128, 128, 33), mask_=1), r"n_actions 33 outside \[1, 32\]"),
             (dict(B=1), r"batch 1 outside \[2, 2\^20\]"),
             (dict(B=(1 << 20) + 1), r"batch 1048577 outside \[2, 2\^20\]"),
             (dict(hp_=hp(flags=GS_HP_BF16)), "bf16"),
             (dict(nbytes=need - 1), "workspace of %d bytes" % (need - 1)),
             (dict(wsp=ws.data_ptr() + 8), "16-byte aligned")]
    for kw, msg in cases:
        for call in (update, loss):
            with pytest.raises(ValueError, match=msg):
                call(**kw)
    with pytest.raises(ValueError, match="communicator"):
        update(comm=ws.data_ptr())
    with pytest.raises(ValueError, match="target_kl needs the stop flag"):
        update(hp_=hp(tkl=0.01), stop_p=None)
    # the act entry; 32 actions take every bit
    obs = f(64, 12)
    scratch = torch.zeros(int(lib.gs_policy_scratch_bytes(ok, 64)), dtype=torch.uint8, device=cuda)
    act, lp, val = torch.zeros(64, dtype=torch.int64, device=cuda), f(64), f(64)
    for dims, bad in ((ok, 1 << 18), (MlpDims(12, 64, 0, 18), 1 << 31)):
        with pytest.raises(ValueError, match="gs_policy_act_masked: valid_mask 0x[0-9a-f]+ has bits past n_actions 18"):
            check(lib.gs_policy_act_masked(p, dims, obs.data_ptr(), 64, 1, 0, 0, act.data_ptr(), lp.data_ptr(),
                                           val.data_ptr(), None, scratch.data_ptr(), None, s, bad), "gs_policy_act_masked")
    torch.cuda.synchronize()
    for a, b in zip(before + [torch.zeros_like(act), f(64), f(64)], bufs + [met, stop, ws, act, lp, val]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------- agent
# (model_id, seed of the 64-row tensor batch: the first from 164 on whose twin meets the input conditions)
AGENTS = [("mlp_small", 164), ("mlp_tiny", 164)]
SPEC = {"action_space": {"discrete": 18, "valid": [0, 3, 4]},
        "observation_space": {"default": "state", "variants": {"state": {"shape": [12]}}}}


def _agent(cuda, model_id, batch_size, use_graph=True):
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(42)
    cfg = load_config("LunarLander-v3", "ppo", overrides=dict(
        env_dynamics="synthetic", spec=SPEC, model_id=model_id, n_envs=32, n_steps=64, batch_size=batch_size, n_epochs=2,
        ent_coef=0.01))
    return DevicePPOAgent(cfg, device=cuda, use_graph=use_graph)


def agent_case(model_id, seed):
    dims = (12, 128, 128, 18) if model_id == "mlp_small" else (12, 64, 18)
    return TW.case(dims, (0, 3, 4), 1, 64, seed)


@pytest.mark.parametrize("model_id,seed", AGENTS, ids=[a[0] for a in AGENTS])
def test_agent_trains_under_the_mask(cuda, model_id, seed):
    """DevicePPOAgent on a 12-observation / 18-action spec with valid [0, 3, 4]: one epoch at batch_size
    2048 and one at 64 (the rows update at both), every rollout action valid, the step graph's rollout
    equal to the eager one, the epoch's entropy at most ln 3, the invalid head rows unchanged;
    losses_for_batch on a tensor batch against the twin."""
    from gsamd._lib import M
    valid = (0, 3, 4)
    for batch_size in (2048, 64):
        agent, eager = _agent(cuda, model_id, batch_size), _agent(cuda, model_id, batch_size, use_graph=False)
        pm = agent.policy_model
        assert pm.valid_mask == 0b11001 and agent._use_rows(batch_size) and agent.n_minibatches == 2 * 2048 // batch_size
        coll = agent.get_rollout_collector("train")
        assert not coll.one_launch and not coll.one_launch_mlp1
        p0 = pm.params.cpu().numpy().copy()
        agent.train_epoch()
        eager.get_rollout_collector("train").collect()
        torch.cuda.synchronize()
        buf, ebuf = coll.buffer, eager.get_rollout_collector("train").buffer
        acts = buf.actions.cpu().numpy()
        assert np.isin(acts, valid).all() and len(np.unique(acts)) == 3
        for name in ("actions", "logprobs", "values", "obs"):
            assert torch.equal(getattr(buf, name), getattr(ebuf, name)), name
        rec = agent.metrics_buf.cpu().numpy()
        assert np.isfinite(rec).all() and (rec[:, M["grad_norm"]] > 0).all() and not rec[:, M["skipped"]].any()
        assert (rec[:, M["entropy"]] <= np.log(3) + 1e-6).all() and agent.epoch_metrics()["opt/policy/entropy"] <= np.log(3) + 1e-6
        assert agent.adam_step == agent.n_minibatches
        p1 = pm.params.cpu().numpy()
        d = pm.dims
        dims = (d.obs_dim, d.hidden1, d.hidden2, d.n_actions) if d.hidden2 else (d.obs_dim, d.hidden1, d.n_actions)
        inv = TW.invalid_slices(dims, valid)
        assert np.array_equal(p1[inv].view(np.uint32), p0[inv].view(np.uint32)) and not np.array_equal(p1, p0)
        assert not agent.adam_m[torch.as_tensor(inv, device=cuda)].any() and not agent.adam_v[torch.as_tensor(inv, device=cuda)].any()
    # losses_for_batch on a 64-row tensor batch (the agent of batch_size 64)
    case = agent_case(model_id, seed)
    rows = np.arange(64)
    hp = dict(clip=float(agent.clip_range), clip_vf=float(agent.clip_range_vf), vf_coef=float(agent.vf_coef),
              ent_coef=float(agent.ent_coef))
    want, met, _, _, _ = TW.loss_and_grads(case["p0"], dims, valid, case["obs"], case["actions"], case["old_logp"],
                                           case["old_values"], case["adv"], case["ret"], **hp)
    assert TW.conditions_met(case, case["p0"], rows, met)
    pm.load_flat(case["p0"])
    batch = types.SimpleNamespace(observations=torch.as_tensor(case["obs"]), actions=torch.as_tensor(case["actions"]),
                                  logprobs=torch.as_tensor(case["old_logp"]), values=torch.as_tensor(case["old_values"]),
                                  advantages=torch.as_tensor(case["adv"]), returns=torch.as_tensor(case["ret"]))
    out = agent.losses_for_batch(batch, 0)
    got, row = float(out["loss"].item()), agent._step_metrics.cpu().numpy()
    print("MEASURED %s losses_for_batch rel %.2e (bar 1e-05)" % (model_id, abs(got - want) / abs(want)))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    for key, slot in RW.METRICS:
        np.testing.assert_allclose(row[M[slot]], met[key], atol=2e-6, rtol=1e-5, err_msg=key)
    assert np.array_equal(pm.params.cpu().numpy(), case["p0"])      # no optimizer step
    steps = agent.adam_step
    agent.training_step(batch, 0)
    torch.cuda.synchronize()
    after = pm.params.cpu().numpy()
    assert agent.adam_step == steps + 1 and not np.array_equal(after, case["p0"])
    assert np.array_equal(after[inv].view(np.uint32), case["p0"][inv].view(np.uint32))
