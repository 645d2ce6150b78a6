"""The two-hidden-layer actor-critic kernels (csrc/gs_mlp.hip: k_fwd_hidden, k_heads_act, k_loss, k_bwd,
k_clip_adam) against the numpy oracle (oracle.ppo_ref, dims = (D, H1, H2, A)) at the shapes the
ABI promises beyond the two compile-time ones: the runtime instantiations ShapeR<4> / ShapeR<32>
(Acrobot's and MountainCar's shipped shapes among them), the compile-time dims at another batch,
A + 1 > 5 (dh2 tile / slab in LDS), H2 % 64 != 0, an odd count of H1 blocks, H1 != H2, D % 4 != 0,
partial row tiles and slabs, several metric groups per role-C workgroup and the batch bounds.

Bars are those of tests/test_gpu_parity.py and tests/test_gpu_mlp1.py: log-prob / value 1e-5
absolute; loss 1e-5 relative; clipped gradient 1e-6 of its largest entry; parameters after one
Adam step 5e-6; after four steps 1e-5 relative L2 and 1e-3 max-abs.  Every case's input
conditions (both clip ranges straddled, no pre-activation within 1e-6 of a ReLU flip relative to
its terms) are asserted from the oracle alone, so no tolerance hides a flipped unit.  The
(3, 32, 16, 32) row is the one that found the head rows 16.. of a column block unstaged in
k_fwd_hidden and k_bwd's role A.

LDS at the batch bound: (4, 64, 64, 2) at B = 1024 takes 160 448 bytes of dynamic LDS in k_bwd's
role A plus 1 088 static, 161 536 of the CU's 163 840: it runs.  (4, 64, 64, 3) at B = 961..976 is
163 600..163 840 dynamic, over the budget with the static part: refused (test_refusals), and
B = 960, the largest batch of those dims that is accepted, is a row of the matrix."""
import functools

import numpy as np
import pytest
import torch

import mlp_cases as C
from mlp_cases import HP, LR, MAX_NORM

pytestmark = pytest.mark.gpu

# (D, H1, H2, A, B, case seed): a seed is moved on where the first one leaves a pre-activation
# within 1e-6 of zero (B = 520, 1024)
SHAPES = [
    (6, 128, 128, 3, 64, 170),      # Acrobot-v1:ppo; ShapeR<4>, the register-dh2 paths
    (2, 256, 256, 3, 64, 166),      # MountainCar-v0:ppo; D = 2, the smallest obs_dim any config ships
    (4, 256, 256, 2, 64, 168),      # ShapeC<4,256,256,2,0>: CartPole dims, B != 256
    (8, 128, 128, 4, 48, 156),      # ShapeC<8,128,128,4,0>: partial 32-row slab, 64-row pad
    (5, 48, 80, 3, 40, 145),        # ka = 1, regsB false (H2 = 80), H1 != H2, odd D, partial 16-row tile
    (7, 80, 48, 5, 100, 207),       # A + 1 = 6: ShapeR<32>, dh2 tile / slab in LDS; ka = 1; B = 6 * 16 + 4
    (9, 64, 64, 6, 64, 173),        # A + 1 = 7 at an aligned batch
    (3, 32, 16, 32, 17, 120),       # A = kMaxActions, one column block, odd B
    (64, 16, 32, 5, 2, 166),        # D = kMaxObsDim, one k-block, B = 2
    (4, 64, 64, 2, 520, 625),       # 32 metric groups on 5 role-C workgroups; 17 role-B slabs; B = 32 * 16 + 8
    (4, 64, 64, 2, 1024, 1130),     # B = 1024: 161 536 bytes of LDS in role A
    (4, 64, 64, 3, 960, 1064),      # the largest batch of (4, 64, 64, 3) within the LDS budget
]
_id = lambda s: "%d-%d-%d-%d-B%d" % s[:5]  # noqa: E731
NETS = sorted({s[:4] for s in SHAPES})
METRICS = [("opt/loss/policy", "policy_loss"), ("opt/loss/value", "value_loss"), ("opt/policy/entropy", "entropy"),
           ("opt/ppo/clip_fraction", "clip_fraction"), ("opt/ppo/clip_fraction_vf", "clip_fraction_vf"),
           ("opt/value/explained_var", "explained_var"), ("opt/ppo/kl", "kl"), ("opt/ppo/approx_kl", "approx_kl"),
           ("roll/adv/norm/std", "adv_norm_std")]


def _dev(a, cuda, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(cuda).contiguous()


def _model(dims, flat, cuda):
    from gsamd.policy import DeviceMLPActorCritic
    pm = DeviceMLPActorCritic(dims[0], dims[1:3], dims[3], device=cuda, init=False)
    assert pm.n_params == flat.size and pm.dims.hidden2 == dims[2]
    pm.load_flat(flat)
    return pm


def _conditions(case, p, rows, met):
    """The input conditions of one oracle step (float64, no device value involved)."""
    assert 0 < met["opt/ppo/clip_fraction"] < 1 and 0 < met["opt/ppo/clip_fraction_vf"] < 1
    margins = C.preact_margins(p, case["dims"], case["obs"][rows])
    assert min(margins) >= 1e-6, margins
    return margins


@functools.lru_cache(maxsize=None)
def _ref(shape):
    """One shape's case, minibatch rows and oracle step (shared by the tests; never written to)."""
    D, H1, H2, A, B, seed = shape
    T, N = 3, max(40, -(-B // 3) + 5)
    case = C.case((D, H1, H2, A), T, N, seed)
    idx = np.random.default_rng(B + D).permutation(T * N)[:B]
    rows = C.rows(idx, T, N)
    zeros = np.zeros_like(case["p0"])
    loss, met, g, gc, total, p1, _, _ = C.oracle_step(case, case["p0"], zeros, zeros, rows, 1)
    return dict(case=case, idx=idx, rows=rows, loss=loss, met=met, g=g, gc=gc, total=total, p1=p1, B=B)


class _Run:
    """Device buffers of one case and the C-ABI calls on them."""

    def __init__(self, case, cuda):
        from gsamd._lib import MlpDims, RolloutView, lib
        c, T, N = case, case["T"], case["N"]
        D = c["dims"][0]
        self.dims = MlpDims(*c["dims"])
        self.P = int(lib.gs_mlp_param_count(self.dims))
        assert self.P == c["p0"].size
        self.keep = dict(obs=_dev(c["obs"].reshape(T, N, D), cuda), actions=_dev(c["actions"].reshape(T, N), cuda, torch.int64),
                         logprobs=_dev(c["old_logp"].reshape(T, N), cuda), values=_dev(c["old_values"].reshape(T, N), cuda),
                         advantages=_dev(c["adv"].reshape(T, N), cuda), returns=_dev(c["ret"].reshape(T, N), cuda))
        k = self.keep
        self.view = RolloutView(k["obs"].data_ptr(), k["actions"].data_ptr(), k["logprobs"].data_ptr(),
                                k["values"].data_ptr(), k["advantages"].data_ptr(), k["returns"].data_ptr(), T, N)
        self.cuda = cuda
        self.reset(c["p0"])

    def reset(self, p0):
        z = dict(device=self.cuda)
        self.params = _dev(p0, self.cuda)
        self.grads = torch.zeros(self.P, **z)
        self.m = torch.zeros(self.P, **z)
        self.v = torch.zeros(self.P, **z)
        self.stop = torch.zeros(1, dtype=torch.int32, **z)

    def hp(self, lr=LR, target_kl=0.0, flags=0):
        from gsamd._lib import PPOHparams
        return PPOHparams(HP["clip"], HP["clip_vf"], HP["vf_coef"], HP["ent_coef"], MAX_NORM, lr, 0.9, 0.999, 1e-8,
                          target_kl, 1, flags)

    def update(self, idx, B, n, step0=0, use_graph=0, dims=None, ws_bytes=None, **hp):
        from gsamd._lib import GS_NUM_METRICS, check, lib
        dims = dims or self.dims
        nbytes = ws_bytes or int(lib.gs_ppo_update_workspace_bytes(dims, B, n))
        assert nbytes > 0
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.cuda)
        self.met = torch.full((n, GS_NUM_METRICS), -3.0, device=self.cuda)
        idx_d = _dev(idx, self.cuda, torch.int32)
        check(lib.gs_ppo_update(self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                dims, self.hp(**hp), self.view, idx_d.data_ptr(), B, n, step0, self.met.data_ptr(),
                                self.stop.data_ptr(), ws.data_ptr(), ws.numel(), None, use_graph,
                                torch.cuda.current_stream().cuda_stream), "gs_ppo_update")
        torch.cuda.synchronize()
        return self.met.cpu().numpy()

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.params, self.m, self.v, self.grads)]


# ------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_input_conditions(shape):
    """From the oracle alone: both clip ranges are straddled and no layer-1 / layer-2
    pre-activation of the minibatch lies within 1e-6 of zero relative to the sum of its terms'
    magnitudes (a kernel's summation order may not decide a ReLU)."""
    r = _ref(shape)
    margins = _conditions(r["case"], r["case"]["p0"], r["rows"], r["met"])
    print("clip fractions", r["met"]["opt/ppo/clip_fraction"], r["met"]["opt/ppo/clip_fraction_vf"], "margins", margins)


# ------------------------------------------------------------------------------- one minibatch
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_one_minibatch_vs_numpy_oracle(cuda, shape):
    from oracle import ppo_ref as R
    from gsamd._lib import ACT_SLOT, GS_HP_ACT_STATS, GS_NUM_METRICS, M, check, lib
    from gsamd.metrics import activation_stats
    D, H1, H2, A, B, _ = shape
    r = _ref(shape)
    case, idx, rows, met, g, gc, p1 = r["case"], r["idx"], r["rows"], r["met"], r["g"], r["gc"], r["p1"]
    _conditions(case, case["p0"], rows, met)
    run = _Run(case, cuda)
    s = torch.cuda.current_stream().cuda_stream
    ws = torch.zeros(int(lib.gs_ppo_workspace_bytes(run.dims, B)), dtype=torch.uint8, device=cuda)
    idx_d = _dev(idx, cuda, torch.int32)
    rec0 = torch.zeros(GS_NUM_METRICS, device=cuda)
    check(lib.gs_ppo_loss(run.params.data_ptr(), run.dims, run.hp(), run.view, idx_d.data_ptr(), B, rec0.data_ptr(),
                          ws.data_ptr(), s), "gs_ppo_loss")
    rec = torch.zeros(GS_NUM_METRICS, device=cuda)
    check(lib.gs_ppo_minibatch_step(run.params.data_ptr(), run.grads.data_ptr(), run.m.data_ptr(), run.v.data_ptr(),
                                    run.dims, run.hp(flags=GS_HP_ACT_STATS), run.view, idx_d.data_ptr(), B, 1,
                                    rec.data_ptr(), run.stop.data_ptr(), ws.data_ptr(), None, s), "gs_ppo_minibatch_step")
    torch.cuda.synchronize()
    rec0, rec = rec0.cpu().numpy(), rec.cpu().numpy()
    gd, pd = run.grads.cpu().numpy(), run.params.cpu().numpy()
    # the measured distances (the device's and the float32 oracle's from the oracle in float64)
    coef = min(1.0, MAX_NORM / (r["total"] + 1e-6))
    g64 = C.grads_f64(case, rows) * coef
    print("MEASURED %s loss rel %.2e (bar 1e-05) grad %.2e (bar %.2e; device - f64 %.2e, f32 oracle - f64 %.2e) "
          "params %.2e (bar 5e-06) norm rel %.2e (bar 1e-05)"
          % (_id(shape), abs(float(rec[M["loss"]]) - r["loss"]) / abs(r["loss"]), np.abs(gd - gc).max(),
             1e-6 * max(1, np.abs(gc).max()), np.abs(gd - g64).max(), np.abs(gc - g64).max(), np.abs(pd - p1).max(),
             abs(float(rec[M["grad_norm"]]) - r["total"]) / r["total"]))
    np.testing.assert_allclose(rec[M["loss"]], r["loss"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(rec0[:12], rec[:12])                   # gs_ppo_loss: the step's record in slots 0..11
    for key, slot in METRICS:
        np.testing.assert_allclose(rec[M[slot]], met[key], atol=2e-6, rtol=1e-5, err_msg=key)
    assert rec[M["kl_stop"]] == rec[M["skipped"]] == rec[M["unevaluated"]] == 0
    np.testing.assert_allclose(gd, gc, atol=1e-6 * max(1, np.abs(gc).max()), rtol=0)
    np.testing.assert_allclose(pd, p1, atol=5e-6, rtol=0)
    # pre-clip norms: the total and the three components; GS_M_GN_MLP is 0
    G = R.unflatten(g, case["dims"])
    comp = {c: np.sqrt(sum(float((G[k].astype(np.float64) ** 2).sum()) for k in G if k.startswith(c)))
            for c in ("backbone", "policy_head", "value_head")}
    np.testing.assert_allclose(rec[M["grad_norm"]], r["total"], rtol=1e-5)
    for c in comp:
        np.testing.assert_allclose(rec[M[f"gn_{c}"]], comp[c], rtol=2e-5, err_msg=c)
    assert rec[M["gn_mlp"]] == 0
    # GS_HP_ACT_STATS: both layers' slots in the step's record
    want = R.activation_stats(case["p0"], case["dims"], case["obs"][rows])
    got = rec[ACT_SLOT:ACT_SLOT + 8]
    for j in range(8):
        tol = 1.0 / B if j % 4 >= 2 else 1e-5 * (1 + abs(want[j]))
        assert abs(got[j] - want[j]) <= tol, (j, got[j], want[j])
    assert not rec[ACT_SLOT + 8:].any()
    # gs_mlp_activation_stats through gsamd.metrics.activation_stats
    nparts = (B + 15) // 16
    parts = torch.zeros(nparts * 2 * (2 + max(H1, H2)), dtype=torch.float64, device=cuda)
    run.reset(case["p0"])
    check(lib.gs_mlp_activation_stats(run.params.data_ptr(), run.dims, run.view, idx_d.data_ptr(), B, parts.data_ptr(),
                                      s), "gs_mlp_activation_stats")
    torch.cuda.synchronize()
    st = activation_stats(parts.cpu().numpy().reshape(nparts, -1), B, (H1, H2))
    assert set(st) == {f"opt/activations/backbone.{l}/{k}" for l in (0, 2) for k in ("mean", "std", "dead_pct", "dead_max")}
    for i, l in enumerate((0, 2)):
        for j, k in enumerate(("mean", "std", "dead_pct", "dead_max")):
            w = want[4 * i + j]
            tol = 1.0 / B if j >= 2 else 1e-5 * (1 + abs(w))
            assert abs(st[f"opt/activations/backbone.{l}/{k}"] - w) <= tol, (l, k, w)


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("dims", NETS, ids=lambda d: "%d-%d-%d-%d" % d)
def test_forward_vs_numpy_oracle(cuda, dims):
    """gs_policy_act in replay and argmax mode and gs_policy_value at 1, 17 and 300 rows (one
    partial row tile; a full and a partial one; two k_heads_act workgroups)."""
    from oracle import ppo_ref as R
    D, A = dims[0], dims[-1]
    flat = C.flat(dims, seed=7 + sum(dims))
    pm = _model(dims, flat, cuda)
    rng = np.random.default_rng(11 + sum(dims))
    obs = rng.standard_normal((300, D)).astype(np.float32)
    acts = rng.integers(0, A, 300)
    logits, value, _ = R.forward(flat, dims, obs)
    logp = R.log_softmax(logits)[np.arange(300), acts]
    top = np.sort(logits, axis=1)
    sure = (top[:, -1] - top[:, -2]) > 1e-5
    for n in (1, 17, 300):
        obs_d = _dev(obs[:n], cuda)
        a, lp, v = pm.act(obs_d, mode=2, actions=_dev(acts[:n], cuda, torch.int64))
        a_det = pm.act(obs_d, mode=1)[0]
        vv = pm.predict_values(obs_d)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.cpu().numpy(), acts[:n])
        np.testing.assert_allclose(lp.cpu().numpy(), logp[:n], atol=1e-5, rtol=0)
        np.testing.assert_allclose(v.cpu().numpy(), value[:n], atol=1e-5, rtol=0)
        np.testing.assert_allclose(vv.cpu().numpy(), value[:n], atol=1e-5, rtol=0)
        assert (~sure[:n]).sum() <= n // 100
        np.testing.assert_array_equal(a_det.cpu().numpy()[sure[:n]], logits[:n].argmax(axis=1)[sure[:n]])


# ------------------------------------------------------------------------------- sampling, A > 4
@pytest.mark.parametrize("dims", [(9, 64, 64, 6), (3, 32, 16, 32)], ids=lambda d: "%d-%d-%d-%d" % d)
def test_sampling_inverse_cdf_rows_many_actions(cuda, dims):
    """The row-exact check of test_gpu_parity.py::test_policy_sampling_inverse_cdf_rows on
    ShapeR<32>: every row's action is the first a with u < cdf[a] (u the row's counter-based
    uniform, cdf the running sum of the row's probabilities from the replay path's log-probs);
    rows whose u lies within 2e-5 of a boundary are left out, at most 64 of the 4096 (up to 31
    boundaries a row: about 5 expected; the oracle's own count is asserted first)."""
    from oracle import ppo_ref as R
    D, A, n = dims[0], dims[-1], 4096
    flat = C.flat(dims, seed=31 + A)
    obs = np.random.default_rng(32 + A).standard_normal((n, D)).astype(np.float32)
    seed, ctr = 1234, 7
    u = C.uniforms(seed, ctr, n)

    def table(lp):
        cdf = np.cumsum(np.exp(lp.astype(np.float64)), axis=1)
        clear = np.abs(u[:, None] - cdf[:, :A - 1]).min(axis=1) > 2e-5
        return np.minimum((u[:, None] >= cdf).sum(axis=1), A - 1), clear

    want_o, clear_o = table(R.log_softmax(R.forward(flat, dims, obs)[0]))
    assert clear_o.sum() >= n - 64 and len(np.unique(want_o)) == A         # the oracle alone: the inputs fit the cap
    pm = _model(dims, flat, cuda)
    obs_d = _dev(obs, cuda)
    a = pm.act(obs_d, mode=0, rng_seed=seed, rng_counter=ctr)[0].cpu().numpy()
    lp = np.zeros((n, A), np.float32)
    for act in range(A):
        lp[:, act] = pm.act(obs_d, mode=2, actions=torch.full((n,), act, device=cuda, dtype=torch.int64))[1].cpu().numpy()
    want, clear = table(lp)
    assert clear.sum() >= n - 64, clear.sum()
    np.testing.assert_array_equal(a[clear], want[clear])
    both = clear & clear_o
    np.testing.assert_array_equal(a[both], want_o[both])
    assert a.min() >= 0 and a.max() < A and len(np.unique(a)) == A


# ------------------------------------------------------------------------------- four minibatches, one call
@pytest.mark.parametrize("shape", [(6, 128, 128, 3, 64, 300), (7, 80, 48, 5, 100, 301), (4, 64, 64, 2, 520, 302)], ids=_id)
def test_four_minibatches_in_one_update(cuda, shape):
    from gsamd._lib import M
    D, H1, H2, A, B, seed = shape
    n, T = 4, 3
    N = -(-n * B // T) + 5
    case = C.case((D, H1, H2, A), T, N, seed)
    idx = np.random.default_rng(seed).permutation(T * N)[:n * B]          # four disjoint minibatches
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    losses = []
    for k in range(n):
        rows = C.rows(idx[k * B:(k + 1) * B], T, N)
        p_k = p
        loss, met, _, _, _, p, m, v = C.oracle_step(case, p, m, v, rows, k + 1)
        _conditions(case, p_k, rows, met)
        losses.append(loss)
    run = _Run(case, cuda)
    rec = run.update(idx, B, n)
    full = run.state()
    pd, pr = full[0].astype(np.float64), p.astype(np.float64)
    print("MEASURED %s losses rel %.2e (bar 1e-05) params rel L2 %.2e (bar 1e-05) max abs %.2e (bar 1e-03)"
          % (_id(shape), np.abs(rec[:, 0] / np.asarray(losses) - 1).max(), np.linalg.norm(pd - pr) / np.linalg.norm(pr),
             np.abs(pd - pr).max()))
    np.testing.assert_allclose(rec[:, M["loss"]], losses, rtol=1e-5, atol=0)
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5
    assert np.abs(pd - pr).max() < 1e-3
    assert not rec[:, [M["kl_stop"], M["skipped"], M["unevaluated"]]].any()
    assert run.stop.item() == 0
    # a second run, and the captured graph's replay: byte-identical parameters, moments, gradient and records
    for use_graph in (0, 1):
        again = _Run(case, cuda)
        rec2 = again.update(idx, B, n, use_graph=use_graph)
        for x, y in zip(full + [rec], again.state() + [rec2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), use_graph


# ------------------------------------------------------------------------------- KL early stop
def test_kl_early_stop_on_a_runtime_shape(cuda):
    """(9, 64, 64, 6) at B = 64 (ShapeR<32>, dh2 in LDS): the stop flag through k_loss, k_bwd and
    k_clip_adam.  target_kl lies between the oracle's approx_kl of steps 4 and 5, more than 10 %
    away from both (and from every earlier step), so the device stops at step 5."""
    from gsamd._lib import GS_NUM_METRICS, M
    dims, B, n = (9, 64, 64, 6), 64, 8
    T, N, lr, kstar = 16, 32, 3e-3, 5
    case = C.case(dims, T, N, 79, self_logp=True)
    idx = np.random.default_rng(6).permutation(T * N)
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    akl, losses, ps = [], [], []
    for k in range(n):
        ps.append(p)
        rows = C.rows(idx[k * B:(k + 1) * B], T, N)
        loss, met, _, _, _, p, m, v = C.oracle_step(case, p, m, v, rows, k + 1, lr=lr)
        if k <= kstar:
            assert min(C.preact_margins(ps[k], dims, case["obs"][rows])) >= 1e-6
        akl.append(met["opt/ppo/approx_kl"])
        losses.append(loss)
    akl = np.asarray(akl)
    target = float(np.sqrt(akl[kstar - 1] * akl[kstar]))
    print("approx_kl", akl, "target", target)
    assert 1.1 * akl[:kstar].max() <= target <= akl[kstar] / 1.1        # the oracle names step kstar, with margin
    run = _Run(case, cuda)
    rec = run.update(idx, B, n, lr=lr, target_kl=target)
    flags = [M["kl_stop"], M["skipped"], M["unevaluated"]]
    assert not rec[:kstar, flags].any()
    np.testing.assert_allclose(rec[:kstar + 1, M["loss"]], losses[:kstar + 1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rec[:kstar + 1, M["approx_kl"]], akl[:kstar + 1], rtol=1e-4, atol=2e-6)
    assert rec[kstar, M["kl_stop"]] == 1 and rec[kstar, M["skipped"]] == 1 and rec[kstar, M["unevaluated"]] == 0
    later = np.zeros(GS_NUM_METRICS, np.float32)
    later[flags] = 1
    assert kstar + 1 < n and all(np.array_equal(x, later) for x in rec[kstar + 1:])
    assert run.stop.item() == 1
    stopped = run.state()
    # parameters, moments and gradient are those after kstar steps: byte-identical to kstar steps without a target
    plain = _Run(case, cuda)
    plain.update(idx[:kstar * B], B, kstar, lr=lr)
    for x, y in zip(stopped, plain.state()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    pd, pr = stopped[0].astype(np.float64), ps[kstar].astype(np.float64)
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5


# ------------------------------------------------------------------------------- refusals
BIG = (64, 1024, 1024, 4)
REFUSALS = [((6, 40, 128, 3), 64, "hidden1 40 must be a positive multiple of 16"),
            ((65, 128, 128, 3), 64, r"obs_dim 65 outside \[1, 64\]"),
            ((6, 128, 128, 33), 64, r"n_actions 33 outside \[1, 32\]"),
            ((6, 128, 128, 3), 1, r"batch 1 outside \[2, 1024\]"),
            ((6, 128, 128, 3), 1025, r"batch 1025 outside \[2, 1024\]"),
            (BIG, 64, "obs_dim x hidden1 too large for the LDS budget"),
            # 163 840 bytes of dynamic LDS + k_bwd's 1 088 static
            ((4, 64, 64, 3), 976, "batch 976 too large for the LDS budget: 164928 bytes"),
            ((4, 64, 64, 3), 961, "batch 961 too large for the LDS budget: 164688 bytes")]


def test_refusals(cuda):
    """Each call returns its error before anything is launched: parameters, gradient, moments, the
    stop flag and the records keep their bytes.  Every buffer is sized for the largest of the
    refused shapes."""
    from gsamd._lib import GS_NUM_METRICS, MlpDims, PPOHparams, RolloutView, check, lib
    T, N, P = 3, 400, int(lib.gs_mlp_param_count(MlpDims(*BIG)))
    rng = np.random.default_rng(3)
    bufs = [_dev(rng.standard_normal(P).astype(np.float32), cuda) for _ in range(4)]      # params, grads, m, v
    met = torch.full((4, GS_NUM_METRICS), -3.0, device=cuda)
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    f = lambda *shp: torch.ones(*shp, device=cuda)  # noqa: E731
    keep = [f(T, N, 65), torch.zeros(T, N, dtype=torch.int64, device=cuda), f(T, N), f(T, N), f(T, N), f(T, N)]
    view = RolloutView(*(t.data_ptr() for t in keep), T, N)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=cuda)
    idx = torch.arange(T * N, dtype=torch.int32, device=cuda)
    hp = PPOHparams(HP["clip"], HP["clip_vf"], HP["vf_coef"], HP["ent_coef"], MAX_NORM, LR, 0.9, 0.999, 1e-8, 0.0, 1, 0)
    s = torch.cuda.current_stream().cuda_stream
    before = [t.clone() for t in bufs + [met, stop]]
    p, g, m, v = (t.data_ptr() for t in bufs)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    acts = torch.zeros(16, dtype=torch.int64, device=cuda)
    lpv = torch.full((2, 16), -3.0, device=cuda)
    for dims, B, msg in REFUSALS:
        d = MlpDims(*dims)
        with pytest.raises(ValueError, match=msg):
            check(lib.gs_ppo_loss(p, d, hp, view, idx.data_ptr(), B, met.data_ptr(), ws.data_ptr(), s), "gs_ppo_loss")
        with pytest.raises(ValueError, match=msg):
            check(lib.gs_ppo_minibatch_step(p, g, m, v, d, hp, view, idx.data_ptr(), B, 1, met.data_ptr(),
                                            stop.data_ptr(), ws.data_ptr(), None, s), "gs_ppo_minibatch_step")
        for use_graph in (0, 1):
            with pytest.raises(ValueError, match=msg):
                check(lib.gs_ppo_update(p, g, m, v, d, hp, view, idx.data_ptr(), B, 1, 0, met.data_ptr(), stop.data_ptr(),
                                        ws.data_ptr(), ws.numel(), None, use_graph, s), "gs_ppo_update")
        if "batch" not in msg and dims != BIG:       # the dims' own checks guard the rollout-step forward too
            with pytest.raises(ValueError, match=msg):
                check(lib.gs_policy_act(p, d, keep[0].data_ptr(), 16, 1, 0, 0, acts.data_ptr(), lpv[0].data_ptr(),
                                        lpv[1].data_ptr(), None, scratch.data_ptr(), None, s), "gs_policy_act")
            with pytest.raises(ValueError, match=msg):
                check(lib.gs_policy_value(p, d, keep[0].data_ptr(), 16, lpv[1].data_ptr(), scratch.data_ptr(), s),
                      "gs_policy_value")
    torch.cuda.synchronize()
    for a, b in zip(before, bufs + [met, stop]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not acts.any() and (lpv == -3.0).all()
