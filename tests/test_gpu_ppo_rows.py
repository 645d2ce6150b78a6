"""The row-parallel PPO update (csrc/gs_ppo_rows.hip: gs_ppo_rows_loss / gs_ppo_rows_update) against
the numpy oracle (oracle.ppo_ref) on one- and two-hidden-layer nets at minibatches beyond the chain's
1024 rows, and DevicePPOAgent on top of it.

Cases are built as tests/test_gpu_mlp2_shapes.py::_ref builds them (T = 3, N = max(40, ceil(B/3) + 5),
idx = default_rng(B + D).permutation(T N)[:B]) and the bars are that module's: loss 1e-5 relative,
metrics 1e-5 relative + 2e-6, clipped gradient 1e-6 of its largest entry, parameters after one Adam
step 5e-6, after four steps 1e-5 relative L2 and 1e-3 max-abs.  Every case first asserts its input
conditions from the oracle alone (both clip fractions strictly inside (0, 1), no pre-activation
within 1e-6 of a ReLU flip relative to its terms)."""
import functools
import types

import numpy as np
import pytest
import torch

import mlp_cases as C
from mlp_cases import HP, LR, MAX_NORM

pytestmark = pytest.mark.gpu

# (dims, B, case seed): the first seed from B + 100 on that meets the input conditions
SHAPES = [
    ((4, 256, 256, 2), 2048, 2181),     # mlp_medium at the reference's large batch; W2 does not fit LDS
    ((12, 128, 128, 18), 1043, 1143),   # Pong-objects dims: A + 1 = 19 > 16, ragged last tile, just past the chain's bound
    ((12, 64, 18), 2048, 2148),         # one hidden layer (mlp_tiny)
    ((5, 48, 80, 3), 1100, 1200),       # H1 != H2, H2 % 64 != 0, odd D
    ((64, 16, 32, 32), 1025, 1125),     # D and A at their bounds, one MFMA column block
    ((8, 512, 512, 4), 1056, 1182),     # the envelope's widest net: the LDS check's edge
    ((4, 16, 16, 2), 4115, 4215),       # 258 row tiles on 256 row workgroups (two of them loop), the last tile ragged
    ((4, 64, 64, 2), 64, 164),          # a batch the chain also serves
]
_id = lambda s: "%s-B%d" % ("-".join(map(str, s[0])), s[1])  # noqa: E731
METRICS = [("opt/loss/policy", "policy_loss"), ("opt/loss/value", "value_loss"), ("opt/policy/entropy", "entropy"),
           ("opt/ppo/clip_fraction", "clip_fraction"), ("opt/ppo/clip_fraction_vf", "clip_fraction_vf"),
           ("opt/value/explained_var", "explained_var"), ("opt/ppo/kl", "kl"), ("opt/ppo/approx_kl", "approx_kl")]


def _dev(a, cuda, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(cuda).contiguous()


def _mlp_dims(dims):
    from gsamd._lib import MlpDims
    return MlpDims(dims[0], dims[1], dims[2] if len(dims) == 4 else 0, dims[-1])


def _conditions(case, p, rows, met):
    """The input conditions of one oracle step (float64, no device value involved)."""
    assert 0 < met["opt/ppo/clip_fraction"] < 1 and 0 < met["opt/ppo/clip_fraction_vf"] < 1
    margins = C.preact_margins(p, case["dims"], case["obs"][rows])
    assert min(margins) >= 1e-6, margins
    return margins


def _oracle_step(case, p, m, v, rows, t, lr=LR, normalize=True):
    """mlp_cases.oracle_step, with the advantage normalisation as an option"""
    if normalize:
        return C.oracle_step(case, p, m, v, rows, t, lr=lr)
    from oracle import ppo_ref as R
    c = case
    loss, met, g = R.ppo_loss_and_grads(p, c["dims"], c["obs"][rows], c["actions"][rows], c["old_logp"][rows],
                                        c["old_values"][rows], c["adv"][rows], c["ret"][rows], normalize=None, **HP)
    gc, total = R.clip_grad_norm(g, c["dims"], MAX_NORM)
    p1, m1, v1 = R.adam_step(p, gc, m, v, t, lr)
    return loss, met, g, gc, total, p1, m1, v1


@functools.lru_cache(maxsize=None)
def _ref(shape, normalize=True):
    """One shape's case, minibatch rows and oracle step (shared by the tests; never written to)."""
    dims, B, seed = shape
    T, N = 3, max(40, -(-B // 3) + 5)
    case = C.case(dims, T, N, seed)
    idx = np.random.default_rng(B + dims[0]).permutation(T * N)[:B]
    rows = C.rows(idx, T, N)
    zeros = np.zeros_like(case["p0"])
    loss, met, g, gc, total, p1, _, _ = _oracle_step(case, case["p0"], zeros, zeros, rows, 1, normalize=normalize)
    return dict(case=case, idx=idx, rows=rows, loss=loss, met=met, g=g, gc=gc, total=total, p1=p1, B=B)


class _Run:
    """Device buffers of one case and the C-ABI calls on them."""

    def __init__(self, case, cuda, p0=None):
        from gsamd._lib import RolloutView, lib
        c, T, N = case, case["T"], case["N"]
        D = c["dims"][0]
        self.dims = _mlp_dims(c["dims"])
        self.P = int(lib.gs_mlp_param_count(self.dims))
        assert self.P == c["p0"].size
        self.keep = dict(obs=_dev(c["obs"].reshape(T, N, D), cuda), actions=_dev(c["actions"].reshape(T, N), cuda, torch.int64),
                         logprobs=_dev(c["old_logp"].reshape(T, N), cuda), values=_dev(c["old_values"].reshape(T, N), cuda),
                         advantages=_dev(c["adv"].reshape(T, N), cuda), returns=_dev(c["ret"].reshape(T, N), cuda))
        k = self.keep
        self.view = RolloutView(k["obs"].data_ptr(), k["actions"].data_ptr(), k["logprobs"].data_ptr(),
                                k["values"].data_ptr(), k["advantages"].data_ptr(), k["returns"].data_ptr(), T, N)
        self.cuda = cuda
        z = dict(device=cuda)
        self.params = _dev(c["p0"] if p0 is None else p0, cuda)
        self.grads = torch.zeros(self.P, **z)
        self.m = torch.zeros(self.P, **z)
        self.v = torch.zeros(self.P, **z)
        self.stop = torch.zeros(1, dtype=torch.int32, **z)

    def hp(self, lr=LR, target_kl=0.0, flags=0, normalize=True):
        from gsamd._lib import PPOHparams
        return PPOHparams(HP["clip"], HP["clip_vf"], HP["vf_coef"], HP["ent_coef"], MAX_NORM, lr, 0.9, 0.999, 1e-8,
                          target_kl, 1 if normalize else 0, flags)

    def _ws(self, B):
        from gsamd._lib import lib
        nbytes = int(lib.gs_ppo_rows_workspace_bytes(self.dims, B))
        assert nbytes > 0
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.cuda)

    def loss(self, idx, B, **hp):
        """gs_ppo_rows_loss -> (record, unclipped gradient)"""
        from gsamd._lib import GS_NUM_METRICS, check, lib
        ws, idx_d = self._ws(B), _dev(idx, self.cuda, torch.int32)
        rec = torch.full((GS_NUM_METRICS,), -3.0, device=self.cuda)
        g = torch.full((self.P,), -3.0, device=self.cuda)
        check(lib.gs_ppo_rows_loss(self.params.data_ptr(), g.data_ptr(), self.dims, self.hp(**hp), self.view,
                                   idx_d.data_ptr(), B, rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream), "gs_ppo_rows_loss")
        torch.cuda.synchronize()
        return rec.cpu().numpy(), g.cpu().numpy()

    def update(self, idx, B, n, step0=0, **hp):
        from gsamd._lib import GS_NUM_METRICS, check, lib
        ws, idx_d = self._ws(B), _dev(idx, self.cuda, torch.int32)
        met = torch.full((n, GS_NUM_METRICS), -3.0, device=self.cuda)
        check(lib.gs_ppo_rows_update(self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                     self.dims, self.hp(**hp), self.view, idx_d.data_ptr(), B, n, step0, met.data_ptr(),
                                     self.stop.data_ptr(), ws.data_ptr(), ws.numel(), None,
                                     torch.cuda.current_stream().cuda_stream), "gs_ppo_rows_update")
        torch.cuda.synchronize()
        return met.cpu().numpy()

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.params, self.m, self.v, self.grads)]


def _same_bytes(xs, ys):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(xs, ys))


# ------------------------------------------------------------------------------- one minibatch
@pytest.mark.parametrize("shape,normalize", [(s, True) for s in SHAPES] + [(SHAPES[3], False)],
                         ids=[_id(s) for s in SHAPES] + [_id(SHAPES[3]) + "-raw-adv"])
def test_one_minibatch_vs_numpy_oracle(cuda, shape, normalize):
    """The record and the unclipped gradient from gs_ppo_rows_loss; the norms, the clipped gradient and
    the parameters from gs_ppo_rows_update with n = 1."""
    from oracle import ppo_ref as R
    from gsamd._lib import M
    dims, B, _ = shape
    r = _ref(shape, normalize)
    case, idx, rows, met, g, gc, p1 = r["case"], r["idx"], r["rows"], r["met"], r["g"], r["gc"], r["p1"]
    _conditions(case, case["p0"], rows, met)
    run = _Run(case, cuda)
    rec0, g0 = run.loss(idx, B, normalize=normalize)
    assert np.array_equal(run.params.cpu().numpy(), case["p0"]) and not run.grads.any()
    rec = run.update(idx, B, 1, normalize=normalize)[0]
    pd, _, _, gd = run.state()
    coef = min(1.0, MAX_NORM / (r["total"] + 1e-6))
    g64 = C.grads_f64(case, rows) if normalize else None
    print("MEASURED %s loss rel %.2e (bar 1e-05) raw grad %.2e (bar %.2e) clipped grad %.2e (bar %.2e%s) "
          "params %.2e (bar 5e-06) norm rel %.2e (bar 1e-05)"
          % (_id(shape), abs(float(rec0[M["loss"]]) - r["loss"]) / abs(r["loss"]), np.abs(g0 - g).max(),
             1e-6 * max(1, np.abs(g).max()), np.abs(gd - gc).max(), 1e-6 * max(1, np.abs(gc).max()),
             "" if g64 is None else "; device - f64 %.2e, f32 oracle - f64 %.2e"
             % (np.abs(gd - g64 * coef).max(), np.abs(gc - g64 * coef).max()),
             np.abs(pd - p1).max(), abs(float(rec[M["grad_norm"]]) - r["total"]) / r["total"]))
    G = R.unflatten(g, dims)
    comp = {c: np.sqrt(sum(float((G[k].astype(np.float64) ** 2).sum()) for k in G if k.startswith(c)))
            for c in ("backbone", "policy_head", "value_head")}
    for which in (rec0, rec):
        np.testing.assert_allclose(which[M["loss"]], r["loss"], rtol=1e-5, atol=1e-6)
        for key, slot in METRICS + ([("roll/adv/norm/std", "adv_norm_std")] if normalize else []):
            np.testing.assert_allclose(which[M[slot]], met[key], atol=2e-6, rtol=1e-5, err_msg=key)
        if not normalize:
            assert which[M["adv_norm_mean"]] == 0 and which[M["adv_norm_std"]] == 0
        assert which[M["kl_stop"]] == which[M["skipped"]] == which[M["unevaluated"]] == 0
        # pre-clip norms: the total and the three components; GS_M_GN_MLP is 0
        np.testing.assert_allclose(which[M["grad_norm"]], r["total"], rtol=1e-5)
        for c in comp:
            np.testing.assert_allclose(which[M[f"gn_{c}"]], comp[c], rtol=2e-5, err_msg=c)
        assert which[M["gn_mlp"]] == 0
    assert np.array_equal(rec0.view(np.uint32), rec.view(np.uint32))      # the same forward and sums in both entries
    np.testing.assert_allclose(g0, g, atol=1e-6 * max(1, np.abs(g).max()), rtol=0)
    np.testing.assert_allclose(gd, gc, atol=1e-6 * max(1, np.abs(gc).max()), rtol=0)
    np.testing.assert_allclose(pd, p1, atol=5e-6, rtol=0)
    assert run.stop.item() == 0


# ------------------------------------------------------------------------------- four minibatches, one call
# seeds: the first from 1140 on whose four steps all meet the input conditions
FOUR = [((12, 128, 128, 18), 1040, 1165), ((12, 64, 18), 1040, 1140)]


@functools.lru_cache(maxsize=None)
def _four(shape):
    dims, B, seed = shape
    n, T = 4, 3
    N = -(-n * B // T) + 5
    case = C.case(dims, T, N, seed)
    idx = np.random.default_rng(seed).permutation(T * N)[:n * B]          # four disjoint minibatches
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    losses, steps = [], []
    for k in range(n):
        rows = C.rows(idx[k * B:(k + 1) * B], T, N)
        steps.append((p, rows))
        loss, met, _, _, _, p, m, v = C.oracle_step(case, p, m, v, rows, k + 1)
        steps[-1] += (met,)
        losses.append(loss)
    return dict(case=case, idx=idx, losses=losses, steps=steps, p=p, m=m, v=v)


@pytest.mark.parametrize("shape", FOUR, ids=_id)
def test_four_minibatches_in_one_update(cuda, shape):
    from gsamd._lib import M
    dims, B, seed = shape
    f = _four(shape)
    case, idx = f["case"], f["idx"]
    for p_k, rows, met in f["steps"]:
        _conditions(case, p_k, rows, met)
    run = _Run(case, cuda)
    rec = run.update(idx, B, 4)
    pd, pr = run.state()[0].astype(np.float64), f["p"].astype(np.float64)
    print("MEASURED %s losses rel %.2e (bar 1e-05) params rel L2 %.2e (bar 1e-05) max abs %.2e (bar 1e-03)"
          % (_id(shape), np.abs(rec[:, 0] / np.asarray(f["losses"]) - 1).max(),
             np.linalg.norm(pd - pr) / np.linalg.norm(pr), np.abs(pd - pr).max()))
    np.testing.assert_allclose(rec[:, M["loss"]], f["losses"], rtol=1e-5, atol=0)
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5
    assert np.abs(pd - pr).max() < 1e-3
    assert not rec[:, [M["kl_stop"], M["skipped"], M["unevaluated"]]].any()
    assert run.stop.item() == 0


# ------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("shape", [((12, 128, 128, 18), 1043, 1143), ((4, 16, 16, 2), 4115, 4215), ((12, 64, 18), 1043, 1143)],
                         ids=_id)
def test_two_runs_and_split_calls_give_the_same_bytes(cuda, shape):
    """Two runs of a three-minibatch update are byte-identical (parameters, moments, gradient,
    records), and one call with n_minibatches = 3 equals three calls of 1."""
    from gsamd._lib import GS_HP_ACT_STATS
    dims, B, seed = shape
    n, T = 3, 3
    N = -(-n * B // T) + 5
    case = C.case(dims, T, N, seed)
    idx = np.random.default_rng(seed).permutation(T * N)[:n * B]
    a, b, c = _Run(case, cuda), _Run(case, cuda), _Run(case, cuda)
    rec_a = a.update(idx, B, n, flags=GS_HP_ACT_STATS)
    rec_b = b.update(idx, B, n, flags=GS_HP_ACT_STATS)
    rec_c = np.concatenate([c.update(idx[k * B:(k + 1) * B], B, 1, step0=k, flags=GS_HP_ACT_STATS) for k in range(n)])
    assert np.isfinite(rec_a).all() and not np.array_equal(a.state()[0], case["p0"])
    assert _same_bytes(a.state() + [rec_a], b.state() + [rec_b])
    assert _same_bytes(a.state() + [rec_a], c.state() + [rec_c])


# ------------------------------------------------------------------------------- KL early stop
def test_kl_early_stop(cuda):
    """The case of test_gpu_mlp2_shapes.py::test_kl_early_stop_on_a_runtime_shape ((9, 64, 64, 6),
    B = 64: four row workgroups): target_kl lies between the oracle's approx_kl of steps 4 and 5,
    more than 10 % away from both (and from every earlier step), so the device stops at step 5."""
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
    assert 1.1 * akl[:kstar].max() <= target <= akl[kstar] / 1.1        # the oracle names step kstar, with margin
    run = _Run(case, cuda)
    rec = run.update(idx[:n * B], B, n, lr=lr, target_kl=target)
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
    assert plain.stop.item() == 0
    assert _same_bytes(stopped, plain.state())
    pd, pr = stopped[0].astype(np.float64), ps[kstar].astype(np.float64)
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5
    # a call that finds the flag set evaluates nothing and changes nothing
    rec2 = run.update(idx[:2 * B], B, 2, step0=kstar, lr=lr, target_kl=target)
    assert all(np.array_equal(x, later) for x in rec2) and _same_bytes(stopped, run.state())


# ------------------------------------------------------------------------------- activation statistics
# seeds: the first from B + 100 on that meets the test's own input condition (its docstring)
@pytest.mark.parametrize("shape", [((5, 48, 80, 3), 1100, 1201), ((12, 64, 18), 1043, 1144)], ids=_id)
def test_activation_statistics(cuda, shape):
    """GS_HP_ACT_STATS against numpy on the oracle's pre-activations: mean and unbiased std at 1e-5
    relative, dead_pct and dead_max exactly.  One unit of each layer has zero weights and bias, so its
    dead fraction is exactly 1; the oracle alone shows that no other pre-activation lies within a
    factor of two of the 1e-6 threshold, so the counts cannot depend on a kernel's summation order.
    B is no multiple of 16: the ragged tile's padding rows count for nothing."""
    from oracle import ppo_ref as R
    from gsamd._lib import ACT_SLOT, GS_HP_ACT_STATS, M
    dims, B, seed = shape
    r = _ref(shape)
    case, idx, rows = r["case"], r["idx"], r["rows"]
    P = {k: v.copy() for k, v in R.unflatten(case["p0"], dims).items()}
    nh = len(dims) - 2
    for i in range(nh):
        P[f"backbone.{2 * i}.weight"][3 + i] = 0
        P[f"backbone.{2 * i}.bias"][3 + i] = 0
    p0 = R.flatten(P, dims)
    x = case["obs"][rows]
    want = []
    for i in range(nh):
        z = (x @ P[f"backbone.{2 * i}.weight"].T + P[f"backbone.{2 * i}.bias"]).astype(np.float32)
        assert (z[:, 3 + i] == 0).all()
        az = np.abs(np.delete(z, 3 + i, axis=1))
        assert not ((az > 5e-7) & (az < 2e-6)).any()                    # the input condition, from the oracle alone
        cnt = (np.abs(z) < np.float32(1e-6)).sum(axis=0)
        assert cnt.max() == B
        zd = z.astype(np.float64)
        want.append((zd.mean(), zd.std(ddof=1), np.float32(cnt.sum() / (B * z.shape[1])), np.float32(cnt.max() / B)))
        x = np.maximum(z, np.float32(0))
    run = _Run(case, cuda, p0=p0)
    rec = run.update(idx, B, 1, flags=GS_HP_ACT_STATS)[0]
    assert np.isfinite(rec).all() and rec[M["grad_norm"]] > 0
    for i, (mean, std, pct, mx) in enumerate(want):
        got = rec[ACT_SLOT + 4 * i:ACT_SLOT + 4 * i + 4]
        print("MEASURED %s layer %d mean rel %.2e std rel %.2e (bars 1e-05) dead_pct %r == %r dead_max %r == %r"
              % (_id(shape), i, abs(got[0] - mean) / abs(mean), abs(got[1] - std) / std, got[2], pct, got[3], mx))
        np.testing.assert_allclose(got[0], mean, rtol=1e-5, atol=0)
        np.testing.assert_allclose(got[1], std, rtol=1e-5, atol=0)
        assert got[2] == pct and got[3] == mx == 1.0
    assert not rec[ACT_SLOT + 4 * nh:].any()
    # without the flag the slots stay 0
    off = _Run(case, cuda, p0=p0).update(idx, B, 1)[0]
    assert not off[ACT_SLOT:].any() and np.array_equal(off[:ACT_SLOT], rec[:ACT_SLOT])


# ------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_buffer_unchanged(cuda):
    from gsamd._lib import GS_HP_BF16, GS_NUM_METRICS, MlpDims, PPOHparams, RolloutView, check, lib
    T, N = 3, 800
    ok = MlpDims(6, 128, 128, 3)
    P = int(lib.gs_mlp_param_count(ok))
    rng = np.random.default_rng(3)
    bufs = [_dev(rng.standard_normal(P).astype(np.float32), cuda) for _ in range(4)]      # params, grads, m, v
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

    def update(dims=ok, B=2048, hp_=None, wsp=ws.data_ptr(), nbytes=need, comm=None, stop_p=stop.data_ptr()):
        check(lib.gs_ppo_rows_update(p, g, m, v, dims, hp_ or hp(), view, idx.data_ptr(), B, 1, 0, met.data_ptr(), stop_p,
                                     wsp, nbytes, comm, s), "gs_ppo_rows_update")

    def loss(dims=ok, B=2048, hp_=None, wsp=ws.data_ptr(), nbytes=need, **_):
        check(lib.gs_ppo_rows_loss(p, g, dims, hp_ or hp(), view, idx.data_ptr(), B, met.data_ptr(), wsp, nbytes, s),
              "gs_ppo_rows_loss")
    cases = [(dict(dims=MlpDims(6, 40, 128, 3)), "hidden1 40 must be a multiple of 16"),
             (dict(dims=MlpDims(6, 528, 128, 3)), "hidden1 528 must be a multiple of 16"),
             (dict(dims=MlpDims(6, 128, 1024, 3)), "hidden2 1024 must be 0"),
             (dict(dims=MlpDims(65, 128, 128, 3)), r"obs_dim 65 outside \[1, 64\]"),
             (dict(dims=MlpDims(6, 128, 128, 33)), r"n_actions 33 outside \[1, 32\]"),
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
    # the chain's entries keep their bound
    with pytest.raises(ValueError, match=r"batch 1025 outside \[2, 1024\]"):
        check(lib.gs_ppo_update(p, g, m, v, ok, hp(), view, idx.data_ptr(), 1025, 1, 0, met.data_ptr(), stop.data_ptr(),
                                ws.data_ptr(), ws.numel(), None, 0, s), "gs_ppo_update")
    torch.cuda.synchronize()
    for a, b in zip(before, bufs + [met, stop, ws]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------- agent
# (env, overrides, minibatches per epoch, seed of the tensor batch: the first from 2148 on with ReLU margins >= 1e-6)
AGENTS = [("CartPole-v1", dict(n_envs=64, n_steps=32, batch_size=2048, n_epochs=2, env_dynamics="cartpole"), 2, 2181),
          ("FrozenLake-v1", dict(n_envs=16, n_steps=128, batch_size=2048, n_epochs=1), 1, 2148)]


@pytest.mark.parametrize("env,over,per_epoch,seed", AGENTS, ids=[a[0] for a in AGENTS])
def test_agent_trains_with_a_2048_row_minibatch(cuda, env, over, per_epoch, seed):
    """DevicePPOAgent with batch_size = 2048 (the chain's entries refuse it: `batch 2048 outside
    [2, 1024]`): two epochs train on the device env with finite records, the optimizer steps as counted
    and moving weights; losses_for_batch on a 2048-row tensor batch matches the oracle's loss."""
    from oracle import ppo_ref as R
    from gsamd._lib import M
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(42)
    agent = DevicePPOAgent(load_config(env, "ppo", overrides=over), device=cuda)
    assert agent.batch_size == 2048 and agent.n_minibatches == per_epoch and agent._use_rows(agent.batch_size)
    p0 = agent.policy_model.params.clone()
    for _ in range(2):
        agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all() and agent.adam_step == 2 * per_epoch
    rec = agent.metrics_buf.cpu().numpy()
    assert np.isfinite(rec).all() and (rec[:, M["grad_norm"]] > 0).all() and not rec[:, M["skipped"]].any()
    assert not torch.equal(p0, agent.policy_model.params)
    m = agent.epoch_metrics()
    assert m["opt/grads/norm/all"] > 0 and "opt/activations/backbone.0/mean" in m
    # losses_for_batch / training_step on a tensor batch of 2048 rows
    d = agent.policy_model.dims
    dims = (d.obs_dim, d.hidden1, d.hidden2, d.n_actions) if d.hidden2 else (d.obs_dim, d.hidden1, d.n_actions)
    B = 2048
    case = C.case(dims, 1, B, seed)
    agent.policy_model.load_flat(case["p0"])
    batch = types.SimpleNamespace(observations=torch.as_tensor(case["obs"]), actions=torch.as_tensor(case["actions"]),
                                  logprobs=torch.as_tensor(case["old_logp"]), values=torch.as_tensor(case["old_values"]),
                                  advantages=torch.as_tensor(case["adv"]), returns=torch.as_tensor(case["ret"]))
    c = agent.config
    want, met, _ = R.ppo_loss_and_grads(case["p0"], dims, case["obs"], case["actions"], case["old_logp"], case["old_values"],
                                        case["adv"], case["ret"], clip=float(agent.clip_range),
                                        clip_vf=float(agent.clip_range_vf), vf_coef=float(agent.vf_coef),
                                        ent_coef=float(agent.ent_coef),
                                        normalize="batch" if c.normalize_advantages == "batch" else None)
    assert min(C.preact_margins(case["p0"], dims, case["obs"])) >= 1e-6
    out = agent.losses_for_batch(batch, 0)
    got = float(out["loss"].item())
    print("MEASURED %s losses_for_batch rel %.2e (bar 1e-05)" % (env, abs(got - want) / abs(want)))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    assert np.array_equal(agent.policy_model.params.cpu().numpy(), case["p0"])      # no optimizer step
    steps = agent.adam_step
    agent.training_step(batch, 0)
    torch.cuda.synchronize()
    assert agent.adam_step == steps + 1 and not np.array_equal(agent.policy_model.params.cpu().numpy(), case["p0"])
