"""AdamW and SGD on the device update paths (include/gsamd.h GS_HP_OPT_ADAMW / GS_HP_OPT_SGD) through
the C ABI — gs_ppo_update (the compile-time fused shape, which has the lagged Adam form, and the
runtime-shape chain), gs_ppo_minibatch_step, the one-hidden-layer update, the row-parallel update
with and without a mask, gs_pg_update and gs_cnn_ppo_update — and DevicePPOAgent /
DeviceREINFORCEAgent with config.optimizer.

Cases are built as tests/test_gpu_ppo_rows.py::_ref builds them from tests/mlp_cases.py (T = 3,
N = max(40, ceil(B/3) + 5), idx = default_rng(B + D).permutation(T N)[:B]; a call of n minibatches
repeats that minibatch), with one change: the last observation column is zero, so the gradient of
W1[:, D-1] is exactly 0 (asserted from the oracle).  A case's seed is the first from B + 100 on that
meets that module's input conditions (first_seed below; asserted from the oracle alone).  The
NatureCNN case is tests/golden/cnn_step.npz's "pong" (tests/test_gpu_cnn.py::_setup), its
zero-gradient entries the invalid actions' policy-head rows.

Every check runs at lr = 0.05: the decay 0.05 * 0.01 * |p| and the SGD step 0.05 * g stand far above
the float32 roundings the bounds allow.
1. AdamW against Adam, one step from the same state: m and v bit-equal; per entry
   |p_adamw - p_adam - (d - 1) p0| <= 2 * 2^-23 * max(|p0|, |p_adamw|, |p_adam|), d the float32
   factor, the left side in float64 — three float32 roundings (the decay multiply, the two final
   adds).  First, from p0 alone: the decay exceeds 100x that bound (taken at |p0| + lr, which the
   first Adam step cannot leave) for at least half the entries.
2. SGD, one step: |p_dev - (p0 - f32(lr) gc_oracle)| <= lr * 1e-6 * max|gc| + 2^-23 |p0| (the
   clipped-gradient bar through a linear map, plus one rounding); m and v, pre-filled with -3, are
   still -3.  First, from the oracle: Adam's step differs from SGD's by at least 100x the bar for
   at least half the entries.
3. Zero-gradient entries over four steps: AdamW p0 * d^4 by repeated float32 multiply bit for bit,
   moments 0; SGD and Adam p0 bit for bit.
4. Graph replay on the two gs_ppo_update shapes.
5. The agents."""
import functools
import json

import numpy as np
import pytest
import torch

import masked_mlp_twin as TW
import mlp_cases as C
import optimizer_twin as OT
import reinforce_twin as PG
from mlp_cases import HP, MAX_NORM

pytestmark = pytest.mark.gpu

LR = 0.05
EPS23 = 2.0 ** -23
N_MAX = 4
VALID = (0, 3, 4)
# name: (kind, dims, B, case seed)
PATHS = {
    "update-fused": ("update", (4, 256, 256, 2), 256, 356),
    "update-runtime": ("update", (6, 128, 128, 3), 64, 164),
    "minibatch-step": ("step", (4, 64, 64, 2), 64, 164),
    "one-hidden-layer": ("update", (12, 64, 18), 64, 164),
    "rows": ("rows", (4, 16, 16, 2), 1043, 1144),
    "rows-masked": ("masked", (12, 128, 128, 18), 1043, 1143),
    "reinforce": ("pg", (10, 128, 128, 10), 130, 230),
}
PG_ENT = 0.01


def _zero_last_column(case):
    c = dict(case)
    c["obs"] = case["obs"].copy()
    c["obs"][:, -1] = 0.0
    return c


def _build(name, seed):
    """One path's case with the zeroed column, its minibatch and the oracle's first step from zero
    moments -> dict with ok (the input conditions), gc (the clipped gradient), zero (the flat indices of
    W1[:, D-1]) and, where only part of the net takes a step, stepped (a mask over the parameters)."""
    kind, dims, B, _ = PATHS[name]
    D = dims[0]
    T, N = 3, max(40, -(-B // 3) + 5)
    case = _zero_last_column(TW.case(dims, VALID, T, N, seed) if kind == "masked" else C.case(dims, T, N, seed))
    idx = np.random.default_rng(B + D).permutation(T * N)[:B]
    rows = C.rows(idx, T, N)
    p0 = case["p0"]
    zeros = np.zeros_like(p0)
    stepped = np.ones(p0.size, bool)
    if kind == "masked":
        _, met, _, gc, _, _, _, _ = TW.step(case, p0, zeros, zeros, rows, 1)
        ok = TW.conditions_met(case, p0, rows, met)
    else:
        _, met, _, gc, _, _, _, _ = C.oracle_step(case, p0, zeros, zeros, rows, 1)
        ok = (0 < met["opt/ppo/clip_fraction"] < 1 and 0 < met["opt/ppo/clip_fraction_vf"] < 1 and
              min(C.preact_margins(p0, dims, case["obs"][rows])) >= 1e-6)
    if kind == "pg":    # the REINFORCE loss on the same rows: targets = the case's returns, batch-normalised
        rec, g = PG.loss_and_grads(p0, dims, case["obs"][rows], case["actions"][rows], case["old_logp"][rows],
                                   case["ret"][rows], PG_ENT, True)
        gc = (g * np.float32(min(1.0, MAX_NORM / (rec["grad_norm"] + 1e-6)))).astype(np.float32)
        stepped[-(dims[2] + 1):] = False            # the value head: no gradient, no step, no decay
    zero = np.arange(dims[1]) * D + (D - 1)
    return dict(case=case, idx=idx, rows=rows, gc=np.asarray(gc, np.float32), ok=bool(ok), zero=zero, stepped=stepped,
                B=B, dims=dims, kind=kind)


def first_seed(name):
    """How PATHS' seeds were found (oracle only; not run by the tests)."""
    seed = PATHS[name][2] + 100
    while not _build(name, seed)["ok"]:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Shared by the tests; never written to."""
    return _build(name, PATHS[name][3])


def _dev(a, cuda, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(cuda).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Run:
    """Device buffers of one path, allocated once (a captured graph is keyed by them), and the C-ABI
    call of its update entry.  run() is n minibatches (the case's one, repeated) from adam_step0."""

    def __init__(self, ref, cuda):
        from gsamd._lib import GS_NUM_METRICS, MlpDims, RolloutView, lib
        c, self.kind, self.B, self.cuda = ref["case"], ref["kind"], ref["B"], cuda
        T, N, dims = c["T"], c["N"], ref["dims"]
        self.dims = MlpDims(dims[0], dims[1], dims[2] if len(dims) == 4 else 0, dims[-1])
        self.P = int(lib.gs_mlp_param_count(self.dims))
        assert self.P == c["p0"].size
        pg = self.kind == "pg"
        self.keep = dict(obs=_dev(c["obs"].reshape(T, N, dims[0]), cuda),
                         actions=_dev(c["actions"].reshape(T, N), cuda, torch.int64),
                         logprobs=_dev(c["old_logp"].reshape(T, N), cuda), values=_dev(c["old_values"].reshape(T, N), cuda),
                         advantages=_dev((c["ret"] if pg else c["adv"]).reshape(T, N), cuda),
                         returns=_dev(c["ret"].reshape(T, N), cuda))
        k = self.keep
        self.view = RolloutView(k["obs"].data_ptr(), k["actions"].data_ptr(), k["logprobs"].data_ptr(),
                                None if pg else k["values"].data_ptr(), k["advantages"].data_ptr(),
                                None if pg else k["returns"].data_ptr(), T, N)
        self.params, self.grads, self.m, self.v = (torch.zeros(self.P, device=cuda) for _ in range(4))
        self.stop = torch.zeros(1, dtype=torch.int32, device=cuda)
        self.met = torch.zeros(N_MAX, GS_NUM_METRICS, device=cuda)
        self.idx = _dev(np.tile(ref["idx"], N_MAX), cuda, torch.int32)
        nbytes = {"update": lambda: lib.gs_ppo_update_workspace_bytes(self.dims, self.B, N_MAX),
                  "step": lambda: lib.gs_ppo_workspace_bytes(self.dims, self.B),
                  "rows": lambda: lib.gs_ppo_rows_workspace_bytes(self.dims, self.B),
                  "masked": lambda: lib.gs_ppo_rows_workspace_bytes(self.dims, self.B),
                  "pg": lambda: lib.gs_pg_update_workspace_bytes(self.dims, self.B)}[self.kind]()
        assert int(nbytes) > 0
        self.ws = torch.zeros(int(nbytes), dtype=torch.uint8, device=cuda)
        self.p0 = c["p0"]

    def load(self, fill=0.0, p=None):
        self.params.copy_(_dev(self.p0 if p is None else p, self.cuda))
        self.m.fill_(fill)
        self.v.fill_(fill)
        self.grads.zero_()
        self.stop.zero_()
        return self

    def run(self, n, flags, step0=0, use_graph=0, lr=LR):
        from gsamd._lib import PGHparams, PPOHparams, check, lib
        assert 1 <= n <= N_MAX
        hp = PPOHparams(HP["clip"], HP["clip_vf"], HP["vf_coef"], HP["ent_coef"], MAX_NORM, lr, 0.9, 0.999, 1e-8, 0.0, 1,
                        flags)
        a = (self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.dims)
        idx, met, ws = self.idx.data_ptr(), self.met.data_ptr(), self.ws
        if self.kind == "update":
            check(lib.gs_ppo_update(*a, hp, self.view, idx, self.B, n, step0, met, self.stop.data_ptr(), ws.data_ptr(),
                                    ws.numel(), None, use_graph, _stream()), "gs_ppo_update")
        elif self.kind == "step":
            for k in range(n):
                check(lib.gs_ppo_minibatch_step(*a, hp, self.view, idx, self.B, step0 + k + 1, met, self.stop.data_ptr(),
                                                ws.data_ptr(), None, _stream()), "gs_ppo_minibatch_step")
        elif self.kind == "rows":
            check(lib.gs_ppo_rows_update(*a, hp, self.view, idx, self.B, n, step0, met, self.stop.data_ptr(),
                                         ws.data_ptr(), ws.numel(), None, _stream()), "gs_ppo_rows_update")
        elif self.kind == "masked":
            check(lib.gs_ppo_rows_update_masked(*a, hp, self.view, idx, self.B, n, step0, met, self.stop.data_ptr(),
                                                ws.data_ptr(), ws.numel(), None, _stream(), TW.mask_of(VALID)),
                  "gs_ppo_rows_update_masked")
        else:
            pg = PGHparams(PG_ENT, MAX_NORM, lr, 0.9, 0.999, 1e-8, 1, flags)
            check(lib.gs_pg_update(*a, pg, self.view, idx, self.B, n, step0, met, ws.data_ptr(), ws.numel(), None,
                                   _stream()), "gs_pg_update")
        torch.cuda.synchronize()
        assert self.stop.item() == 0
        return self.state()

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.params, self.m, self.v)]


class _CnnRun:
    """The NatureCNN case on the device; parameters and moments are read back in the reference's layout."""

    def __init__(self, cuda):
        import test_gpu_cnn as TC
        from gsamd._lib import GS_NUM_METRICS, lib
        self.pm, self.p0, self.bufs, self.view, _, self.idx, self.batch = TC._setup(cuda, "pong")
        self.valid, self.clip, self.ent, _, self.B, _, _ = TC.CASES["pong"]
        P = self.pm.n_params
        self.grads, self.m, self.v = (torch.zeros(P, device=cuda) for _ in range(3))
        self.ws = torch.empty(int(lib.gs_cnn_workspace_bytes(self.pm.dims, self.B)), dtype=torch.uint8, device=cuda)
        self.met = torch.zeros(N_MAX, GS_NUM_METRICS, device=cuda)
        self.stop = torch.zeros(1, dtype=torch.int32, device=cuda)
        self.idx4 = self.idx.repeat(N_MAX).contiguous()

    def load(self, fill=0.0):
        self.pm.load_reference_flat(self.p0)
        self.m.fill_(fill)
        self.v.fill_(fill)
        self.grads.zero_()
        return self

    def run(self, n, flags, step0=0, lr=LR):
        from gsamd._lib import PPOHparams, check, lib
        hp = PPOHparams(self.clip, 0.2, 0.5, self.ent, 0.5, lr, 0.9, 0.999, 1e-8, 0.0, 1, flags)
        pm = self.pm
        check(lib.gs_cnn_ppo_update(pm.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                    pm.dims, hp, self.view, self.idx4.data_ptr(), self.B, n, step0, self.met.data_ptr(),
                                    self.stop.data_ptr(), self.ws.data_ptr(), None, _stream()), "gs_cnn_ppo_update")
        torch.cuda.synchronize()
        return [pm.flat_to_reference(t).copy() for t in (pm.params, self.m, self.v)]


@functools.lru_cache(maxsize=None)
def _cnn_ref():
    """The NatureCNN case's clipped oracle gradient and its invalid actions' policy-head entries
    (reference layout); shared, never written to."""
    import test_gpu_cnn as TC
    from oracle import cnn_case as K
    from oracle import cnn_ref as CR
    valid, clip, ent, _, B, pseed, bseed = TC.CASES["pong"]
    p0 = K.cnn_params(pseed)
    shapes = CR.cnn_param_shapes()
    _, _, g, _, _ = CR.loss_and_grads(p0, shapes, *K.cnn_batch(bseed, B, valid), valid=valid, clip=clip, clip_vf=0.2,
                                      vf_coef=0.5, ent_coef=ent)
    z = np.zeros(p0.size, np.float32)
    _, _, _, gc, _ = CR.clip_and_adam(p0, g, shapes, z, z.copy(), 1, LR)
    off, o = {}, 0
    for name, shp in shapes:
        off[name] = (o, shp)
        o += int(np.prod(shp))
    (ow, (A, H)), (ob, _) = off["policy_head.weight"], off["policy_head.bias"]
    inv = [a for a in range(A) if a not in valid]
    zero = np.concatenate([np.arange(ow + a * H, ow + (a + 1) * H) for a in inv] + [np.array([ob + a]) for a in inv])
    return dict(p0=p0, gc=np.asarray(gc, np.float32), zero=zero, stepped=np.ones(p0.size, bool))


def _flags():
    from gsamd._lib import GS_HP_OPT_ADAMW, GS_HP_OPT_SGD
    return {"adam": 0, "adamw": GS_HP_OPT_ADAMW, "sgd": GS_HP_OPT_SGD}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


# ------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(PATHS))
def test_input_conditions(name):
    """From the oracle alone: the module's input conditions hold at the case's seed, the gradient of
    W1[:, D-1] is exactly zero and the rest of the clipped gradient is not."""
    r = _ref(name)
    assert r["ok"]
    assert r["zero"].size == r["dims"][1] and not r["gc"][r["zero"]].any()
    assert np.count_nonzero(r["gc"]) > r["gc"].size // 2


def _check_differential(tag, p0, stepped, adam, adamw):
    """check 1 of the module docstring"""
    d = OT.decay_factor(LR)
    a0 = np.abs(p0.astype(np.float64))
    assert ((LR * OT.WEIGHT_DECAY * a0 > 100 * 2 * EPS23 * (a0 + LR))[stepped]).mean() >= 0.5      # from p0 alone
    (pa, ma, va), (pw, mw, vw) = adam, adamw
    assert _same((ma, va), (mw, vw))
    assert ma[stepped].any() and va[stepped].any()
    f64 = lambda x: x.astype(np.float64)  # noqa: E731
    left = np.abs(f64(pw) - f64(pa) - (float(d) - 1.0) * f64(p0))
    bound = 2 * EPS23 * np.maximum(a0, np.maximum(np.abs(f64(pw)), np.abs(f64(pa))))
    nz = stepped & (bound > 0)                   # a parameter that is and stays exactly 0 has a bound of 0, which it meets
    print("MEASURED %s AdamW - Adam - (d - 1) p0: worst %.2f of the bound, decay / bound median %.0f"
          % (tag, float((left[nz] / bound[nz]).max()), float(np.median(LR * OT.WEIGHT_DECAY * a0[nz] / bound[nz]))))
    assert (left[stepped] <= bound[stepped]).all()
    # what takes no step (REINFORCE's value head) is not decayed either
    assert _same((pw[~stepped], pa[~stepped]), (p0[~stepped], p0[~stepped]))
    assert not np.array_equal(_bits(pw[stepped]), _bits(pa[stepped]))


def _check_sgd(tag, p0, gc, stepped, sgd):
    """check 2 of the module docstring"""
    from oracle import ppo_ref as R
    ps, ms, vs = sgd
    lr32 = float(np.float32(LR))
    want = p0.astype(np.float64) - lr32 * gc.astype(np.float64)
    bar = LR * 1e-6 * float(np.abs(gc).max()) + EPS23 * np.abs(p0.astype(np.float64))
    z = np.zeros_like(p0)
    p_adam, _, _ = R.adam_step(p0, gc, z, z, 1, LR)                  # from the oracle: Adam's step is another one
    apart = np.abs(p_adam.astype(np.float64) - want)
    assert ((apart >= 100 * bar)[stepped]).mean() >= 0.5
    err = np.abs(ps.astype(np.float64) - want)
    print("MEASURED %s SGD step: worst %.3f of the bar (max-abs %.2e, lr max|gc| %.2e); Adam - SGD median %.0f bars"
          % (tag, float((err[stepped] / bar[stepped]).max()), float(err[stepped].max()), LR * float(np.abs(gc).max()),
             float(np.median(apart[stepped] / bar[stepped]))))
    assert (err[stepped] <= bar[stepped]).all()
    assert _same((ps[~stepped],), (p0[~stepped],))
    assert (ms == -3.0).all() and (vs == -3.0).all()


def _check_zero_entries(p0, zero, runs):
    """check 3 of the module docstring; runs: name -> (p, m, v) after four steps from zero moments"""
    for name, (p, m, v) in runs.items():
        want = OT.decayed(p0[zero], LR, 4) if name == "adamw" else p0[zero]
        assert np.array_equal(_bits(p[zero]), _bits(want)), name
        assert not m[zero].any() and not v[zero].any(), name
        moved = np.ones(p0.size, bool)
        moved[zero] = False
        assert not np.array_equal(_bits(p[moved]), _bits(p0[moved])), name
    assert not np.array_equal(_bits(runs["adamw"][0][zero]), _bits(p0[zero]))


# ------------------------------------------------------------------------------- checks 1-3, MLP paths
@pytest.mark.parametrize("name", list(PATHS))
def test_adamw_and_sgd_steps(cuda, name):
    """Checks 1, 2 and 3 on one path (module docstring).  rows-masked: check 3 also on the invalid
    actions' policy-head rows.  reinforce: under AdamW every value-head parameter is bit-equal to p0
    with zero moments, and policy_head.bias has moved."""
    from oracle import ppo_ref as R
    r = _ref(name)
    assert r["ok"] and not r["gc"][r["zero"]].any()
    p0, gc, stepped, F = r["case"]["p0"], r["gc"], r["stepped"], _flags()
    run = _Run(r, cuda)
    one = {o: run.load().run(1, F[o]) for o in ("adam", "adamw")}
    _check_differential(name, p0, stepped, one["adam"], one["adamw"])
    _check_sgd(name, p0, gc, stepped, run.load(fill=-3.0).run(1, F["sgd"]))
    four = {o: run.load().run(4, F[o]) for o in ("adam", "adamw", "sgd")}
    assert all(np.isfinite(x).all() for s in four.values() for x in s)
    assert not four["sgd"][1].any() and not four["sgd"][2].any()
    zero = r["zero"]
    if name == "rows-masked":
        zero = np.concatenate([zero, TW.invalid_slices(r["dims"], VALID)])
    _check_zero_entries(p0, zero, four)
    if name == "reinforce":
        nv = r["dims"][2] + 1
        p, m, v = four["adamw"]
        assert np.array_equal(_bits(p[-nv:]), _bits(p0[-nv:])) and not m[-nv:].any() and not v[-nv:].any()
        bias = lambda flat: R.unflatten(flat, r["dims"])["policy_head.bias"]  # noqa: E731
        assert (bias(p) != bias(p0)).all()


def test_adamw_and_sgd_steps_nature_cnn(cuda):
    """Checks 1 and 2 on gs_cnn_ppo_update at the case of tests/golden/cnn_step.npz, one step at its
    batch; check 3 on the invalid actions' policy-head rows, whose gradient oracle/cnn_ref.py gives as
    exactly zero (asserted; were it not, this test would say so and end after checks 1 and 2)."""
    r, F = _cnn_ref(), _flags()
    p0, gc, zero = r["p0"], r["gc"], r["zero"]
    run = _CnnRun(cuda)
    assert np.array_equal(run.p0, p0)
    one = {o: run.load().run(1, F[o]) for o in ("adam", "adamw")}
    _check_differential("nature-cnn", p0, r["stepped"], one["adam"], one["adamw"])
    _check_sgd("nature-cnn", p0, gc, r["stepped"], run.load(fill=-3.0).run(1, F["sgd"]))
    if gc[zero].any():
        print("nature-cnn: cnn_ref's gradient of the invalid policy-head rows is not exactly zero: checks 1 and 2 only")
        return
    four = {o: run.load().run(4, F[o]) for o in ("adam", "adamw", "sgd")}
    assert not four["sgd"][1].any() and not four["sgd"][2].any()
    _check_zero_entries(p0, zero, four)


# ------------------------------------------------------------------------------- check 4
@pytest.mark.parametrize("name", ["update-fused", "update-runtime"])
def test_graph_replay_and_the_adam_calls_around_it(cuda, name):
    """gs_ppo_update with use_graph = 1 on one set of buffers (what a captured graph is keyed by): three
    minibatches in one call equal three calls of one with adam_step0 = 0, 1, 2, bit for bit in p, m and
    v, for AdamW and for SGD; at another lr the same holds (the decay factor and SGD's step size follow
    the call's lr).  The Adam call before them and the Adam call after them give the same bytes, which
    are the eager (use_graph = 0) Adam call's: the optimizer bit selects a graph of its own."""
    r, F = _ref(name), _flags()
    assert r["ok"]
    run = _Run(r, cuda)
    adam_eager = run.load().run(3, F["adam"])
    adam_before = run.load().run(3, F["adam"], use_graph=1)
    seen = {}
    for o in ("adamw", "sgd"):
        for lr in (LR, 3e-4):
            whole = run.load().run(3, F[o], use_graph=1, lr=lr)
            run.load()
            for k in range(3):
                split = run.run(1, F[o], step0=k, use_graph=1, lr=lr)
            eager = run.load().run(3, F[o], lr=lr)
            assert _same(whole, split) and _same(whole, eager), (o, lr)
            seen[o, lr] = whole
        assert not _same(seen[o, LR][:1], seen[o, 3e-4][:1])
    adam_after = run.load().run(3, F["adam"], use_graph=1)
    assert _same(adam_before, adam_after) and _same(adam_before, adam_eager)
    assert not _same(adam_before[:1], seen["adamw", LR][:1]) and not _same(adam_before[:1], seen["sgd", LR][:1])
    assert not seen["sgd", LR][1].any() and not seen["sgd", LR][2].any() and seen["adamw", LR][1].any()


# ------------------------------------------------------------------------------- check 5: the agents
def _ppo_agent(cuda, optimizer):
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent
    torch.manual_seed(42)
    over = dict(n_envs=8, n_steps=32, batch_size=64, n_epochs=2, model_id="mlp_small", env_dynamics="cartpole",
                optimizer=optimizer)
    return DevicePPOAgent(load_config("CartPole-v1", "ppo", overrides=over), device=cuda)


ENV_STATE = ("state", "meta", "ep_ret", "obs")


@pytest.mark.parametrize("optimizer", ["adamw", "sgd"])
def test_agent_trains_and_resumes(cuda, tmp_path, optimizer):
    """DevicePPOAgent on device CartPole (8 envs x 32 steps, batch 64, 2 epochs, mlp_small): two epochs
    run and every recorded metric is finite.  save_checkpoint: the matching torch optimizer over CPU
    parameters of the same shapes accepts optimizer.pt through load_state_dict and its group shows
    torch's defaults; a fresh agent of the same optimizer loads the checkpoint and its next epoch is
    bit-equal to the uninterrupted run's (the checkpoint holds the learner, not the env: the env's
    state tensors at the checkpoint are handed to the fresh agent's env); a fresh agent of another
    optimizer gets a ValueError naming both."""
    from gsamd._lib import M
    agent = _ppo_agent(cuda, optimizer)
    assert agent.optimizer_name == optimizer and agent.n_minibatches == 8
    p0 = agent.policy_model.params.clone()
    for _ in range(2):
        agent.train_epoch()
        torch.cuda.synchronize()
        rec = agent.metrics_buf.cpu().numpy()
        assert np.isfinite(rec).all() and (rec[:, M["grad_norm"]] > 0).all() and not rec[:, M["skipped"]].any()
        assert all(np.isfinite(v) for v in agent.epoch_metrics().values() if isinstance(v, float))
    assert np.isfinite(agent.minibatch_losses()).all() and agent.adam_step == 16
    assert not torch.equal(p0, agent.policy_model.params)
    assert bool(agent.adam_m.any()) == (optimizer == "adamw") == bool(agent.adam_v.any())
    # the checkpoint in torch's layout
    agent.save_checkpoint(tmp_path)
    assert json.loads((tmp_path / "state.json").read_text())["optimizer"] == optimizer
    sd = torch.load(tmp_path / "optimizer.pt", map_location="cpu", weights_only=True)[0]
    params = [torch.nn.Parameter(torch.zeros(shp)) for _, shp in agent.policy_model.shapes()]
    opt = (torch.optim.AdamW if optimizer == "adamw" else torch.optim.SGD)(params, lr=1.0)
    opt.load_state_dict(sd)
    group = opt.param_groups[0]
    assert group["lr"] == pytest.approx(agent.policy_lr)
    if optimizer == "adamw":
        assert group["weight_decay"] == 0.01 and group["decoupled_weight_decay"] is True
        assert group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8 and group["amsgrad"] is False
        assert len(opt.state) == len(params) and all(float(s["step"]) == 16 for s in opt.state.values())
        assert all(s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape for p, s in opt.state.items())
    else:
        assert group["momentum"] == 0 and group["dampening"] == 0 and group["weight_decay"] == 0
        assert group["nesterov"] is False and len(opt.state) == 0 and sd["state"] == {}
    # resume: the same optimizer continues bit for bit, another one is refused
    env = agent.get_env("train")
    snap = {k: getattr(env, k).clone() for k in ENV_STATE}
    agent.train_epoch()
    torch.cuda.synchronize()
    other = _ppo_agent(cuda, optimizer)
    other.load_checkpoint(tmp_path)
    assert other.adam_step == 16 and other.current_epoch == agent.current_epoch - 1
    assert other.get_rollout_collector("train").buffer is not None       # the collector's first use resets its env
    oenv = other.get_env("train")
    for k in ENV_STATE:
        getattr(oenv, k).copy_(snap[k])
    other.train_epoch()
    torch.cuda.synchronize()
    for x, y in ((agent.policy_model.params, other.policy_model.params), (agent.adam_m, other.adam_m),
                 (agent.adam_v, other.adam_v), (agent.metrics_buf, other.metrics_buf)):
        assert torch.equal(x, y)
    wrong = "sgd" if optimizer == "adamw" else "adam"
    with pytest.raises(ValueError, match=f"optimizer '{optimizer}'.*'{wrong}'"):
        _ppo_agent(cuda, wrong).load_checkpoint(tmp_path)


def test_reinforce_agent_runs_an_epoch_of_sgd(cuda):
    from gsamd import build_agent
    from gsamd._lib import GS_HP_OPT_SGD
    from gsamd.config import load_config
    torch.manual_seed(42)
    agent = build_agent(load_config("Bandit-v0", "reinforce", overrides=dict(optimizer="sgd")), device=cuda)
    assert agent.optimizer_name == "sgd" and int(agent.hparams().flags) & GS_HP_OPT_SGD
    p0 = agent.policy_model.params.clone()
    agent.train_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(agent.minibatch_losses()).all() and agent.adam_step == agent.n_minibatches
    assert np.isfinite(agent.metrics_buf.cpu().numpy()).all()
    assert not torch.equal(p0, agent.policy_model.params) and not agent.adam_m.any() and not agent.adam_v.any()
