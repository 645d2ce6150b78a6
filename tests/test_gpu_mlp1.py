"""The one-hidden-layer actor-critic (gs_mlp_dims.hidden2 == 0, csrc/gs_mlp1.hip) against the numpy
oracle (oracle.ppo_ref with dims = (D, H, A)): the rollout-step forward, sampling against the
two-hidden-layer head on the identity-extended net, one minibatch step, eight minibatches in one
launch (determinism, split runs), the KL early stop and the refusals.

Bars are those of tests/test_gpu_parity.py for two hidden layers: log-prob / value 1e-5 absolute;
loss 1e-5 relative; clipped gradient 1e-6 of its largest entry; parameters after one Adam step
5e-6; after eight steps 1e-5 relative L2 and 1e-3 max-abs (Adam turns last-bit gradient differences
of near-zero-gradient weights into up to lr-sized moves)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 4, 37), (16, 64, 4, 256), (9, 64, 6, 1000), (5, 16, 3, 17)]
HP = dict(clip=0.2, clip_vf=0.2, vf_coef=0.5, ent_coef=0.01)
MAX_NORM, LR = 0.5, 3e-4


def _dev(a, cuda, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(cuda).contiguous()


def _params(D, H, A, seed, dims=None):
    """A random net with O(1) logits gaps (the reference's 0.01-gain policy head would leave every
    row near uniform)."""
    from oracle import ppo_ref as R
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in R.param_shapes(dims or (D, H, A)):
        if name.endswith("bias"):
            out[name] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
        else:
            scale = (1.0 if name.startswith("policy") else 0.5) / np.sqrt(shp[-1])
            out[name] = (scale * rng.standard_normal(shp)).astype(np.float32)
    return out


def _flat(D, H, A, seed):
    from oracle import ppo_ref as R
    return R.flatten(_params(D, H, A, seed), (D, H, A))


def _obs(D, n, rng):
    """Observations of magnitude at most 16: state indices 0..15 (D = 1), one-hot (D = 16) or bit
    vectors (D = 9) of a state, N(0, 1) otherwise."""
    if D == 1:
        return rng.integers(0, 16, (n, 1)).astype(np.float32)
    if D == 16:
        return np.eye(16, dtype=np.float32)[rng.integers(0, 16, n)]
    if D == 9:
        s = rng.integers(0, 500, n)
        return ((s[:, None] >> np.arange(9)) & 1).astype(np.float32)
    return rng.standard_normal((n, D)).astype(np.float32)


def _model(D, H, A, flat, cuda):
    from gsamd.policy import DeviceMLPActorCritic
    pm = DeviceMLPActorCritic(D, (H,), A, device=cuda, init=False)
    pm.load_flat(flat)
    return pm


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("D,H,A,N", SHAPES)
def test_forward_replay_value_store_and_clock(cuda, D, H, A, N):
    from oracle import ppo_ref as R
    rng = np.random.default_rng(D * 131 + N)
    flat = _flat(D, H, A, seed=N)
    obs = _obs(D, N, rng)
    acts = rng.integers(0, A, N)
    logits, value, _ = R.forward(flat, (D, H, A), obs)
    logp = R.log_softmax(logits)[np.arange(N), acts]
    pm = _model(D, H, A, flat, cuda)
    assert pm.n_params == flat.size and pm.dims.hidden2 == 0
    obs_d = _dev(obs, cuda)
    store = torch.full((N, D), -7.0, device=cuda)
    a, lp, v = pm.act(obs_d, mode=2, actions=_dev(acts, cuda, torch.int64), obs_store=store)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.cpu().numpy(), acts)
    np.testing.assert_allclose(lp.cpu().numpy(), logp, atol=1e-5, rtol=0)
    np.testing.assert_allclose(v.cpu().numpy(), value, atol=1e-5, rtol=0)
    assert torch.equal(store, obs_d)
    vv = pm.predict_values(obs_d)
    assert torch.equal(vv.view(torch.int32), v.view(torch.int32))         # bit for bit
    # the rollout clock shifts the counter exactly as a larger rng_counter does
    clock = torch.tensor([7, 0], dtype=torch.int64, device=cuda)
    a1, lp1, _ = pm.act(obs_d, mode=0, rng_seed=99, rng_counter=5, clock=clock)
    a2, lp2, _ = pm.act(obs_d, mode=0, rng_seed=99, rng_counter=12)
    a3, _, _ = pm.act(obs_d, mode=0, rng_seed=99, rng_counter=5)
    assert torch.equal(a1, a2) and torch.equal(lp1.view(torch.int32), lp2.view(torch.int32))
    if N >= 256:
        assert not torch.equal(a1, a3)
    assert int(a1.min()) >= 0 and int(a1.max()) < A


def _mix64(x):
    """SplitMix64 finaliser on uint64 numpy arrays (csrc/gs_head.h mix64), wrapping arithmetic"""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def test_sampling_equals_the_two_layer_head_on_the_identity_extended_net(cuda):
    """Mode 0 draws the same counter-based uniform and inverts the same CDF as the two-hidden-layer
    gs_policy_act: on the net (D, H, H, A) with backbone.2 = I, bias 0 (relu(h1 I) = h1, the same
    function) both pick the same action on every row whose uniform lies more than 2e-5 from a CDF
    boundary (the rule of test_policy_sampling_inverse_cdf_rows).  Mode 1 is the oracle's argmax
    wherever the top two logits are more than 1e-5 apart."""
    from oracle import ppo_ref as R
    from gsamd.policy import DeviceMLPActorCritic
    D, H, A, n = 8, 64, 4, 4096
    rng = np.random.default_rng(11)
    p1 = _params(D, H, A, seed=21)
    flat1 = R.flatten(p1, (D, H, A))
    p2 = dict(p1)
    p2["backbone.2.weight"], p2["backbone.2.bias"] = np.eye(H, dtype=np.float32), np.zeros(H, np.float32)
    flat2 = R.flatten(p2, (D, H, H, A))
    obs = (2.0 * rng.standard_normal((n, D))).astype(np.float32)
    obs_d = _dev(obs, cuda)
    pm1 = _model(D, H, A, flat1, cuda)
    pm2 = DeviceMLPActorCritic(D, (H, H), A, device=cuda, init=False)
    pm2.load_flat(flat2)
    seed, ctr = 1234, 7
    a1 = pm1.act(obs_d, mode=0, rng_seed=seed, rng_counter=ctr)[0].cpu().numpy()
    a2 = pm2.act(obs_d, mode=0, rng_seed=seed, rng_counter=ctr)[0].cpu().numpy()
    lp = np.zeros((n, A), np.float32)
    for act in range(A):
        lp[:, act] = pm1.act(obs_d, mode=2, actions=torch.full((n,), act, device=cuda, dtype=torch.int64))[1].cpu().numpy()
    cdf = np.cumsum(np.exp(lp.astype(np.float64)), axis=1)
    with np.errstate(over="ignore"):
        h = _mix64(_mix64(_mix64(np.uint64(seed)) ^ np.uint64(ctr)) ^ np.arange(n, dtype=np.uint64))
    u = (h >> np.uint64(40)).astype(np.float64) / 16777216.0
    clear = np.abs(u[:, None] - cdf[:, :A - 1]).min(axis=1) > 2e-5
    assert (~clear).sum() <= n // 100, (~clear).sum()
    np.testing.assert_array_equal(a1[clear], a2[clear])
    want = np.minimum((u[:, None] >= cdf).sum(axis=1), A - 1)
    np.testing.assert_array_equal(a1[clear], want[clear])
    assert len(np.unique(a1)) == A
    # mode 1: first max wins
    logits, _, _ = R.forward(flat1, (D, H, A), obs)
    top = np.sort(logits, axis=1)
    sure = (top[:, -1] - top[:, -2]) > 1e-5
    assert (~sure).sum() <= n // 100
    a_det = pm1.act(obs_d, mode=1)[0].cpu().numpy()
    np.testing.assert_array_equal(a_det[sure], logits.argmax(axis=1)[sure])


# ------------------------------------------------------------------------------- update helpers
@functools.lru_cache(maxsize=None)
def _case(D, H, A, T, N, seed, self_logp=False):
    """A (T, N) rollout with plausible fields: old log-probs / values from a perturbed copy of the
    net (ratios straddle the clip range, value deltas the value clip range) — or, self_logp, from
    the net itself as a real rollout has them."""
    from oracle import ppo_ref as R
    rng = np.random.default_rng(seed)
    dims = (D, H, A)
    p0 = _flat(D, H, A, seed)
    obs = _obs(D, T * N, rng)
    actions = rng.integers(0, A, T * N)
    old = p0 if self_logp else (p0 + 0.08 * rng.standard_normal(p0.shape)).astype(np.float32)
    logits, value, _ = R.forward(old, dims, obs)
    old_logp = R.log_softmax(logits)[np.arange(T * N), actions].astype(np.float32)
    if not self_logp:       # one-hot / index observations move the perturbed net's logits little: spread the ratios
        old_logp = (old_logp + 0.15 * rng.standard_normal(T * N)).astype(np.float32)
    old_values = (value + 0.3 * rng.standard_normal(T * N)).astype(np.float32)
    adv = (0.5 + 2.0 * rng.standard_normal(T * N)).astype(np.float32)
    ret = (value + rng.standard_normal(T * N)).astype(np.float32)
    return dict(dims=dims, p0=p0, obs=obs, actions=actions, old_logp=old_logp, old_values=old_values, adv=adv,
                ret=ret, T=T, N=N)


def _rows(idx, T, N):
    """env-major sample indices i = env * T + t -> rows of the time-major (T, N) buffers"""
    idx = np.asarray(idx, np.int64)
    return (idx % T) * N + idx // T


class _Run:
    """Device buffers of one case and the C-ABI calls on them."""

    def __init__(self, case, cuda):
        from gsamd._lib import MlpDims, RolloutView, lib
        c, T, N = case, case["T"], case["N"]
        D, H, A = c["dims"]
        self.dims = MlpDims(D, H, 0, A)
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

    def update(self, idx, B, n, step0=0, use_graph=0, **hp):
        from gsamd._lib import GS_NUM_METRICS, check, lib
        ws = torch.zeros(int(lib.gs_ppo_update_workspace_bytes(self.dims, B, n)), dtype=torch.uint8, device=self.cuda)
        assert ws.numel() > 0
        met = torch.full((n, GS_NUM_METRICS), -3.0, device=self.cuda)
        idx_d = _dev(idx, self.cuda, torch.int32)
        check(lib.gs_ppo_update(self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                self.dims, self.hp(**hp), self.view, idx_d.data_ptr(), B, n, step0, met.data_ptr(),
                                self.stop.data_ptr(), ws.data_ptr(), ws.numel(), None, use_graph,
                                torch.cuda.current_stream().cuda_stream), "gs_ppo_update")
        torch.cuda.synchronize()
        return met.cpu().numpy()

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.params, self.m, self.v, self.grads)]


def _oracle_step(case, p, m, v, rows, t, lr=LR):
    from oracle import ppo_ref as R
    c = case
    loss, met, g = R.ppo_loss_and_grads(p, c["dims"], c["obs"][rows], c["actions"][rows], c["old_logp"][rows],
                                        c["old_values"][rows], c["adv"][rows], c["ret"][rows], **HP)
    gc, total = R.clip_grad_norm(g, c["dims"], MAX_NORM)
    p1, m1, v1 = R.adam_step(p, gc, m, v, t, lr)
    return loss, met, g, gc, total, p1, m1, v1


# ------------------------------------------------------------------------------- one minibatch
@pytest.mark.parametrize("D,H,A,B", [(1, 64, 4, 64), (16, 64, 4, 64), (9, 64, 6, 64), (5, 16, 3, 64), (5, 16, 3, 48)])
def test_one_minibatch_vs_numpy_oracle(cuda, D, H, A, B):
    from oracle import ppo_ref as R
    from gsamd._lib import ACT_SLOT, GS_HP_ACT_STATS, GS_NUM_METRICS, M, check, lib
    from gsamd.metrics import activation_stats
    T, N = 3, 40
    case = _case(D, H, A, T, N, seed=100 + D + B)
    rng = np.random.default_rng(B + D)
    idx = rng.permutation(T * N)[:B]
    rows = _rows(idx, T, N)
    zeros = np.zeros_like(case["p0"])
    loss, met, g, gc, total, p1, _, _ = _oracle_step(case, case["p0"], zeros, zeros, rows, 1)
    assert 0 < met["opt/ppo/clip_fraction"] < 1 and 0 < met["opt/ppo/clip_fraction_vf"] < 1      # both ranges straddled
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
    print("loss", rec[0], loss, "norm", rec[M["grad_norm"]], total)
    np.testing.assert_allclose(rec[M["loss"]], loss, rtol=1e-5, atol=1e-6)
    assert np.array_equal(rec0[:12], rec[:12])                   # gs_ppo_loss: the same steps 1-3
    assert rec0[M["grad_norm"]] == 0 and not rec0[ACT_SLOT:].any()
    for key, slot in [("opt/loss/policy", "policy_loss"), ("opt/loss/value", "value_loss"),
                      ("opt/policy/entropy", "entropy"), ("opt/ppo/clip_fraction", "clip_fraction"),
                      ("opt/ppo/clip_fraction_vf", "clip_fraction_vf"), ("opt/value/explained_var", "explained_var"),
                      ("opt/ppo/kl", "kl"), ("opt/ppo/approx_kl", "approx_kl"), ("roll/adv/norm/std", "adv_norm_std")]:
        np.testing.assert_allclose(rec[M[slot]], met[key], atol=2e-6, rtol=1e-5, err_msg=key)
    assert rec[M["kl_stop"]] == rec[M["skipped"]] == rec[M["unevaluated"]] == 0
    np.testing.assert_allclose(run.grads.cpu().numpy(), gc, atol=1e-6 * max(1, np.abs(gc).max()), rtol=0)
    np.testing.assert_allclose(run.params.cpu().numpy(), p1, atol=5e-6, rtol=0)
    # pre-clip norms: the total and the three components; GS_M_GN_MLP is 0
    G = R.unflatten(g, case["dims"])
    comp = {c: np.sqrt(sum(float((G[k].astype(np.float64) ** 2).sum()) for k in G if k.startswith(c)))
            for c in ("backbone", "policy_head", "value_head")}
    np.testing.assert_allclose(rec[M["grad_norm"]], total, rtol=1e-5)
    for c in comp:
        np.testing.assert_allclose(rec[M[f"gn_{c}"]], comp[c], rtol=2e-5, err_msg=c)
    assert rec[M["gn_mlp"]] == 0
    # GS_HP_ACT_STATS: backbone.0's slots; the other layers' stay 0
    want = R.activation_stats(case["p0"], case["dims"], case["obs"][rows])
    got = rec[ACT_SLOT:ACT_SLOT + 4]
    for j in (0, 1):
        assert abs(got[j] - want[j]) <= 1e-5 * (1 + abs(want[j])), (j, got[j], want[j])
    for j in (2, 3):
        assert abs(got[j] - want[j]) <= 1.0 / B, (j, got[j], want[j])
    assert not rec[ACT_SLOT + 4:].any()
    # gs_mlp_activation_stats: the layer-0 part in its documented format, the layer-1 part zero
    nparts = (B + 15) // 16
    parts = torch.full((nparts, 2, 2 + H), -1.0, dtype=torch.float64, device=cuda)
    run.reset(case["p0"])
    check(lib.gs_mlp_activation_stats(run.params.data_ptr(), run.dims, run.view, idx_d.data_ptr(), B, parts.data_ptr(),
                                      s), "gs_mlp_activation_stats")
    torch.cuda.synchronize()
    parts = parts.cpu().numpy()
    assert not parts[:, 1].any()
    st = activation_stats(parts.reshape(nparts, -1), B, (H,))
    assert set(st) == {f"opt/activations/backbone.0/{k}" for k in ("mean", "std", "dead_pct", "dead_max")}
    for j, k in enumerate(("mean", "std")):
        assert abs(st[f"opt/activations/backbone.0/{k}"] - want[j]) <= 1e-5 * (1 + abs(want[j]))
    for j, k in ((2, "dead_pct"), (3, "dead_max")):
        assert abs(st[f"opt/activations/backbone.0/{k}"] - want[j]) <= 1.0 / B


# ------------------------------------------------------------------------------- eight minibatches, one launch
def test_eight_minibatches_in_one_launch(cuda):
    from gsamd._lib import M
    D, H, A, B, n = 1, 64, 4, 64, 8
    T, N = 16, 32
    case = _case(D, H, A, T, N, seed=77)
    idx = np.random.default_rng(5).permutation(T * N)
    assert idx.size == n * B
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    losses = []
    for k in range(n):
        loss, _, _, gc, _, p, m, v = _oracle_step(case, p, m, v, _rows(idx[k * B:(k + 1) * B], T, N), k + 1)
        losses.append(loss)
    run = _Run(case, cuda)
    rec = run.update(idx, B, n)
    full = run.state()
    print("losses", rec[:, 0], losses)
    np.testing.assert_allclose(rec[:, M["loss"]], losses, rtol=1e-5, atol=0)
    pd, pr = full[0].astype(np.float64), p.astype(np.float64)
    print("params rel L2", np.linalg.norm(pd - pr) / np.linalg.norm(pr), "max abs", np.abs(pd - pr).max())
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5
    assert np.abs(pd - pr).max() < 1e-3
    assert not rec[:, [M["kl_stop"], M["skipped"], M["unevaluated"]]].any()
    assert run.stop.item() == 0
    # twice: byte-identical parameters, moments, gradient and records (use_graph is accepted and ignored)
    run.reset(case["p0"])
    rec2 = run.update(idx, B, n, use_graph=1)
    for a, b in zip(full + [rec], run.state() + [rec2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # split 3 + 5 with adam_step0 = 3: the LDS-resident state's write-back and reload are exact
    run.reset(case["p0"])
    rec_a = run.update(idx[:3 * B], B, 3)
    rec_b = run.update(idx[3 * B:], B, 5, step0=3)
    for a, b in zip(full + [rec], run.state() + [np.concatenate([rec_a, rec_b])]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------- KL early stop
def test_kl_early_stop(cuda):
    from gsamd._lib import GS_NUM_METRICS, M
    D, H, A, B, n = 1, 64, 4, 64, 8
    T, N = 16, 32
    lr = 1e-2
    case = _case(D, H, A, T, N, seed=78, self_logp=True)
    idx = np.random.default_rng(6).permutation(T * N)
    p, m, v = case["p0"], np.zeros_like(case["p0"]), np.zeros_like(case["p0"])
    akl, losses, ps = [], [], []
    for k in range(n):
        ps.append(p)
        loss, met, _, _, _, p, m, v = _oracle_step(case, p, m, v, _rows(idx[k * B:(k + 1) * B], T, N), k + 1, lr=lr)
        akl.append(met["opt/ppo/approx_kl"])
        losses.append(loss)
    akl = np.asarray(akl)
    target = 0.5 * float(akl[1:].max())
    kstar = int(np.argmax(akl > target))
    print("approx_kl", akl, "target", target, "k*", kstar)
    assert 1 <= kstar < n
    assert (np.abs(akl[:kstar + 1] - target) > 1e-3 * target).all()      # no step sits on the threshold
    run = _Run(case, cuda)
    rec = run.update(idx, B, n, lr=lr, target_kl=target)
    flags = [M["kl_stop"], M["skipped"], M["unevaluated"]]
    assert not rec[:kstar, flags].any()
    np.testing.assert_allclose(rec[:kstar + 1, M["loss"]], losses[:kstar + 1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rec[:kstar + 1, M["approx_kl"]], akl[:kstar + 1], rtol=1e-4, atol=2e-6)
    assert rec[kstar, M["kl_stop"]] == 1 and rec[kstar, M["skipped"]] == 1 and rec[kstar, M["unevaluated"]] == 0
    later = np.zeros(GS_NUM_METRICS, np.float32)
    later[flags] = 1
    assert kstar + 1 < n and all(np.array_equal(r, later) for r in rec[kstar + 1:])
    assert run.stop.item() == 1
    stopped = run.state()
    # the parameters are those after k* steps: byte-identical to k* steps without a target
    plain = _Run(case, cuda)
    plain.update(idx[:kstar * B], B, kstar, lr=lr)
    for a, b in zip(stopped, plain.state()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pd, pr = stopped[0].astype(np.float64), ps[kstar].astype(np.float64)
    assert np.linalg.norm(pd - pr) / np.linalg.norm(pr) < 1e-5
    # sticky: with the flag still set the next call evaluates nothing and moves nothing
    rec3 = run.update(idx, B, 2, step0=kstar, lr=lr, target_kl=target)
    assert all(np.array_equal(r, later) for r in rec3)
    for a, b in zip(stopped, run.state()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # target_kl unset: the flag is neither read nor written
    rec4 = run.update(idx, B, 2, step0=kstar, lr=lr)
    assert not rec4[:, flags].any() and run.stop.item() == 1


# ------------------------------------------------------------------------------- refusals
def test_refusals(cuda):
    from gsamd._lib import GS_ENV_CARTPOLE, GS_HP_BF16, GS_NUM_METRICS, MlpDims, PPOGlobal, check, lib
    case = _case(1, 64, 4, 16, 32, seed=77)
    run = _Run(case, cuda)
    idx = np.arange(128)
    with pytest.raises(ValueError, match="one hidden layer"):
        run.update(idx, 64, 2, flags=GS_HP_BF16)
    s = torch.cuda.current_stream().cuda_stream
    met = torch.zeros(2, GS_NUM_METRICS, device=cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    idx_d = _dev(idx, cuda, torch.int32)
    with pytest.raises(ValueError, match="one hidden layer"):
        check(lib.gs_ppo_stage(0, run.params.data_ptr(), run.grads.data_ptr(), run.m.data_ptr(), run.v.data_ptr(),
                               run.dims, run.hp(), run.view, idx_d.data_ptr(), 64, 1, met.data_ptr(), ws.data_ptr(), s),
              "gs_ppo_stage")
    sums = torch.zeros(2, 14, dtype=torch.float64, device=cuda)
    stats = torch.zeros(2, 2, device=cuda)
    glob = PPOGlobal(64, stats.data_ptr(), sums.data_ptr())
    with pytest.raises(ValueError, match="one hidden layer"):
        check(lib.gs_ppo_update_global(run.params.data_ptr(), run.grads.data_ptr(), run.m.data_ptr(),
                                       run.v.data_ptr(), run.dims, run.hp(), run.view, idx_d.data_ptr(), 64, 2, 0,
                                       met.data_ptr(), run.stop.data_ptr(), ws.data_ptr(), ws.numel(), None, 0,
                                       ctypes.byref(glob), s), "gs_ppo_update_global")
    # a shape whose optimizer state does not fit in LDS: refused with the byte counts
    big = MlpDims(64, 1024, 0, 4)
    with pytest.raises(ValueError, match=r"one hidden layer.*bytes"):
        check(lib.gs_ppo_update(run.params.data_ptr(), run.grads.data_ptr(), run.m.data_ptr(), run.v.data_ptr(), big,
                                run.hp(), run.view, idx_d.data_ptr(), 64, 2, 0, met.data_ptr(), run.stop.data_ptr(),
                                ws.data_ptr(), ws.numel(), None, 0, s), "gs_ppo_update")
    v = ctypes.c_int(5)
    check(lib.gs_rollout_env_supported(run.dims, GS_ENV_CARTPOLE, ctypes.byref(v)), "gs_rollout_env_supported")
    assert v.value == 0
    # nothing above ran a kernel on the buffers
    torch.cuda.synchronize()
    assert np.array_equal(run.params.cpu().numpy(), case["p0"])
