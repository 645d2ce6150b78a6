"""Cases for the parity tests of the two-hidden-layer MLP kernels (tests/test_gpu_mlp2_shapes.py):
the case generator of tests/test_gpu_mlp1.py for dims = (D, H1, H2, A), the numpy-oracle step, and
the input conditions a case has to meet before a tolerance may be trusted.  numpy only."""
import functools

import numpy as np

HP = dict(clip=0.2, clip_vf=0.2, vf_coef=0.5, ent_coef=0.01)
MAX_NORM, LR = 0.5, 3e-4


def params(dims, seed):
    """A random net with O(1) logit gaps (the reference's 0.01-gain policy head would leave every
    row near uniform)."""
    from oracle import ppo_ref as R
    rng = np.random.default_rng(seed)
    out = {}
    for name, shp in R.param_shapes(dims):
        if name.endswith("bias"):
            out[name] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
        else:
            scale = (1.0 if name.startswith("policy") else 0.5) / np.sqrt(shp[-1])
            out[name] = (scale * rng.standard_normal(shp)).astype(np.float32)
    return out


def flat(dims, seed):
    from oracle import ppo_ref as R
    return R.flatten(params(dims, seed), dims)


@functools.lru_cache(maxsize=None)
def case(dims, T, N, seed, self_logp=False):
    """A (T, N) rollout of N(0, 1) observations with plausible fields: old log-probs / values from
    a perturbed copy of the net (ratios straddle the clip range, value deltas the value clip
    range) — or, self_logp, from the net itself as a real rollout has them."""
    from oracle import ppo_ref as R
    rng = np.random.default_rng(seed)
    D, A = dims[0], dims[-1]
    p0 = flat(dims, seed)
    obs = rng.standard_normal((T * N, D)).astype(np.float32)
    actions = rng.integers(0, A, T * N)
    old = p0 if self_logp else (p0 + 0.08 * rng.standard_normal(p0.shape)).astype(np.float32)
    logits, value, _ = R.forward(old, dims, obs)
    old_logp = R.log_softmax(logits)[np.arange(T * N), actions].astype(np.float32)
    if not self_logp:
        old_logp = (old_logp + 0.15 * rng.standard_normal(T * N)).astype(np.float32)
    old_values = (value + 0.3 * rng.standard_normal(T * N)).astype(np.float32)
    adv = (0.5 + 2.0 * rng.standard_normal(T * N)).astype(np.float32)
    ret = (value + rng.standard_normal(T * N)).astype(np.float32)
    return dict(dims=dims, p0=p0, obs=obs, actions=actions, old_logp=old_logp, old_values=old_values, adv=adv,
                ret=ret, T=T, N=N)


def rows(idx, T, N):
    """env-major sample indices i = env * T + t -> rows of the time-major (T, N) buffers"""
    idx = np.asarray(idx, np.int64)
    return (idx % T) * N + idx // T


def oracle_step(c, p, m, v, rws, t, lr=LR, dtype=np.float32):
    """One minibatch step of the oracle on rows rws of case c: loss, metrics, gradient, clipped
    gradient, pre-clip norm and the Adam step (float32 throughout, as the reference runs it)."""
    from oracle import ppo_ref as R
    loss, met, g = R.ppo_loss_and_grads(p, c["dims"], c["obs"][rws], c["actions"][rws], c["old_logp"][rws],
                                        c["old_values"][rws], c["adv"][rws], c["ret"][rws], **HP)
    gc, total = R.clip_grad_norm(g, c["dims"], MAX_NORM)
    p1, m1, v1 = R.adam_step(p, gc, m, v, t, lr)
    return loss, met, g, gc, total, p1, m1, v1


def grads_f64(c, rws):
    """The oracle's unclipped gradient of case c's rows evaluated in float64: the oracle's own
    formulas (its float32 casts rebound to float64 for the call) on the float32 inputs cast up."""
    from oracle import ppo_ref as R
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    saved = R.F32
    R.F32 = np.float64
    try:
        _, _, g = R.ppo_loss_and_grads(f64(c["p0"]), c["dims"], f64(c["obs"][rws]), c["actions"][rws],
                                       f64(c["old_logp"][rws]), f64(c["old_values"][rws]), f64(c["adv"][rws]),
                                       f64(c["ret"][rws]), **HP)
    finally:
        R.F32 = saved
    return g


def preact_margins(p, dims, obs):
    """Per hidden layer the smallest |z| / (sum of |terms| of z) over the batch's pre-activations,
    in float64: how far the nearest pre-activation is from a ReLU flip, relative to the size of
    the terms whose float32 summation order differs between the oracle and a kernel."""
    from oracle import ppo_ref as R
    P = R.unflatten(p, dims)
    x = np.asarray(obs, np.float64)
    out = []
    for i in range(len(dims) - 2):
        W = P[f"backbone.{2 * i}.weight"].astype(np.float64)
        b = P[f"backbone.{2 * i}.bias"].astype(np.float64)
        z = x @ W.T + b
        mag = np.abs(x) @ np.abs(W).T + np.abs(b)
        out.append(float((np.abs(z) / mag).min()))
        x = np.maximum(z, 0.0)
    return out


def mix64(x):
    """SplitMix64 finaliser on uint64 numpy arrays (csrc/gs_head.h mix64), wrapping arithmetic"""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniforms(seed, ctr, n):
    """The rows' counter-based uniforms of gs_policy_act's mode 0 (csrc/gs_head.h head_act_row)"""
    with np.errstate(over="ignore"):
        h = mix64(mix64(mix64(np.uint64(seed)) ^ np.uint64(ctr)) ^ np.arange(n, dtype=np.uint64))
    return (h >> np.uint64(40)).astype(np.float64) / 16777216.0
