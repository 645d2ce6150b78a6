"""A float64 restatement of one masked-MLP PPO step (the twin of loss_row_masked / head_act_row_masked
in csrc/gs_head.h and of the reference's MLPActorCritic(valid_actions=...), utils/models.py:285-346):
torch autograd on CPU over oracle.ppo_ref's parameter layout (unflatten) and forward, restated in
float64 with the invalid logits filled with -inf, oracle.cnn_ref.dist_terms for the
(Masked)Categorical's log-prob and entropy, the PPO terms as oracle.cnn_ref.loss_and_grads writes
them, then oracle.ppo_ref.clip_grad_norm / adam_step.  The parameters and the batch are the float32
values the device holds, cast up; nothing here reads a device result.

Also the cases of tests/test_gpu_masked_mlp.py: tests/mlp_cases.case's recipe with the recorded
actions drawn from the valid set and the old log-probs taken under the mask."""
import functools
import os

import numpy as np
import torch

import mlp_cases as C
from mlp_cases import HP, LR, MAX_NORM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_mlp.npz")
FIXTURE_DIMS = {"small": (12, 128, 128, 18), "tiny": (12, 64, 18)}
FIXTURE_HP = dict(clip=0.2, clip_vf=0.2, vf_coef=0.5, ent_coef=0.01)       # make_masked_mlp_golden.HP


def mask_of(valid):
    m = 0
    for a in valid:
        m |= 1 << int(a)
    return m


def _tensors(p, dims, grad=False):
    from oracle import ppo_ref as R
    return {k: torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(grad)
            for k, v in R.unflatten(p, dims).items()}


def forward(P, dims, obs, valid):
    """oracle.ppo_ref.forward on float64 tensors -> (logits with -inf at the invalid actions, value)"""
    x = torch.as_tensor(np.asarray(obs, np.float64))
    for i in range(len(dims) - 2):
        x = torch.relu(x @ P[f"backbone.{2 * i}.weight"].T + P[f"backbone.{2 * i}.bias"])
    logits = x @ P["policy_head.weight"].T + P["policy_head.bias"]
    if valid is not None:
        mask = torch.ones_like(logits, dtype=torch.bool)
        mask[:, list(valid)] = False
        logits = logits.masked_fill(mask, float("-inf"))
    value = (x @ P["value_head.weight"].T + P["value_head.bias"])[:, 0]
    return logits, value


def loss_and_grads(p, dims, valid, obs, actions, old_logp, old_values, adv, ret, *, clip, clip_vf, vf_coef, ent_coef,
                   normalize=True):
    """-> (loss, metrics, flat float64 gradient, per-row log-probs, per-row entropies)"""
    from oracle import cnn_ref as CR
    from oracle import ppo_ref as R
    P = _tensors(p, dims, grad=True)
    f64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    adv, old_logp, old_values, ret = f64(adv), f64(old_logp), f64(old_values), f64(ret)
    met = {}
    if normalize:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        met["roll/adv/norm/mean"], met["roll/adv/norm/std"] = float(adv.mean()), float(adv.std())
    logits, value = forward(P, dims, obs, valid)
    lp, H = CR.dist_terms(logits, np.asarray(actions), valid)
    ratio = torch.exp(lp - old_logp)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    vdelta = value - old_values
    vl = torch.max((value - ret) ** 2, (old_values + torch.clamp(vdelta, -clip_vf, clip_vf) - ret) ** 2).mean()
    ent = H.mean()
    loss = pl + vf_coef * vl + ent_coef * (-ent)
    loss.backward()
    g = np.concatenate([P[n].grad.reshape(-1).numpy() for n, _ in R.param_shapes(dims)])
    with torch.no_grad():
        r2 = torch.exp(torch.clamp(lp - old_logp, -20.0, 20.0))
        met.update({
            "opt/loss/total": float(loss), "opt/loss/policy": float(pl), "opt/policy/entropy": float(ent),
            "opt/loss/value": float(vl),
            "opt/ppo/clip_fraction": float(((ratio < 1 - clip) | (ratio > 1 + clip)).double().mean()),
            "opt/ppo/clip_fraction_vf": float(((vdelta < -clip_vf) | (vdelta > clip_vf)).double().mean()),
            "opt/value/explained_var": float(1 - torch.var(ret - value) / torch.var(ret)),
            "opt/ppo/kl": float((old_logp - lp).mean()),
            "opt/ppo/approx_kl": float(((r2 - 1) - torch.log(r2)).mean()),
        })
    return float(loss.detach()), met, g, lp.detach().numpy(), H.detach().numpy()


def step(case, p, m, v, rows, t, lr=LR, hp=HP):
    """One minibatch step on rows of a case from the float32 state (p, m, v): the float64 loss and
    gradient, then the oracle's clip and Adam -> (loss, metrics, g, gc, total, p1, m1, v1)"""
    from oracle import ppo_ref as R
    c = case
    loss, met, g, _, _ = loss_and_grads(p, c["dims"], c["valid"], c["obs"][rows], c["actions"][rows], c["old_logp"][rows],
                                        c["old_values"][rows], c["adv"][rows], c["ret"][rows], **hp)
    gc, total = R.clip_grad_norm(g, c["dims"], MAX_NORM)
    p1, m1, v1 = R.adam_step(np.asarray(p, np.float32), gc, m, v, t, lr)
    return loss, met, g, gc, total, p1, m1, v1


def act(p, dims, valid, obs):
    """-> (values, log-softmax over the valid actions (-inf elsewhere), the first maximum among them)"""
    with torch.no_grad():
        logits, value = forward(_tensors(p, dims), dims, obs, valid)
        ln = (logits - torch.logsumexp(logits, dim=-1, keepdim=True)).numpy()
    return value.numpy(), ln, ln.argmax(axis=1)


def sample(ln, valid, u):
    """The inverse CDF over the valid actions in index order at the uniforms u (the fallback is the last
    valid action) -> (actions, each row's distance from u to the nearest CDF boundary)"""
    valid = sorted(valid)
    cdf = np.cumsum(np.exp(ln[:, valid]), axis=1)
    k = (u[:, None] >= cdf).sum(axis=1)
    actions = np.asarray(valid)[np.minimum(k, len(valid) - 1)]
    return actions, np.abs(cdf[:, :-1] - u[:, None]).min(axis=1) if len(valid) > 1 else np.ones_like(u)


@functools.lru_cache(maxsize=None)
def case(dims, valid, T, N, seed):
    """tests/mlp_cases.case under a mask: the same draws in the same order, the recorded actions drawn
    from the valid set, the old log-probs the perturbed net's log-softmax over the valid actions."""
    rng = np.random.default_rng(seed)
    D = dims[0]
    p0 = C.flat(dims, seed)
    obs = rng.standard_normal((T * N, D)).astype(np.float32)
    actions = np.asarray(valid)[rng.integers(0, len(valid), T * N)]
    old = (p0 + 0.08 * rng.standard_normal(p0.shape)).astype(np.float32)
    value, ln, _ = act(old, dims, valid, obs)
    old_logp = (ln[np.arange(T * N), actions] + 0.15 * rng.standard_normal(T * N)).astype(np.float32)
    old_values = (value + 0.3 * rng.standard_normal(T * N)).astype(np.float32)
    adv = (0.5 + 2.0 * rng.standard_normal(T * N)).astype(np.float32)
    ret = (value + rng.standard_normal(T * N)).astype(np.float32)
    return dict(dims=dims, valid=tuple(valid), p0=p0, obs=obs, actions=actions, old_logp=old_logp,
                old_values=old_values, adv=adv, ret=ret, T=T, N=N)


def conditions_met(c, p, rows, met):
    """The input conditions of one twin step (no device value involved): both clip fractions strictly
    inside (0, 1), no pre-activation within 1e-6 of a ReLU flip, every recorded action valid."""
    return (0 < met["opt/ppo/clip_fraction"] < 1 and 0 < met["opt/ppo/clip_fraction_vf"] < 1 and
            min(C.preact_margins(p, c["dims"], c["obs"][rows])) >= 1e-6 and
            set(np.unique(c["actions"][rows]).tolist()) <= set(c["valid"]))


def invalid_slices(dims, valid):
    """The flat-parameter index ranges of the invalid actions' policy-head rows and biases"""
    from oracle import ppo_ref as R
    A, HK = dims[-1], dims[-2]
    o = 0
    for name, shp in R.param_shapes(dims):
        if name == "policy_head.weight":
            ow = o
        if name == "policy_head.bias":
            ob = o
        o += int(np.prod(shp))
    idx = [np.arange(ow + a * HK, ow + (a + 1) * HK) for a in range(A) if a not in valid]
    idx += [np.array([ob + a]) for a in range(A) if a not in valid]
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def fixture(tag):
    """tests/golden/masked_mlp.npz's case `tag`: dims, the flat parameters, the batch and the records"""
    from oracle import ppo_ref as R
    z = np.load(GOLDEN)
    dims = FIXTURE_DIMS[tag]
    sd = {k[len(tag) + 7:]: z[k] for k in z.files if k.startswith(f"{tag}/state/")}
    out = dict(dims=dims, valid=tuple(int(a) for a in z["valid"]), p0=R.flatten(sd, dims), state=sd)
    for k in z.files:
        if k.startswith(f"{tag}/") and "/state/" not in k:
            out[k[len(tag) + 1:]] = z[k]
    return out
