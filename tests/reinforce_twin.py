"""Plain numpy / torch-CPU restatement of the reference's REINFORCE path, for the CPU tests (against
tests/golden/reinforce.npz) and as the GPU tests' entry-for-entry reference where the fixture keeps only
samples.  The loss and the steps run the same torch ops as the reference's model, so on a CPU they
reproduce the fixture bit for bit: a restatement, not an independent summation order (adam_steps'
dtype=torch.float64 is the independent evaluation):

  mc_returns / episode_returns / valid_index_map    utils/returns_advantages.py:19-113
  targets                                           utils/rollout_collector.py:385-457 (mc:* branch)
  loss_and_grads / adam_steps                       agents/reinforce/reinforce_agent.py:11-88 +
                                                    agents/base_agent.py:591-621 (clip_grad_norm_, Adam)
Nothing here imports the reference or the device library.
"""
from __future__ import annotations

import numpy as np
import torch

PARAM_NAMES = ("backbone.0.weight", "backbone.0.bias", "backbone.2.weight", "backbone.2.bias",
               "policy_head.weight", "policy_head.bias", "value_head.weight", "value_head.bias")


def terminal_mask(dones, timeouts=None):
    d = np.asarray(dones).astype(bool)
    if timeouts is None:            # mc_treat_timeouts_as_terminals=True: every done cuts the return
        return d
    return d & ~np.asarray(timeouts).astype(bool)


def mc_returns(rewards, dones, timeouts, gamma):
    """float32 loop acc = r[t] + f32(gamma) * (acc * nt[t]): three roundings per step, no FMA."""
    rewards = np.asarray(rewards, np.float32)
    T, N = rewards.shape
    nt = (~terminal_mask(dones, timeouts)).astype(np.float32)
    g = np.float32(gamma)
    out = np.zeros((T, N), np.float32)
    acc = np.zeros(N, np.float32)
    for t in range(T - 1, -1, -1):
        acc = (rewards[t] + (g * (acc * nt[t]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        out[t] = acc
    return out


def episode_returns(returns, dones, timeouts):
    """Every step of an episode segment takes the segment's first reward-to-go."""
    term = terminal_mask(dones, timeouts)
    out = np.array(returns, np.float32, copy=True)
    T, N = out.shape
    for j in range(N):
        seg = out[0, j]
        for t in range(T):
            nxt = out[t + 1, j] if (term[t, j] and t + 1 < T) else seg
            out[t, j] = seg
            seg = nxt
    return out


def valid_index_map(dones, timeouts):
    """(last_terminal (N,), idx_map (N*T,) env-major or identity when nothing is valid, valid mask)."""
    term = terminal_mask(dones, timeouts)
    T, N = term.shape
    last = np.full(N, -1, np.int32)
    for j in range(N):
        w = np.flatnonzero(term[:, j])
        if w.size:
            last[j] = w[-1]
    valid = (np.arange(T)[None, :] <= last[:, None]).reshape(-1)      # env-major
    n = N * T
    if not valid.any():
        return last, np.arange(n, dtype=np.int32), valid
    cur = np.where(valid, np.arange(n), -1)
    filled = np.maximum.accumulate(cur)
    filled[filled < 0] = int(np.argmax(valid))
    return last, filled.astype(np.int32), valid


class BaseStats:
    """utils/rollout_stats.py RunningStats on Python floats."""

    def __init__(self):
        self.count, self.sum, self.sum_squared = 0, 0.0, 0.0

    def update(self, count, s, sq):
        self.count += int(count)
        self.sum += float(s)
        self.sum_squared += float(sq)

    def mean(self):
        return self.sum / self.count if self.count else 0.0

    def std(self):
        if not self.count:
            return 0.0
        m = self.mean()
        return float(np.sqrt(max(0.0, self.sum_squared / self.count - m * m)))


def normalize_rollout(x, eps=1e-8):
    x = np.asarray(x, np.float32)
    f = x.reshape(-1)
    return ((x - f.mean()) / (f.std() + np.float32(eps))).astype(np.float32)


def targets(rewards, dones, timeouts, gamma, kind, base: BaseStats, normalize_returns=False,
            normalize_advantages=False):
    """The collector's mc:* branch -> (advantages, returns, idx_map, last_terminal)."""
    ret = mc_returns(rewards, dones, timeouts, gamma)
    if kind == "mc:episode":
        ret = episode_returns(ret, dones, timeouts)
    last, idx_map, valid = valid_index_map(dones, timeouts)
    if valid.any():
        v = ret.T.reshape(-1)[valid].astype(np.float64)
        base.update(v.size, v.sum(), (v * v).sum())
    adv = (ret - np.float32(base.mean())).astype(np.float32)
    if normalize_returns:
        ret = normalize_rollout(ret)
    if normalize_advantages:
        adv = normalize_rollout(adv)
    return adv, ret, idx_map, last


# ---- model, loss, step --------------------------------------------------------------------------
def shapes(D, H1, H2, A):
    return ((H1, D), (H1,), (H2, H1), (H2,), (A, H2), (A,), (1, H2), (1,))


def unflatten(flat, D, H1, H2, A):
    out, o = [], 0
    flat = torch.as_tensor(flat, dtype=torch.float32)
    for shp in shapes(D, H1, H2, A):
        n = int(np.prod(shp))
        out.append(flat[o:o + n].reshape(shp).clone())
        o += n
    assert o == flat.numel()
    return out


def n_params(D, H1, H2, A):
    return sum(int(np.prod(s)) for s in shapes(D, H1, H2, A))


def loss_and_grads(flat, dims, obs, actions, old_logp, t, ent_coef, normalize):
    """-> (record dict, flat gradient with zeros on the value head).  obs (B, D), t (B,)."""
    D, H1, H2, A = dims
    ps = [p.requires_grad_(True) for p in unflatten(flat, *dims)]
    W1, b1, W2, b2, Wp, bp, Wv, bv = ps
    obs = torch.as_tensor(obs, dtype=torch.float32)
    t = torch.as_tensor(t, dtype=torch.float32)
    rec = {}
    if normalize:
        t = (t - t.mean()) / (t.std() + 1e-8)
        rec["norm_mean"], rec["norm_std"] = float(t.mean()), float(t.std())
    h = torch.relu(torch.relu(obs @ W1.T + b1) @ W2.T + b2)
    dist = torch.distributions.Categorical(logits=h @ Wp.T + bp)
    logp = dist.log_prob(torch.as_tensor(actions, dtype=torch.int64))
    policy_loss = -(logp * t).mean()
    entropy = dist.entropy().mean()
    loss = policy_loss + ent_coef * (-entropy)
    loss.backward()
    old = torch.as_tensor(old_logp, dtype=torch.float32)
    with torch.no_grad():
        ratio = torch.exp(torch.clamp(logp - old, -20.0, 20.0))
        rec.update(loss=float(loss), policy_loss=float(policy_loss), entropy=float(entropy),
                   kl=float((old - logp).mean()), approx_kl=float(((ratio - 1) - torch.log(ratio)).mean()),
                   target_mean=float(t.mean()), target_std=float(t.std()))
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]
    g = torch.cat([x.reshape(-1) for x in grads]).numpy()
    nb = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads[:4])))
    npol = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads[4:6])))
    rec.update(gn_backbone=nb, gn_policy_head=npol, grad_norm=float(np.hypot(nb, npol)))
    return rec, g


def adam_steps(flat, dims, batches, lr, ent_coef, normalize, max_grad_norm=0.5, m0=None, v0=None, step0=0,
               dtype=torch.float32):
    """clip_grad_norm_ + torch.optim.Adam over `batches` [(obs, actions, old_logp, t), ...]; the value
    head has no gradient and is skipped by both.  m0 / v0: starting moments of the trained tensors
    (flat, value-head slice ignored).  dtype=torch.float64 evaluates the same float32 inputs in double
    (what the reference's own rounding is measured against).  -> flat parameters after the steps."""
    ps = [torch.nn.Parameter(p.to(dtype)) for p in unflatten(flat, *dims)]
    opt = torch.optim.Adam(ps, lr=lr)
    if m0 is not None:
        ms, vs = unflatten(m0, *dims), unflatten(v0, *dims)
        for p, m, v in list(zip(ps, ms, vs))[:6]:
            opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m.to(dtype), "exp_avg_sq": v.to(dtype)}
    W1, b1, W2, b2, Wp, bp, Wv, bv = ps
    for obs, actions, old_logp, t in batches:
        obs = torch.as_tensor(obs, dtype=torch.float32).to(dtype)
        t = torch.as_tensor(t, dtype=torch.float32).to(dtype)
        if normalize:
            t = (t - t.mean()) / (t.std() + 1e-8)
        h = torch.relu(torch.relu(obs @ W1.T + b1) @ W2.T + b2)
        dist = torch.distributions.Categorical(logits=h @ Wp.T + bp)
        loss = -(dist.log_prob(torch.as_tensor(actions, dtype=torch.int64)) * t).mean() - ent_coef * dist.entropy().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if max_grad_norm and max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in ps]).numpy()


# ---- deterministic case construction shared by the fixture generator and the tests ---------------
LOSS_SHAPES = {"small42": (4, 128, 128, 2), "small1010": (10, 128, 128, 10), "medium42": (4, 256, 256, 2)}
POOLS = {"small42": "d4a2", "small1010": "d10a10", "medium42": "d4a2"}      # the rollout a shape trains on
POOL_T, POOL_N = 64, 32


def loss_cases():
    """(tag, shape, B, normalise, ent_coef): mlp_small at (D, A) = (4, 2) and (10, 10) over B in
    {2, 48, 2048} x {raw, batch-normalised returns} x ent_coef in {0, 0.01}; one mlp_medium case."""
    out = []
    for shape in ("small42", "small1010"):
        for B in (2, 48, 2048):
            for norm in (False, True):
                for ent in (0.0, 0.01):
                    out.append((f"{shape}_B{B}_{'norm' if norm else 'raw'}_ent{ent:g}", shape, B, norm, ent))
    out.append(("medium42_B2048_norm_ent0.01", "medium42", 2048, True, 0.01))
    return out


def hash_params(P, salt=1, scale=0.2):
    """P float32 parameters in [-scale/2, scale/2) from an integer hash: exact arithmetic, so the
    generator and every test machine build the same bits without storing them."""
    i = np.arange(P, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    return ((h.astype(np.float64) / float(1 << 32) - 0.5) * scale).astype(np.float32)


def sample_positions(P, n=1024):
    """The gradient / parameter entries a fixture keeps: n positions spread over the flat vector."""
    return np.unique(np.linspace(0, P - 1, num=min(n, P)).astype(np.int64))


def batch_rows(pool, perm, B):
    """The minibatch `perm[:B]` (env-major sample indices) of a pool -> (obs, actions, old logp, targets)."""
    T, N = pool["actions"].shape
    idx = np.asarray(perm[:B], np.int64)
    rows = (idx % T) * N + idx // T
    D = pool["obs"].shape[-1]
    return (pool["obs"].reshape(-1, D)[rows], pool["actions"].reshape(-1)[rows], pool["logprobs"].reshape(-1)[rows],
            pool["returns"].reshape(-1)[rows])


def simulate_bandit(seed, rollouts=9, N=32, T=64, lr0=0.04, budget=20000, ent_coef=0.01, max_grad_norm=0.5):
    """Bandit-v0:reinforce end to end on the CPU, as the device agent runs it: zero observations and
    zero biases leave the backbone dead (h = 0, every weight gradient 0), so the policy is
    softmax(policy_head.bias) and only that bias trains.  Rows alternate pull / autoreset (reward 0,
    not done; NEXT_STEP autoreset), gamma 1, mc:rtg returns, the index map (the rollout's last row,
    an autoreset row after the last terminal, maps to the pull before it), one 2048-row minibatch
    per rollout, clip_grad_norm_ + Adam, policy_lr linear lr0 -> 0 over `budget` env steps.
    -> (final bias, [mean reward of each rollout's pulls])."""
    means = np.arange(10, dtype=np.float32)
    rng = np.random.default_rng(seed)
    bias = torch.nn.Parameter(torch.zeros(10))
    opt = torch.optim.Adam([bias], lr=lr0)
    pulls = []
    for k in range(rollouts):
        with torch.no_grad():
            p = torch.softmax(bias, 0).numpy().astype(np.float64)
        acts = rng.choice(10, size=(T, N), p=p / p.sum())
        rew = (means[acts] + rng.normal(size=(T, N))).astype(np.float32)
        dones = np.zeros((T, N), bool)
        dones[0::2] = True
        rew[1::2] = 0.0
        pulls.append(float(rew[0::2].mean()))
        ret = mc_returns(rew, dones, None, 1.0)
        _, idx_map, _ = valid_index_map(dones, None)
        idx = idx_map[rng.permutation(N * T)]
        rows = (idx % T) * N + idx // T
        a, t = torch.as_tensor(acts.reshape(-1)[rows]), torch.as_tensor(ret.reshape(-1)[rows])
        dist = torch.distributions.Categorical(logits=bias.expand(a.numel(), 10))
        loss = -(dist.log_prob(a) * t).mean() - ent_coef * dist.entropy().mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([bias], max_grad_norm)
        opt.step()
        for g in opt.param_groups:
            g["lr"] = lr0 * max(0.0, 1.0 - (k + 1) * N * T / budget)
    return bias.detach().numpy(), pulls
