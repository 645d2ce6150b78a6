"""numpy twins of the two optimizer steps the device path adds beside Adam (include/gsamd.h
GS_HP_OPT_ADAMW / GS_HP_OPT_SGD): torch 2.10's torch.optim.AdamW(params, lr=lr) and
torch.optim.SGD(params, lr=lr) on their single-tensor paths, float32 throughout — every scalar is
formed in double as torch forms it and cast to float32 once, every array operation rounds to
float32, in torch's order.  tests/test_optimizers_cpu.py holds them to torch on the CPU; the GPU
tests use decay_factor and the zero-gradient chain.  numpy only."""
import numpy as np

F32 = np.float32
WEIGHT_DECAY = 0.01          # torch.optim.AdamW's default; include/gsamd.h GS_ADAMW_WEIGHT_DECAY


def decay_factor(lr):
    """f32(1 - (double)lr * 0.01) from the float32 lr a hyper-parameter struct carries"""
    return F32(1.0 - float(F32(lr)) * WEIGHT_DECAY)


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor step t (1-based), amsgrad off, no decay"""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    m = m + F32(1.0 - b1) * (g - m)                      # exp_avg.lerp_(grad, 1 - beta1)
    v = v * F32(b2) + (F32(1.0 - b2) * g) * g            # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    step_size = float(F32(lr)) / (1.0 - b1 ** t)
    bc2_sqrt = (1.0 - b2 ** t) ** 0.5
    denom = np.sqrt(v) / F32(bc2_sqrt) + F32(eps)
    p = p + F32(-step_size) * (m / denom)                # param.addcdiv_(exp_avg, denom, value=-step_size)
    return p.astype(F32), m.astype(F32), v.astype(F32)


def adamw_step(p, g, m, v, t, lr, **kw):
    """torch.optim.AdamW: param.mul_(1 - lr * weight_decay), then Adam's step"""
    p = np.asarray(p, F32) * decay_factor(lr)
    return adam_step(p, g, m, v, t, lr, **kw)


def sgd_step(p, g, lr):
    """torch.optim.SGD, momentum 0, no decay: param.add_(grad, alpha=-lr)"""
    return (np.asarray(p, F32) + F32(-float(F32(lr))) * np.asarray(g, F32)).astype(F32)


def decayed(p0, lr, n):
    """p0 multiplied n times by decay_factor(lr) in float32: an AdamW parameter whose gradient stays 0"""
    p, d = np.asarray(p0, F32).copy(), decay_factor(lr)
    for _ in range(n):
        p = (p * d).astype(F32)
    return p
