"""Test helper: the reference's CartPoleV1_RewardShaper arithmetic (gym_wrappers/CartPoleV1/
reward_shaper.py) restated in Python floats, the twin of cartpole_phi / CartPoleShapedEnv in
csrc/gs_cartpole_env.h.  tests/golden/cartpole_shaper.npz pins it to the class bit for bit
(test_cartpole_bandit_cpu.py); the GPU test then uses it where the fixture cannot reach (envs whose
reset hash is not the fixture's).
"""
from __future__ import annotations

import math

import numpy as np

X_THR, TH_THR = 2.4, 12.0 * 2.0 * math.pi / 360.0


def phi(obs, angle_reward_scale=1.0, position_reward_scale=0.25, clip_potential=True) -> float:
    x, theta = float(obs[0]), float(obs[2])
    pos = 1.0 - abs(x) / max(X_THR, 1e-6)
    ang = 1.0 - abs(theta) / max(TH_THR, 1e-6)
    if clip_potential:
        pos = min(max(pos, 0.0), 1.0)
        ang = min(max(ang, 0.0), 1.0)
    return angle_reward_scale * ang + position_reward_scale * pos


def shaped_rewards(obs0, obs, reset, **kw):
    """(rewards (S, N) float32, final prev_phi (N) float64) of the wrapper over recorded float32
    observations obs (S, N, 4) that follow the reset observations obs0 (N, 4); reset (S, N) marks
    the NEXT_STEP autoreset rows (reward 0, prev_phi re-armed)."""
    S, N = reset.shape
    prev = np.array([phi(obs0[e], **kw) for e in range(N)], np.float64)
    rew = np.zeros((S, N), np.float32)
    for t in range(S):
        for e in range(N):
            p = phi(obs[t][e], **kw)
            if not reset[t][e]:
                rew[t][e] = np.float32(1.0 + (p - prev[e]))
            prev[e] = p
    return rew, prev
