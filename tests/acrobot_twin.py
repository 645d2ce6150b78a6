"""Test helper: pure-Python float64 twin of the device Acrobot-v1 dynamics
(gymnasium-solver_amd/csrc/gs_acrobot_env.h).

gymnasium 1.x's AcrobotEnv ("book" variant, no torque noise; gymnasium is not installed here) is
restated from its published equations: one classical RK4 step of dt = 0.2, angles wrapped into
[-pi, pi] by repeated +-2 pi (at most WRAP_CAP turns each way, as on the device), velocities
clamped to 4 pi / 9 pi, terminated when -cos t1 - cos(t1 + t2) > 1, reward -1 (0 on the
terminating step), TimeLimit, vector NEXT_STEP autoreset (reset step: reward 0, no done, action
ignored).  Reset draws are the device's counter hash, uniform in [-0.1, 0.1) and rounded to
float32, not numpy's PCG64: parity with gymnasium's own episodes is UNPINNED; this twin pins the
kernel (device sin / cos are not glibc's correctly rounded ones, so states agree to ~1e-12).
"""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
PI = math.pi
DT = 0.2
MAX_VEL_1, MAX_VEL_2 = 4.0 * PI, 9.0 * PI
WRAP_CAP = 16       # csrc/gs_acrobot_env.h kAcWrapCap, with the bound's derivation


def _mix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def reset_uniform(seed: int, env: int, episode: int, c: int) -> float:
    h = _mix64(_mix64(_mix64(_mix64(seed) ^ env) ^ episode) ^ (0xC0 + c))
    return float(np.float32(-0.1 + 0.2 * ((h >> 11) * (1.0 / 9007199254740992.0))))


def _cos(x):
    return math.cos(x) if math.isfinite(x) else math.nan      # C's cos, not Python's ValueError


def _sin(x):
    return math.sin(x) if math.isfinite(x) else math.nan


def dsdt(y, a):
    """AcrobotEnv._dsdt ("book"): d/dt of (t1, t2, w1, w2) under torque a."""
    t1, t2, w1, w2 = y
    m1 = m2 = l1 = I1 = I2 = 1.0
    lc1 = lc2 = 0.5
    g = 9.8
    c2, s2 = _cos(t2), _sin(t2)
    d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * c2) + I1 + I2
    d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2
    phi2 = m2 * lc2 * g * _cos(t1 + t2 - PI / 2.0)
    phi1 = (-m2 * l1 * lc2 * (w2 * w2) * s2 - 2.0 * m2 * l1 * lc2 * w2 * w1 * s2
            + (m1 * lc1 + m2 * l1) * g * _cos(t1 - PI / 2.0) + phi2)
    dw2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * s2 - phi2) / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1)
    dw1 = -(d2 * dw2 + phi1) / d1
    return (w1, w2, dw1, dw2)


def rk4(y, a, dt):
    """One classical RK4 step, summed in the device's order ((k1 + 2 k2) + 2 k3) + k4."""
    k = (0.0, 0.0, 0.0, 0.0)
    acc = [0.0, 0.0, 0.0, 0.0]
    for c, w in ((0.0, 1.0), (dt / 2.0, 2.0), (dt / 2.0, 2.0), (dt, 1.0)):
        k = dsdt(tuple(y[j] + c * k[j] for j in range(4)), a)
        for j in range(4):
            acc[j] += w * k[j]
    return [y[j] + dt / 6.0 * acc[j] for j in range(4)]


def wrap(x):
    """(wrapped x, turns taken): repeated -+2 pi, at most WRAP_CAP turns each way."""
    n = 0
    i = 0
    while i < WRAP_CAP and x > PI:
        x -= 2.0 * PI
        i += 1
    n += i
    i = 0
    while i < WRAP_CAP and x < -PI:
        x += 2.0 * PI
        i += 1
    return x, n + i


def clamp(x, lim):
    return -lim if x < -lim else (lim if x > lim else x)


def height(s):
    return -_cos(s[0]) - _cos(s[0] + s[1])


def step_state(s, action):
    """The dynamics of one env step on a bare state: (new state, terminated, info); info counts
    what the step exercised (wrap turns per angle, clamps)."""
    y = rk4(list(s), float(int(action) - 1), DT)
    t1, n1 = wrap(y[0])
    t2, n2 = wrap(y[1])
    w1, w2 = clamp(y[2], MAX_VEL_1), clamp(y[3], MAX_VEL_2)
    ns = [t1, t2, w1, w2]
    info = {"wrap1": n1, "wrap2": n2, "clamp1": w1 != y[2], "clamp2": w2 != y[3]}
    return ns, height(ns) > 1.0, info


def obs_of(s):
    return np.array([_cos(s[0]), _sin(s[0]), _cos(s[1]), _sin(s[1]), s[2], s[3]], dtype=np.float32)


class AcrobotTwin:
    def __init__(self, n_envs, seed=42, env_offset=0, max_steps=500):
        self.N, self.seed, self.off, self.max_steps = n_envs, seed, env_offset, max_steps
        self.state = [[reset_uniform(seed, env_offset + e, 0, c) for c in range(4)] for e in range(n_envs)]
        self.steps = [0] * n_envs
        self.episodes = [0] * n_envs
        self.pending = [False] * n_envs
        self.infos = [None] * n_envs      # per env: step_state's info, or "reset" on a reset step

    def obs(self):
        return np.stack([obs_of(s) for s in self.state])

    def step(self, actions):
        rew = np.zeros(self.N, np.float32)
        done = np.zeros(self.N, bool)
        trunc = np.zeros(self.N, bool)
        for e in range(self.N):
            if self.pending[e]:
                self.state[e] = [reset_uniform(self.seed, self.off + e, self.episodes[e], c) for c in range(4)]
                self.steps[e] = 0
                self.pending[e] = False
                self.infos[e] = "reset"
                continue
            self.state[e], term, self.infos[e] = step_state(self.state[e], actions[e])
            self.steps[e] += 1
            tr = (not term) and self.steps[e] >= self.max_steps
            rew[e] = 0.0 if term else -1.0
            done[e], trunc[e] = term or tr, tr
            if term or tr:
                self.episodes[e] += 1
                self.pending[e] = True
        return rew, done, trunc
