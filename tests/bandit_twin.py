"""Test helper: numpy twin of the device Bandit-v0 (gymnasium-solver_amd/csrc/gs_bandit_env.h) —
the counter hash of its two uniforms, the Box-Muller normal, reward = mean[a] + std[a] z in double
stored as float32, termination at episode_length, TimeLimit and the vector NEXT_STEP autoreset
(reset step: reward 0, no done, action ignored).  parse_arms restates how the reference's
MultiArmedBanditEnv (gym_envs/mab_env.py:179-187) builds its float32 means and stds; it is pinned to
the class by tests/golden/bandit_env.npz.  The draws are the device's hash, not numpy's PCG64
ziggurat: parity with the reference's own reward stream is UNPINNED.
"""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
NORMAL_TAG = 0xBA0             # csrc/gs_bandit_env.h: component c of a draw hashes 0xBA0 + c
UNIT = 1.0 / 9007199254740992.0


def _mix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def unit(seed: int, env: int, episode: int, step: int, c: int) -> float:
    h = _mix64(_mix64(_mix64(_mix64(_mix64(seed) ^ env) ^ episode) ^ step) ^ (NORMAL_TAG + c))
    return (h >> 11) * UNIT


def normal(seed: int, env: int, episode: int, step: int) -> float:
    u1, u2 = unit(seed, env, episode, step, 0), unit(seed, env, episode, step, 1)
    return math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(2.0 * math.pi * u2)


def parse_arms(n_arms: int, means=None, stds=1.0):
    """(means, stds) float32 [n_arms]: the default means are linspace(0, n_arms, n_arms) in
    float32, a scalar std is broadcast."""
    n = int(n_arms)
    m = np.linspace(0, n, num=n, dtype=np.float32) if means is None else np.asarray(means, dtype=np.float32)
    s = np.full(n, float(stds), dtype=np.float32) if isinstance(stds, (int, float)) else np.asarray(stds, np.float32)
    assert m.shape == (n,) and s.shape == (n,)
    return m, s


class BanditTwin:
    def __init__(self, n_envs, n_arms=10, means=None, stds=1.0, episode_length=1, seed=42, env_offset=0,
                 max_steps=None):
        self.N, self.n_arms, self.episode_length = int(n_envs), int(n_arms), int(episode_length)
        self.means, self.stds = parse_arms(n_arms, means, stds)
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.max_steps = int(max_steps if max_steps else episode_length)
        self.meta = np.zeros((self.N, 3), np.int32)          # steps, episodes, pending
        self.ep_ret = np.zeros(self.N, np.float32)
        self.ep_count = np.zeros(self.N, np.int32)
        self.ep_ret_sum = np.zeros(self.N, np.float32)
        self.ep_len_sum = np.zeros(self.N, np.float32)

    def reset(self):
        self.meta[:] = 0
        self.ep_ret[:] = 0
        return self.obs()

    def obs(self):
        return np.zeros((self.N, self.n_arms), np.float32)

    def step(self, actions):
        rew = np.zeros(self.N, np.float32)
        done = np.zeros(self.N, np.uint8)
        trunc = np.zeros(self.N, np.uint8)
        for e in range(self.N):
            steps, episodes, pending = (int(v) for v in self.meta[e])
            if pending:
                self.meta[e] = (0, episodes, 0)
                self.ep_ret[e] = 0
                continue
            a = min(max(int(actions[e]), 0), self.n_arms - 1)
            z = normal(self.seed, self.env_offset + e, episodes, steps)
            rew[e] = np.float32(float(self.means[a]) + float(self.stds[a]) * z)
            steps += 1
            terminated = steps >= self.episode_length
            truncated = (not terminated) and steps >= self.max_steps
            self.ep_ret[e] = np.float32(self.ep_ret[e] + rew[e])
            if terminated or truncated:
                self.ep_count[e] += 1
                self.ep_ret_sum[e] = np.float32(self.ep_ret_sum[e] + self.ep_ret[e])
                self.ep_len_sum[e] = np.float32(self.ep_len_sum[e] + np.float32(steps))
                episodes += 1
                pending = 1
                done[e], trunc[e] = 1, int(truncated)
            self.meta[e] = (steps, episodes, pending)
        return rew, done, trunc
