"""Test helper: numpy twin of the device tabular env (gymnasium-solver_amd/csrc/gs_tabular.hip) —
the counter hash of its outcome and reset draws, the table lookup, TimeLimit, the vector NEXT_STEP
autoreset (reset step: reward 0, no done, action ignored) and the reference's DiscreteEncoder
(gym_wrappers/discrete_encoder.py) restated as float32.  It runs on the product's own tables
(gsamd.toytext), so it pins the kernel, not gymnasium: parity with gymnasium's own episodes is
UNPINNED (the draws are the device's hash, not numpy's PCG64).
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
OUTCOME_STREAM = 0x7AB1E       # csrc/gs_tabular.hip kOutcomeStream
UNIT = 1.0 / 9007199254740992.0


def _mix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def reset_unit(seed: int, env: int, episode: int) -> float:
    """env_reset_unit(seed, env, episode, 0) of csrc/gs_env_episode.h."""
    h = _mix64(_mix64(_mix64(_mix64(seed) ^ env) ^ episode) ^ 0xC0)
    return (h >> 11) * UNIT


def outcome_unit(seed: int, env: int, episode: int, step: int) -> float:
    h = _mix64(_mix64(_mix64(_mix64(_mix64(seed) ^ env) ^ episode) ^ step) ^ OUTCOME_STREAM)
    return (h >> 11) * UNIT


def encoding_dim(encoding: str, n_states: int) -> int:
    if encoding == "array":
        return 1
    if encoding == "binary":
        n_bits = 1
        while (1 << n_bits) < n_states:
            n_bits += 1
        return n_bits
    assert encoding == "onehot"
    return n_states


def encode(encoding: str, n_states: int, s: int) -> np.ndarray:
    """DiscreteEncoder.observation(s) as the float32 vector the policy reads."""
    if encoding == "array":
        return np.array([s], np.float32)
    vec = np.zeros(encoding_dim(encoding, n_states), np.float32)
    if encoding == "binary":
        for i in range(vec.shape[0]):       # LSB first
            vec[i] = float((s >> i) & 1)
    else:
        vec[int(s)] = 1.0
    return vec


class TabularTwin:
    def __init__(self, tables, n_envs, encoding, seed=42, env_offset=0, max_steps=100):
        self.next, self.reward, self.term, self.starts, self.S, self.A, self.K = tables
        self.N, self.encoding = int(n_envs), encoding
        self.seed, self.env_offset, self.max_steps = int(seed), int(env_offset), int(max_steps)
        self.state = np.zeros(self.N, np.int32)
        self.meta = np.zeros((self.N, 3), np.int32)          # steps, episodes, pending
        self.ep_ret = np.zeros(self.N, np.float32)
        self.ep_count = np.zeros(self.N, np.int32)
        self.ep_ret_sum = np.zeros(self.N, np.float32)
        self.ep_len_sum = np.zeros(self.N, np.float32)
        self.outcomes = np.full(self.N, -1)                  # the last step's outcome index (-1: reset step)

    def _reset_state(self, e, episode):
        u = reset_unit(self.seed, self.env_offset + e, episode)
        return int(self.starts[min(len(self.starts) - 1, int(u * len(self.starts)))])

    def reset(self):
        for e in range(self.N):
            self.state[e] = self._reset_state(e, 0)
        self.meta[:] = 0
        self.ep_ret[:] = 0
        return self.obs()

    def obs(self):
        return np.stack([encode(self.encoding, self.S, int(s)) for s in self.state])

    def step(self, actions):
        rew = np.zeros(self.N, np.float32)
        done = np.zeros(self.N, np.uint8)
        trunc = np.zeros(self.N, np.uint8)
        for e in range(self.N):
            steps, episodes, pending = (int(v) for v in self.meta[e])
            if pending:
                self.state[e] = self._reset_state(e, episodes)
                self.meta[e] = (0, episodes, 0)
                self.ep_ret[e] = 0
                self.outcomes[e] = -1
                continue
            a = min(max(int(actions[e]), 0), self.A - 1)
            u = outcome_unit(self.seed, self.env_offset + e, episodes, steps)
            k = min(self.K - 1, int(u * self.K))
            s = int(self.state[e])
            terminated = bool(self.term[s, a, k])
            rew[e] = self.reward[s, a, k]
            self.state[e] = self.next[s, a, k]
            self.outcomes[e] = k
            steps += 1
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
