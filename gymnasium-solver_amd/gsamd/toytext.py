"""Transition tables of gymnasium 1.x FrozenLake-v1 and Taxi-v3 for the device tabular env
(csrc/gs_tabular.hip, gsamd.rollout.DeviceTabularVecEnv).  Pure numpy, no device import.

Both envs are finite MDPs whose outcomes per (state, action) are K equiprobable alternatives, so
each is three arrays of shape (S, A, K): the next state (int32), the reward (float32) and the
terminated flag (uint8), plus the start states a reset draws from uniformly.

The rules below restate gymnasium 1.x's ``toy_text/frozen_lake.py`` and ``toy_text/taxi.py`` (the
default Taxi: no rain, no fickle passenger).  gymnasium is not installed here, so nothing is
compared with gymnasium's own tables or episodes: that parity stays UNPINNED, exactly as for the
other device envs (the device also draws outcomes and resets from its counter hash, not from
gymnasium's PCG64 stream).  What is pinned: a second, naive per-state simulator and the envs'
published facts (tests/test_toytext_cpu.py).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

Tables = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int, int, int]

FROZENLAKE_MAPS = {
    "4x4": ("SFFF", "FHFH", "FFFH", "HFFG"),
    "8x8": ("SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG"),
}
# TimeLimit of the registered ids (gymnasium/envs/__init__.py): FrozenLake-v1 100 whatever the map
# (the 8x8 map's 200 belongs to the id FrozenLake8x8-v1), Taxi-v3 200
MAX_EPISODE_STEPS = {"frozenlake": 100, "taxi": 200}

TAXI_MAP = ("+---------+", "|R: | : :G|", "| : | : : |", "| : : : : |", "| | : | : |", "|Y| : |B: |", "+---------+")
TAXI_LOCS = ((0, 0), (0, 4), (4, 0), (4, 3))


def frozenlake_table(map_name: str = "4x4", is_slippery: bool = True) -> Tables:
    """(next, reward, term, starts, n_states, n_actions, K) of FrozenLake-v1.  Actions 0 LEFT,
    1 DOWN, 2 RIGHT, 3 UP, clipped to the grid; slippery: the three outcomes are the moves of
    (a - 1) % 4, a, (a + 1) % 4 in that order (probability 1/3 each), else the move of a alone;
    reward 1 on entering G; terminated on entering H or G; every entry of an H or G state stays
    there with reward 0, terminated; the episode starts at state 0."""
    desc = FROZENLAKE_MAPS[map_name]
    nrow, ncol = len(desc), len(desc[0])
    S, A, K = nrow * ncol, 4, 3 if is_slippery else 1
    nxt = np.zeros((S, A, K), np.int32)
    rew = np.zeros((S, A, K), np.float32)
    term = np.zeros((S, A, K), np.uint8)

    def move(row, col, a):
        if a == 0:
            col = max(col - 1, 0)
        elif a == 1:
            row = min(row + 1, nrow - 1)
        elif a == 2:
            col = min(col + 1, ncol - 1)
        else:
            row = max(row - 1, 0)
        return row, col

    for row in range(nrow):
        for col in range(ncol):
            s = row * ncol + col
            for a in range(A):
                for k in range(K):
                    if desc[row][col] in "GH":
                        nxt[s, a, k], rew[s, a, k], term[s, a, k] = s, 0.0, 1
                        continue
                    b = (a - 1 + k) % 4 if is_slippery else a
                    r2, c2 = move(row, col, b)
                    letter = desc[r2][c2]
                    nxt[s, a, k] = r2 * ncol + c2
                    rew[s, a, k] = 1.0 if letter == "G" else 0.0
                    term[s, a, k] = 1 if letter in "GH" else 0
    return nxt, rew, term, np.zeros(1, np.int32), S, A, K


def taxi_encode(row: int, col: int, passenger: int, dest: int) -> int:
    return ((row * 5 + col) * 5 + passenger) * 4 + dest


def taxi_table() -> Tables:
    """(next, reward, term, starts, 500, 6, 1) of Taxi-v3.  State ((row 5 + col) 5 + pass) 4 + dest
    with pass 4 = in the taxi; actions 0 south, 1 north, 2 east, 3 west (east / west only through a
    ':' of the map), 4 pickup, 5 dropoff; reward -1 per step, -10 for an illegal pickup / dropoff,
    +20 and terminated for a dropoff at the destination; starts: the 300 states with the passenger
    at a location other than the destination."""
    S, A, K = 500, 6, 1
    nxt = np.zeros((S, A, K), np.int32)
    rew = np.zeros((S, A, K), np.float32)
    term = np.zeros((S, A, K), np.uint8)
    starts = []
    for row in range(5):
        for col in range(5):
            for p in range(5):
                for dest in range(4):
                    s = taxi_encode(row, col, p, dest)
                    if p < 4 and p != dest:
                        starts.append(s)
                    for a in range(A):
                        r2, c2, p2, reward, done = row, col, p, -1.0, 0
                        loc = (row, col)
                        if a == 0:
                            r2 = min(row + 1, 4)
                        elif a == 1:
                            r2 = max(row - 1, 0)
                        elif a == 2:
                            if TAXI_MAP[1 + row][2 * col + 2] == ":":
                                c2 = col + 1
                        elif a == 3:
                            if TAXI_MAP[1 + row][2 * col] == ":":
                                c2 = col - 1
                        elif a == 4:
                            if p < 4 and loc == TAXI_LOCS[p]:
                                p2 = 4
                            else:
                                reward = -10.0
                        else:
                            if p == 4 and loc == TAXI_LOCS[dest]:
                                p2, reward, done = dest, 20.0, 1
                            elif p == 4 and loc in TAXI_LOCS:
                                p2 = TAXI_LOCS.index(loc)
                            else:
                                reward = -10.0
                        nxt[s, a, 0], rew[s, a, 0], term[s, a, 0] = taxi_encode(r2, c2, p2, dest), reward, done
    return nxt, rew, term, np.asarray(starts, np.int32), S, A, K


def tables_for(kind: str, map_name: str = "4x4", is_slippery: bool = True) -> Tables:
    if kind == "frozenlake":
        return frozenlake_table(map_name, is_slippery)
    if kind == "taxi":
        return taxi_table()
    raise ValueError(f"no tabular env {kind!r}")
