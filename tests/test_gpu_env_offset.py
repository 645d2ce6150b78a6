"""env_offset partitions the same trajectories, for every device env class: N envs as one env
object and the same global envs as two objects compute the same bits.  An env thread indexes its
tensors (and MountainCar its count table) by the local env index and draws its hashes from the
global one, env_offset + local; the split at 256 puts the two on different sides of a block."""
import numpy as np
import pytest
import torch

import mountaincar_twin as MT

pytestmark = pytest.mark.gpu

N, SPLIT, STEPS, MAXS, SEED = 257, 256, 24, 5, 11
MC_BOTH = [{"id": MT.SHAPER}, {"id": MT.BONUS, "position_bins": 12, "velocity_bins": 10}]


def _make(name, n, off, cuda):
    from gsamd import rollout as R
    kw = dict(seed=SEED, env_offset=off, max_steps=MAXS, device=cuda)
    if name == "synthetic":
        return R.DeviceSyntheticVecEnv(n, 5, 3, episode_len=MAXS, seed=SEED, truncate_every=2, env_offset=off,
                                       device=cuda)
    if name == "cartpole":
        return R.DeviceCartPoleVecEnv(n, **kw)
    if name == "cartpole_shaped":
        return R.DeviceCartPoleVecEnv(n, wrappers=[{"id": "CartPoleV1_RewardShaper"}], **kw)
    if name == "acrobot":
        return R.DeviceAcrobotVecEnv(n, **kw)
    if name == "mountaincar_bonus":
        return R.DeviceMountainCarVecEnv(n, wrappers=MC_BOTH, **kw)
    if name == "bandit":
        return R.DeviceBanditVecEnv(n, n_arms=4, episode_length=8, **kw)
    return R.DeviceTabularVecEnv(n, kind="frozenlake", encoding="binary", **kw)


def _rows(n, cuda):
    return (torch.zeros(n, device=cuda), torch.zeros(n, dtype=torch.uint8, device=cuda),
            torch.zeros(n, dtype=torch.uint8, device=cuda))


# every per-env tensor an env class may carry; all of them are indexed by the local env
TENSORS = ("obs", "state", "meta", "prev_phi", "counts", "ep_ret", "ep_count", "ep_ret_sum", "ep_len_sum")


def _per_env(env):
    out = {}
    for k in TENSORS:
        t = getattr(env, k, None)
        if t is not None:
            out[k] = t.reshape(env.num_envs, -1)
    return out


@pytest.mark.parametrize("name", ["synthetic", "cartpole", "cartpole_shaped", "acrobot", "mountaincar_bonus", "bandit",
                                  "tabular"])
def test_env_offset_partitions_the_same_trajectories(cuda, name):
    """257 envs as one object against the same global envs as [0, 256) and [256, 257): 24 steps of
    fixed random actions under max_steps 5, so every env crosses several autoresets.  Rewards,
    dones, timeouts and every per-env tensor (observations, state, meta, the shaper's potentials,
    the count tables, the episode counters) are bitwise equal after each step."""
    whole, parts = _make(name, N, 0, cuda), (_make(name, SPLIT, 0, cuda), _make(name, N - SPLIT, SPLIT, cuda))
    for env in (whole, *parts):
        env.reset()
    rw, rp = _rows(N, cuda), (_rows(SPLIT, cuda), _rows(N - SPLIT, cuda))
    rng = np.random.default_rng(3)
    dones = 0
    for step in range(STEPS + 1):
        a, b = _per_env(whole), [_per_env(p) for p in parts]
        assert a.keys() == b[0].keys() == b[1].keys() and "obs" in a and "ep_ret" in a
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), torch.cat([b[0][k], b[1][k]]).view(torch.uint8)), (step, k)
        if step:
            for x, y0, y1 in zip(rw, *rp):
                assert torch.equal(x.view(torch.uint8), torch.cat([y0, y1]).view(torch.uint8)), step
            dones += int(rw[1].sum())
        if step == STEPS:
            break
        act = torch.as_tensor(rng.integers(0, whole.n_actions, N), dtype=torch.int64, device=cuda)
        whole.step_into(*rw, actions=act)
        parts[0].step_into(*rp[0], actions=act[:SPLIT].contiguous())
        parts[1].step_into(*rp[1], actions=act[SPLIT:].contiguous())
    # NEXT_STEP autoreset under max_steps 5: an episode and its reset row take at most 6 steps
    assert dones >= N * (STEPS // (MAXS + 1))
    if name == "mountaincar_bonus":
        assert int(whole.counts[SPLIT:].sum()) > 0          # the last env's own table took its visits
