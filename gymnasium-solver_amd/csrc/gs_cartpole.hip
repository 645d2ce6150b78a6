// gs_cartpole.hip — device-resident CartPole-v1 dynamics.
//
// The reference trains on gymnasium 1.x `CartPole-v1` (not vendored: gymnasium is absent
// offline, so parity with its trajectories is UNPINNED).  This kernel restates its published
// dynamics: cart-pole constants, Euler integration with tau = 0.02 in double precision (the
// environment keeps its state as Python floats), termination at |x| > 2.4 or |theta| > 12 deg,
// TimeLimit truncation at 500 steps, reward 1, and the vector env's NEXT_STEP autoreset: the
// step after a done resets that env, ignores its action and returns the reset observation
// with reward 0 and no done flag (the zero-reward transition the reference trains on,
// SURVEY §8 a4).  Reset states are uniform in [-0.05, 0.05) from a counter-based hash
// (numpy's PCG64 stream is not reproduced).  The numpy twin is oracle/cartpole_ref.py.
// The per-env arithmetic lives in gs_cartpole_env.h.
// gs_cartpole_shaped_*: the same env under the reference's CartPoleV1_RewardShaper
// (CartPole-v1:ppo_rewardshaped), with the wrapper's previous potential in an (N) f64 tensor of
// its own; the (N, 4) state and the unshaped entries are unchanged.  The shaper's arithmetic is
// pinned to the reference's class by tests/golden/cartpole_shaper.npz.
#include <math.h>

#include "gs_common.h"
#include "gs_cartpole_env.h"   // the per-env arithmetic, shared with the one-launch rollout

namespace {

using namespace gs;

__global__ __launch_bounds__(256) void k_cartpole_reset(double *__restrict__ st, int32_t *__restrict__ meta,
                                                        float *__restrict__ ep_ret, float *__restrict__ obs, int64_t N,
                                                        uint64_t seed, int64_t env_offset)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    CPState s;
    cartpole_reset_state(s, seed, (uint64_t)(env_offset + e), 0);
    reinterpret_cast<CPState *>(st)[e] = s;
    meta[3 * e + 0] = 0;   // steps in the current episode
    meta[3 * e + 1] = 0;   // episodes finished (the reset counter)
    meta[3 * e + 2] = 0;   // 1 = the previous step ended an episode (autoreset pending)
    ep_ret[e] = 0.0f;
    cartpole_write_obs(s, obs + 4 * e);
}

__global__ __launch_bounds__(256) void k_cartpole_step(double *__restrict__ st, int32_t *__restrict__ meta,
                                                       float *__restrict__ ep_ret, float *__restrict__ obs,
                                                       const int64_t *__restrict__ actions, int64_t N, int max_steps,
                                                       uint64_t seed, int64_t env_offset, float *__restrict__ rew_row,
                                                       uint8_t *__restrict__ done_row, uint8_t *__restrict__ to_row,
                                                       int32_t *__restrict__ ep_cnt, float *__restrict__ ep_ret_sum,
                                                       float *__restrict__ ep_len_sum)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    CPState s = reinterpret_cast<CPState *>(st)[e];
    int32_t m[3] = {meta[3 * e + 0], meta[3 * e + 1], meta[3 * e + 2]};
    float er = ep_ret[e];
    const EnvStepOut so = cartpole_env_step(s, m, er, actions[e], max_steps, seed, (uint64_t)(env_offset + e),
                                            ep_cnt ? ep_cnt + e : nullptr, ep_ret_sum ? ep_ret_sum + e : nullptr,
                                            ep_len_sum ? ep_len_sum + e : nullptr);
    rew_row[e] = so.reward;
    done_row[e] = so.done ? 1 : 0;
    to_row[e] = so.timeout ? 1 : 0;
    meta[3 * e + 0] = m[0];
    meta[3 * e + 1] = m[1];
    meta[3 * e + 2] = m[2];
    ep_ret[e] = er;
    reinterpret_cast<CPState *>(st)[e] = s;
    cartpole_write_obs(s, obs + 4 * e);
}

__global__ __launch_bounds__(256) void k_cartpole_shaped_reset(double *__restrict__ st, double *__restrict__ prev_phi,
                                                               int32_t *__restrict__ meta, float *__restrict__ ep_ret,
                                                               float *__restrict__ obs, gs_cartpole_wrappers w,
                                                               int64_t N, uint64_t seed, int64_t env_offset)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    CPState s;
    cartpole_reset_state(s, seed, (uint64_t)(env_offset + e), 0);
    reinterpret_cast<CPState *>(st)[e] = s;
    prev_phi[e] = cartpole_phi(w, s);      // the wrapper's reset(): the reset observation's potential
    meta[3 * e + 0] = 0;
    meta[3 * e + 1] = 0;
    meta[3 * e + 2] = 0;
    ep_ret[e] = 0.0f;
    cartpole_write_obs(s, obs + 4 * e);
}

__global__ __launch_bounds__(256) void k_cartpole_shaped_step(
    double *__restrict__ st, double *__restrict__ prev_phi, int32_t *__restrict__ meta, float *__restrict__ ep_ret,
    float *__restrict__ obs, gs_cartpole_wrappers w, const int64_t *__restrict__ actions, int64_t N, int max_steps,
    uint64_t seed, int64_t env_offset, float *__restrict__ rew_row, uint8_t *__restrict__ done_row,
    uint8_t *__restrict__ to_row, int32_t *__restrict__ ep_cnt, float *__restrict__ ep_ret_sum,
    float *__restrict__ ep_len_sum)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    CPState s = reinterpret_cast<CPState *>(st)[e];
    double pp = prev_phi[e];
    int32_t m[3] = {meta[3 * e + 0], meta[3 * e + 1], meta[3 * e + 2]};
    float er = ep_ret[e];
    const EnvStepOut so = cartpole_shaped_env_step(s, pp, m, er, actions[e], max_steps, seed,
                                                   (uint64_t)(env_offset + e), w, ep_cnt ? ep_cnt + e : nullptr,
                                                   ep_ret_sum ? ep_ret_sum + e : nullptr,
                                                   ep_len_sum ? ep_len_sum + e : nullptr);
    rew_row[e] = so.reward;
    done_row[e] = so.done ? 1 : 0;
    to_row[e] = so.timeout ? 1 : 0;
    meta[3 * e + 0] = m[0];
    meta[3 * e + 1] = m[1];
    meta[3 * e + 2] = m[2];
    ep_ret[e] = er;
    prev_phi[e] = pp;
    reinterpret_cast<CPState *>(st)[e] = s;
    cartpole_write_obs(s, obs + 4 * e);
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int gs_cartpole_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int64_t N,
                                 uint64_t seed, int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev, "gs_cartpole_reset: bad argument");
    hipLaunchKernelGGL(k_cartpole_reset, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev, meta_dev,
                       ep_ret_dev, obs_dev, N, seed, env_offset);
    GS_LAUNCH_CHECK("k_cartpole_reset");
    return GS_OK;
}

extern "C" int gs_cartpole_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                                const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                                int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                                uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                                float *ep_len_sum_dev, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_cartpole_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_cartpole_step: null output row");
    hipLaunchKernelGGL(k_cartpole_step, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev, meta_dev,
                       ep_ret_dev, obs_dev, actions_dev, N, max_steps, seed, env_offset, rewards_row_dev,
                       dones_row_dev, timeouts_row_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev);
    GS_LAUNCH_CHECK("k_cartpole_step");
    return GS_OK;
}

extern "C" int gs_cartpole_shaped_reset(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                                        float *obs_dev, gs_cartpole_wrappers wrappers, int64_t N, uint64_t seed,
                                        int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && prev_phi_dev && meta_dev && ep_ret_dev && obs_dev,
               "gs_cartpole_shaped_reset: bad argument");
    hipLaunchKernelGGL(k_cartpole_shaped_reset, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev,
                       prev_phi_dev, meta_dev, ep_ret_dev, obs_dev, wrappers, N, seed, env_offset);
    GS_LAUNCH_CHECK("k_cartpole_shaped_reset");
    return GS_OK;
}

extern "C" int gs_cartpole_shaped_step(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                                       float *obs_dev, gs_cartpole_wrappers wrappers, const int64_t *actions_dev,
                                       int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                                       float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                                       int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                                       void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && prev_phi_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_cartpole_shaped_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_cartpole_shaped_step: null output row");
    hipLaunchKernelGGL(k_cartpole_shaped_step, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev,
                       prev_phi_dev, meta_dev, ep_ret_dev, obs_dev, wrappers, actions_dev, N, max_steps, seed,
                       env_offset, rewards_row_dev, dones_row_dev, timeouts_row_dev, ep_done_count_dev,
                       ep_ret_sum_dev, ep_len_sum_dev);
    GS_LAUNCH_CHECK("k_cartpole_shaped_step");
    return GS_OK;
}
