// gs_bandit.hip — device-resident Bandit-v0, the reference's algorithm-correctness environment
// (gym_envs/mab_env.py MultiArmedBanditEnv).
//
// A stateless Gaussian multi-armed bandit: the observation is zeros(n_arms) on reset and after
// every step, the reward of arm a is mean[a] + std[a] z, the episode terminates after
// episode_length steps.  The per-env arithmetic and the normal draw are in gs_bandit_env.h
// (shared with the one-launch rollout).  numpy's PCG64 ziggurat stream is not reproduced: the
// draw is Box-Muller on the counter hash, so parity with the reference's own reward stream is
// UNPINNED, as parity with gymnasium's streams is for the other device envs.  The arms' float32
// means and stds travel by value in gs_bandit_spec.  The numpy twin is tests/bandit_twin.py.
#include <math.h>

#include "gs_common.h"
#include "gs_bandit_env.h"

namespace gs {

// what the entries check before a launch: the arm count keeps every index inside the spec's arrays
const char *bandit_spec_error(const gs_bandit_spec &sp)
{
    if (sp.n_arms < 2 || sp.n_arms > GS_BANDIT_MAX_ARMS) return "n_arms must be in [2, 32]";
    if (sp.episode_length < 1) return "episode_length must be >= 1";
    for (int a = 0; a < sp.n_arms; ++a) {
        if (!(fabsf(sp.means[a]) <= 3.4028234e38f)) return "means must be finite";
        if (!(sp.stds[a] >= 0.0f && sp.stds[a] <= 3.4028234e38f)) return "stds must be finite and >= 0";
    }
    return nullptr;
}

}  // namespace gs

namespace {

using namespace gs;

__global__ __launch_bounds__(256) void k_bandit_reset(int32_t *__restrict__ meta, float *__restrict__ ep_ret,
                                                      float *__restrict__ obs, int n_arms, int64_t N)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    meta[3 * e + 0] = 0;   // steps in the current episode
    meta[3 * e + 1] = 0;   // episodes finished
    meta[3 * e + 2] = 0;   // 1 = the previous step ended an episode (autoreset pending)
    ep_ret[e] = 0.0f;
    for (int d = 0; d < n_arms; ++d) obs[e * n_arms + d] = 0.0f;
}

__global__ __launch_bounds__(256) void k_bandit_step(int32_t *__restrict__ meta, float *__restrict__ ep_ret,
                                                     float *__restrict__ obs, gs_bandit_spec sp,
                                                     const int64_t *__restrict__ actions, int64_t N, int max_steps,
                                                     uint64_t seed, int64_t env_offset, float *__restrict__ rew_row,
                                                     uint8_t *__restrict__ done_row, uint8_t *__restrict__ to_row,
                                                     int32_t *__restrict__ ep_cnt, float *__restrict__ ep_ret_sum,
                                                     float *__restrict__ ep_len_sum)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    int32_t m[3] = {meta[3 * e + 0], meta[3 * e + 1], meta[3 * e + 2]};
    float er = ep_ret[e];
    const EnvStepOut so = bandit_env_step(m, er, actions[e], max_steps, seed, (uint64_t)(env_offset + e), sp,
                                          ep_cnt ? ep_cnt + e : nullptr, ep_ret_sum ? ep_ret_sum + e : nullptr,
                                          ep_len_sum ? ep_len_sum + e : nullptr);
    rew_row[e] = so.reward;
    done_row[e] = so.done ? 1 : 0;
    to_row[e] = so.timeout ? 1 : 0;
    meta[3 * e + 0] = m[0];
    meta[3 * e + 1] = m[1];
    meta[3 * e + 2] = m[2];
    ep_ret[e] = er;
    for (int d = 0; d < sp.n_arms; ++d) obs[e * sp.n_arms + d] = 0.0f;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int gs_bandit_reset(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec, int64_t N,
                               void *stream)
{
    GS_REQUIRE(N > 0 && meta_dev && ep_ret_dev && obs_dev, "gs_bandit_reset: bad argument");
    const char *bad = bandit_spec_error(spec);
    GS_REQUIRE(!bad, "gs_bandit_reset: %s", bad);
    hipLaunchKernelGGL(k_bandit_reset, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, meta_dev, ep_ret_dev, obs_dev,
                       (int)spec.n_arms, N);
    GS_LAUNCH_CHECK("k_bandit_reset");
    return GS_OK;
}

extern "C" int gs_bandit_step(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec,
                              const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                              int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                              uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                              float *ep_len_sum_dev, void *stream)
{
    GS_REQUIRE(N > 0 && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_bandit_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_bandit_step: null output row");
    const char *bad = bandit_spec_error(spec);
    GS_REQUIRE(!bad, "gs_bandit_step: %s", bad);
    hipLaunchKernelGGL(k_bandit_step, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, meta_dev, ep_ret_dev, obs_dev,
                       spec, actions_dev, N, max_steps, seed, env_offset, rewards_row_dev, dones_row_dev,
                       timeouts_row_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev);
    GS_LAUNCH_CHECK("k_bandit_step");
    return GS_OK;
}
