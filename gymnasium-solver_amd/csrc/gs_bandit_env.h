// gs_bandit_env.h — device Bandit-v0's per-env arithmetic, shared by the step kernels
// (gs_bandit.hip) and the one-launch rollout (gs_mlp.hip k_rollout_env), so both produce the same
// bits.  Both files compile with -ffp-contract=off.  Twin: tests/bandit_twin.py.
//
// The env restates the reference's gym_envs/mab_env.py MultiArmedBanditEnv: a stateless Gaussian
// multi-armed bandit whose observation is zeros(n_arms), reward = mean[a] + std[a] z in double
// (means / stds are float32, as the class keeps them), stored as float32, terminated when the
// steps in the episode reach episode_length; the env itself never truncates, a config's
// max_episode_steps adds the usual TimeLimit.  NEXT_STEP autoreset as every device env here.
//
// The normal draw is Box-Muller on two 53-bit uniforms of the counter hash of (seed, global env
// index, episode index, step in episode, component): z = sqrt(-2 log(1 - u1)) cos(2 pi u2).  The
// device cannot reproduce numpy's PCG64 ziggurat, so parity with the reference's own reward
// stream is UNPINNED, as parity with gymnasium's streams is for the other device envs.  The
// draw depends on those counters only: the step loop, a captured graph and the one-launch
// rollout see the same bits.  The component tags 0xBA0 + c are disjoint from the reset tags
// 0xC0 + c of env_reset_unit.
#pragma once

#include "gs_cartpole_env.h"   // env_mix64, EnvStepOut
#include "../../include/gsamd.h"

namespace gs {

// uniform in [0, 1): 53-bit mantissa from the hash of (seed, env, episode, step, component)
__device__ __forceinline__ double bandit_unit(uint64_t seed, uint64_t env, uint64_t episode, uint64_t step, int c)
{
    const uint64_t h = env_mix64(
        env_mix64(env_mix64(env_mix64(env_mix64(seed) ^ env) ^ episode) ^ step) ^ (uint64_t)(0xBA0 + c));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// standard normal of (seed, env, episode, step): 1 - u1 is in (0, 1], so the log is finite
__device__ __forceinline__ double bandit_normal(uint64_t seed, uint64_t env, uint64_t episode, uint64_t step)
{
    const double u1 = bandit_unit(seed, env, episode, step, 0), u2 = bandit_unit(seed, env, episode, step, 1);
    return sqrt(-2.0 * log(1.0 - u1)) * cos(2.0 * M_PI * u2);
}

// One env's step: meta {steps, episodes, pending} and the running return advance; on a done the
// (null-tolerant) episode counters add the finished episode.  ge = the global env index.  An
// action outside [0, n_arms) is clamped, so no index leaves the spec's arrays.
__device__ __forceinline__ EnvStepOut bandit_env_step(int32_t (&meta)[3], float &er, int64_t action, int max_steps,
                                                      uint64_t seed, uint64_t ge, const gs_bandit_spec &sp,
                                                      int32_t *ep_cnt, float *ep_ret_sum, float *ep_len_sum)
{
    if (meta[2] != 0) {        // NEXT_STEP autoreset: this step only resets
        meta[0] = 0;
        meta[2] = 0;
        er = 0.0f;
        return EnvStepOut{0.0f, false, false};
    }
    const int last = (sp.n_arms < GS_BANDIT_MAX_ARMS ? sp.n_arms : GS_BANDIT_MAX_ARMS) - 1;
    const int a = action < 0 ? 0 : (action > last ? last : (int)action);
    const double z = bandit_normal(seed, ge, (uint64_t)meta[1], (uint64_t)meta[0]);
    const float reward = (float)((double)sp.means[a] + (double)sp.stds[a] * z);
    const int steps = meta[0] + 1;
    const bool terminated = steps >= sp.episode_length;
    const bool truncated = !terminated && steps >= max_steps;
    er = er + reward;
    if (terminated || truncated) {
        if (ep_cnt) *ep_cnt += 1;
        if (ep_ret_sum) *ep_ret_sum += er;
        if (ep_len_sum) *ep_len_sum += (float)steps;
        meta[1] += 1;
        meta[2] = 1;
    }
    meta[0] = steps;
    return EnvStepOut{reward, terminated || truncated, truncated};
}

}  // namespace gs
