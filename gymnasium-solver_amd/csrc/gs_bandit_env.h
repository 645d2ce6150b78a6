// gs_bandit_env.h — device Bandit-v0: the env type BanditEnv behind the step kernels
// (gs_bandit.hip) and the one-launch rollout (gs_mlp.hip k_rollout_env), see gs_env_episode.h.
// Twin: tests/bandit_twin.py.
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

#include "gs_env_episode.h"

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

// null, or what is wrong with the spec: every bandit entry checks this before a launch, so no
// index leaves the spec's arrays (gs_bandit.hip)
const char *bandit_spec_error(const gs_bandit_spec &sp);

// No state beyond meta and the running return; the observation rows stay zero.  An action outside
// [0, n_arms) is clamped, so no index leaves the spec's arrays.  The policy of a one-launch rollout
// has n_arms actions: a 10-action runtime shape serves the reference's 10 arms (head_act_row's sums
// run over a < A in order, so its rows equal gs_policy_act's 32-action shape); more arms take the
// step loop.
struct BanditEnv : EnvEpisode {
    struct Args : EnvArgs {
        gs_bandit_spec sp;
    };
    static constexpr int kRolloutAmax = GS_BANDIT_ROLLOUT_MAX_ARMS;
    static bool takes_policy(int D, int A) { return D == A && A >= 2 && A <= GS_BANDIT_ROLLOUT_MAX_ARMS; }
    static __device__ __forceinline__ int obs_dim(const Args &ev) { return ev.sp.n_arms; }
    __device__ __forceinline__ void load(const Args &ev, int64_t me) { load_episode(ev, me); }
    __device__ __forceinline__ void store(const Args &ev, int64_t me) const { store_episode(ev, me); }
    __device__ __forceinline__ void reset(const Args &, int64_t) { reset_episode(); }
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (autoreset()) return EnvStepOut{};
        const gs_bandit_spec &sp = ev.sp;
        const int last = (sp.n_arms < GS_BANDIT_MAX_ARMS ? sp.n_arms : GS_BANDIT_MAX_ARMS) - 1;
        const int a = action < 0 ? 0 : (action > last ? last : (int)action);
        const double z = bandit_normal(ev.seed, (uint64_t)(ev.env_offset + me), (uint64_t)meta[1], (uint64_t)meta[0]);
        const float reward = (float)((double)sp.means[a] + (double)sp.stds[a] * z);
        return finish_step(ev, me, reward, meta[0] + 1 >= sp.episode_length);
    }
    __device__ __forceinline__ void write_obs(const Args &ev, float *o) const
    {
        for (int d = 0; d < ev.sp.n_arms; ++d) o[d] = 0.0f;
    }
    __device__ __forceinline__ void next_obs(const Args &, float *xs, int64_t, int64_t, int D, int, int tid, bool) const
    {
        for (int u = tid; u < 16 * D; u += 256) xs[u] = 0.0f;
    }
};

}  // namespace gs
