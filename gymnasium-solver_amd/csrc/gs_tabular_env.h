// gs_tabular_env.h — the generic tabular device env: the env type TabularEnv behind the step
// kernels (gs_tabular.hip) and the one-hidden-layer policy's one-launch rollout (gs_mlp1.hip
// k_rollout1, entry gs_rollout1_tabular), see gs_env_episode.h.  Any finite MDP whose outcomes per (state,
// action) are K equiprobable alternatives, given as three read-only tables in HBM (next state,
// reward, terminated; [S][A][K]).  The observation is the reference's
// gym_wrappers/discrete_encoder.py applied on the env's own thread, as float32.  The
// two-hidden-layer one-launch rollout (gs_mlp.hip k_rollout_env) does not serve it.
// Twin: tests/tabular_twin.py.
#pragma once

#include "gs_env_episode.h"

namespace gs {

constexpr uint64_t kOutcomeStream = 0x7AB1E;    // distinct from the reset draws' 0xC0 + c

// uniform in [0, 1) of (seed, global env, episode, step in episode): the outcome draw
__device__ __forceinline__ double tabular_outcome_unit(uint64_t seed, uint64_t ge, uint64_t episode, uint64_t step)
{
    const uint64_t h = env_mix64(
        env_mix64(env_mix64(env_mix64(env_mix64(seed) ^ ge) ^ episode) ^ step) ^ kOutcomeStream);
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct TabularEnv : EnvEpisode {
    struct Args : EnvArgs {
        int32_t *state;              // [N]
        gs_tabular_spec sp;
        const int32_t *next_tab;     // [S][A][K]; null for a reset
        const float *reward_tab;
        const uint8_t *term_tab;
        const int32_t *starts;       // [n_starts]
    };
    static __device__ __forceinline__ int obs_dim(const Args &ev) { return ev.sp.obs_dim; }
    int s;
    __device__ __forceinline__ void draw_start(const Args &ev, int64_t me)
    {
        const double u = env_reset_unit(ev.seed, (uint64_t)(ev.env_offset + me), (uint64_t)meta[1], 0);
        const int j = min(ev.sp.n_starts - 1, (int)(u * (double)ev.sp.n_starts));
        s = clampi(ev.starts[j], 0, ev.sp.n_states - 1);
    }
    __device__ __forceinline__ void load(const Args &ev, int64_t me)
    {
        s = clampi(ev.state[me], 0, ev.sp.n_states - 1);
        load_episode(ev, me);
    }
    __device__ __forceinline__ void store(const Args &ev, int64_t me) const
    {
        ev.state[me] = s;
        store_episode(ev, me);
    }
    __device__ __forceinline__ void reset(const Args &ev, int64_t me)
    {
        reset_episode();
        draw_start(ev, me);
    }
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (autoreset()) {
            draw_start(ev, me);
            return EnvStepOut{};
        }
        // every table index is range-checked: a bad action or table entry cannot leave the tables
        const gs_tabular_spec &sp = ev.sp;
        const int a = action < 0 ? 0 : (action >= sp.n_actions ? sp.n_actions - 1 : (int)action);
        const double u = tabular_outcome_unit(ev.seed, (uint64_t)(ev.env_offset + me), (uint64_t)meta[1],
                                              (uint64_t)meta[0]);
        const int k = min(sp.n_outcomes - 1, (int)(u * (double)sp.n_outcomes));
        const int64_t at = ((int64_t)s * sp.n_actions + a) * sp.n_outcomes + k;
        const int ns = ev.next_tab[at];
        const bool bad = ns < 0 || ns >= sp.n_states;      // forced terminal
        const bool terminated = ev.term_tab[at] != 0 || bad;
        const float reward = ev.reward_tab[at];
        s = bad ? s : ns;
        return finish_step(ev, me, reward, terminated);
    }
    // gym_wrappers/discrete_encoder.py observation(), as float32
    __device__ __forceinline__ void write_obs(const Args &ev, float *__restrict__ o) const
    {
        const gs_tabular_spec &sp = ev.sp;
        if (sp.encoding == GS_ENC_ARRAY) {
            o[0] = (float)s;
        } else if (sp.encoding == GS_ENC_BINARY) {
            for (int i = 0; i < sp.obs_dim; ++i) o[i] = (float)((s >> i) & 1);      // LSB first
        } else {
            for (int i = 0; i < sp.obs_dim; ++i) o[i] = i == s ? 1.0f : 0.0f;
        }
    }
};

}  // namespace gs
