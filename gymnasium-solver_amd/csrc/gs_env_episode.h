// gs_env_episode.h — what every device env with real dynamics shares: the counter hash of the
// reset draws, the step's result, the common tensors, and the episode bookkeeping (NEXT_STEP
// autoreset, TimeLimit truncation, the finished-episode counters) written once.
//
// An env type E (one per gs_*_env.h) is the only description of its env on the device.  It derives
// from EnvEpisode and adds: `Args` (EnvArgs plus its own tensors and parameters), its per-thread
// state, obs_dim(ev), load / store (registers <-> tensors of local env `me`), reset (episode 0),
// step (one vector step given the action), write_obs (the observation of the state, to a row),
// and, with a one-launch rollout, next_obs (called by all 256 threads: the next observations into
// the LDS rows xs [16][D]), kRolloutAmax (the ShapeR the rollout runs on) and takes_policy(D, A).
// k_env_reset / k_env_step (gs_env_kernels.h) and k_rollout_env (gs_mlp.hip) are generic over E,
// so the step loop and the one-launch rollout produce the same bits; all compile with
// -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/gsamd.h"

namespace gs {

__device__ __forceinline__ uint64_t env_mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// uniform in [0, 1): 53-bit mantissa from the hash of (seed, env, episode, component)
__device__ __forceinline__ double env_reset_unit(uint64_t seed, uint64_t env, uint64_t episode, int c)
{
    const uint64_t h = env_mix64(env_mix64(env_mix64(env_mix64(seed) ^ env) ^ episode) ^ (uint64_t)(0xC0 + c));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// what one env step writes into the rollout rows; EnvStepOut{} is a reset row (reward 0, no flag)
struct EnvStepOut {
    float reward;
    bool done, timeout;
};

// the tensors and scalars every env's Args start with; env `me` of them is global env env_offset + me
struct EnvArgs {
    int32_t *meta;                   // [N][3] {steps in the episode, episodes finished, autoreset pending}
    float *ep_ret, *obs;             // [N], [N][D]: running return, current observation
    int32_t *ep_cnt;                 // [N] finished-episode counters (may be null)
    float *ep_ret_sum, *ep_len_sum;
    int max_steps;
    uint64_t seed;
    int64_t env_offset;
};
struct DynEnvArgs : EnvArgs {        // CartPole, Acrobot, MountainCar: a state of four doubles
    double *state;                   // [N][4]
};

// the per-thread registers every env carries, and the bookkeeping on them
struct EnvEpisode {
    int32_t meta[3];
    float er;
    __device__ __forceinline__ void load_episode(const EnvArgs &ev, int64_t me)
    {
        meta[0] = ev.meta[3 * me + 0];
        meta[1] = ev.meta[3 * me + 1];
        meta[2] = ev.meta[3 * me + 2];
        er = ev.ep_ret[me];
    }
    __device__ __forceinline__ void store_episode(const EnvArgs &ev, int64_t me) const
    {
        ev.meta[3 * me + 0] = meta[0];
        ev.meta[3 * me + 1] = meta[1];
        ev.meta[3 * me + 2] = meta[2];
        ev.ep_ret[me] = er;
    }
    __device__ __forceinline__ void reset_episode()
    {
        meta[0] = meta[1] = meta[2] = 0;
        er = 0.0f;
    }
    // NEXT_STEP autoreset: true when the previous step ended an episode, so this step only resets.
    // The caller then draws episode meta[1]'s reset state and returns the zero row, EnvStepOut{}.
    __device__ __forceinline__ bool autoreset()
    {
        if (meta[2] == 0) return false;
        meta[0] = 0;
        meta[2] = 0;
        er = 0.0f;
        return true;
    }
    // the end of a step that ran the dynamics: TimeLimit truncation, the running return, and on a
    // done the (null-tolerant) episode counters, then meta
    __device__ __forceinline__ EnvStepOut finish_step(const EnvArgs &ev, int64_t me, float reward, bool terminated)
    {
        const int steps = meta[0] + 1;
        const bool truncated = !terminated && steps >= ev.max_steps;
        er = er + reward;
        if (terminated || truncated) {
            if (ev.ep_cnt) ev.ep_cnt[me] += 1;
            if (ev.ep_ret_sum) ev.ep_ret_sum[me] += er;
            if (ev.ep_len_sum) ev.ep_len_sum[me] += (float)steps;
            meta[1] += 1;
            meta[2] = 1;
        }
        meta[0] = steps;
        return EnvStepOut{reward, terminated || truncated, truncated};
    }
};

// CartPole / Acrobot / MountainCar: State is four doubles in ev.state, ResetState the reset draw of
// (seed, global env, episode), WriteObs the observation; in a one-launch rollout the env thread
// writes it into its LDS row
template <class State, int OBS_DIM, int ACTIONS, void (*ResetState)(State &, uint64_t, uint64_t, uint64_t),
          void (*WriteObs)(const State &, float *)>
struct DynEnv : EnvEpisode {
    static constexpr int kObsDim = OBS_DIM, kActions = ACTIONS;
    static constexpr int kRolloutAmax = 4;       // no compile-time shape of these dims fits in LDS: ShapeR<4>
    static bool takes_policy(int D, int A) { return D == OBS_DIM && A == ACTIONS; }
    static __device__ __forceinline__ int obs_dim(const EnvArgs &) { return OBS_DIM; }
    State s;
    __device__ __forceinline__ void load(const DynEnvArgs &ev, int64_t me)
    {
        s = reinterpret_cast<const State *>(ev.state)[me];
        load_episode(ev, me);
    }
    __device__ __forceinline__ void store(const DynEnvArgs &ev, int64_t me) const
    {
        reinterpret_cast<State *>(ev.state)[me] = s;
        store_episode(ev, me);
    }
    __device__ __forceinline__ void reset(const DynEnvArgs &ev, int64_t me)
    {
        ResetState(s, ev.seed, (uint64_t)(ev.env_offset + me), 0);
        reset_episode();
    }
    // the NEXT_STEP autoreset row: true when this step only reset the env, ignoring its action
    __device__ __forceinline__ bool reset_row(const DynEnvArgs &ev, int64_t me)
    {
        if (!autoreset()) return false;
        ResetState(s, ev.seed, (uint64_t)(ev.env_offset + me), (uint64_t)meta[1]);
        return true;
    }
    __device__ __forceinline__ void write_obs(const EnvArgs &, float *o) const { WriteObs(s, o); }
    __device__ __forceinline__ void next_obs(const EnvArgs &, float *xs, int64_t, int64_t, int, int, int tid,
                                             bool env_thread) const
    {
        if (env_thread) WriteObs(s, xs + OBS_DIM * tid);
    }
};

}  // namespace gs
