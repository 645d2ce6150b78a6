// gs_rollout1.h — the one-launch rollout of the one-hidden-layer policy (gs_mlp1.hip
// k_rollout1<AMAX, E>) as the gs_rollout1_* entries see it: the LDS rule, the checks every entry
// runs alike, and the launch of env type E (gs_env_episode.h), instantiated in gs_mlp1.hip for
// TabularEnv, CartPoleEnv, CartPoleShapedEnv, AcrobotEnv, MountainCarEnv and BanditEnv.
#pragma once

#include "gs_common.h"
#include "gs_env_episode.h"

namespace gs {

constexpr int kRollout1Envs = 64;    // envs of one workgroup: one wave, one env per lane

// LDS of one workgroup: the parameters plus kRollout1Envs observation rows of stride D | 1
size_t mlp1_rollout_lds_bytes(const gs_mlp_dims &d);
bool mlp1_rollout_fits(const gs_mlp_dims &d);

// What the gs_rollout1_* entries check alike, under the entry's name: check_rollout_entry's list
// (gs_ppo.hip) with the one-layer condition inverted, and the one-hidden-layer envelope.
int mlp1_check_rollout_entry(const char *who, const gs_mlp_dims &dims, int64_t N, int64_t T, int mode,
                             const float *params, const EnvArgs &ev, const RolloutRows &rw);

template <class E>
int mlp1_launch_rollout(const float *P, const gs_mlp_dims &d, int64_t N, int T, int mode, uint64_t rng_seed,
                        uint64_t counter0, const typename E::Args &ev, const RolloutRows &rw, hipStream_t s);

// the rollout of env type E behind its entry: the shared checks, then `bad` (null, or what the
// entry found wrong with its own tensors and parameters), then the policy's shape against the
// env's (env_D observation values, env_A actions); nothing to do for T == 0
template <class E>
int rollout1_entry(const char *who, const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                   uint64_t rng_seed, uint64_t rng_counter0, const typename E::Args &ev, const RolloutRows &rw,
                   int env_D, int env_A, const char *bad, void *stream)
{
    int rc = mlp1_check_rollout_entry(who, dims, N, T, mode, params, ev, rw);
    if (rc) return rc;
    GS_REQUIRE(!bad, "%s: %s", who, bad);
    GS_REQUIRE(dims.obs_dim == env_D && dims.n_actions == env_A,
               "%s: the policy (obs dim %d, %d actions) is not the env's (obs dim %d, %d actions)", who, dims.obs_dim,
               dims.n_actions, env_D, env_A);
    GS_REQUIRE(mlp1_rollout_fits(dims), "%s: the parameters and %d observation rows need %zu bytes of LDS", who,
               kRollout1Envs, mlp1_rollout_lds_bytes(dims));
    if (T == 0) return GS_OK;
    return mlp1_launch_rollout<E>(params, dims, N, (int)T, mode, rng_seed, rng_counter0, ev, rw, (hipStream_t)stream);
}

}  // namespace gs
