// gs_env_kernels.h — the reset and step kernels of every device env, generic over the env type E
// (gs_env_episode.h), one thread per env, and their launch helpers.  The per-env .hip files keep
// the extern "C" entries: argument checks, E::Args, one call to a helper.
#pragma once

#include "gs_common.h"
#include "gs_env_episode.h"

namespace gs {

template <class E>
__global__ __launch_bounds__(256) void k_env_reset(typename E::Args ev, int64_t N)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    E env;
    env.reset(ev, e);
    env.store(ev, e);
    env.write_obs(ev, ev.obs + e * E::obs_dim(ev));
}

template <class E>
__global__ __launch_bounds__(256) void k_env_step(typename E::Args ev, const int64_t *__restrict__ actions, int64_t N,
                                                  float *__restrict__ rew_row, uint8_t *__restrict__ done_row,
                                                  uint8_t *__restrict__ to_row)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    E env;
    env.load(ev, e);
    const EnvStepOut so = env.step(ev, e, actions[e]);
    rew_row[e] = so.reward;
    done_row[e] = so.done ? 1 : 0;
    to_row[e] = so.timeout ? 1 : 0;
    env.store(ev, e);
    env.write_obs(ev, ev.obs + e * E::obs_dim(ev));
}

template <class E>
int launch_env_reset(const typename E::Args &ev, int64_t N, void *stream)
{
    hipLaunchKernelGGL(k_env_reset<E>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ev, N);
    GS_LAUNCH_CHECK("k_env_reset");
    return GS_OK;
}

template <class E>
int launch_env_step(const typename E::Args &ev, const int64_t *actions, int64_t N, float *rew_row, uint8_t *done_row,
                    uint8_t *to_row, void *stream)
{
    hipLaunchKernelGGL(k_env_step<E>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ev,
                       actions, N, rew_row, done_row, to_row);
    GS_LAUNCH_CHECK("k_env_step");
    return GS_OK;
}

}  // namespace gs
