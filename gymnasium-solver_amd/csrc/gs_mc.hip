// gs_mc.hip — Monte Carlo returns for REINFORCE (gs_mc_returns_f32): the reference's
// compute_batched_mc_returns / convert_returns_to_full_episode (utils/returns_advantages.py:67-113)
// and _build_valid_mask_and_index_map (:33-52) on time-major (T, N) rows.  Compiled with
// -ffp-contract=off: the scan is three float32 roundings per step, as numpy's.
#include <limits.h>

#include "gs_head.h"

namespace gs {
namespace {

// One lane per env: the backward return scan, the env's last terminal, and (kind GS_MC_EPISODE) the
// forward pass that holds every episode segment at its first step's return.
__global__ void __launch_bounds__(256)
k_mc_scan(const float *__restrict__ rew, const uint8_t *__restrict__ dones, const uint8_t *__restrict__ timeouts, int T,
          int N, float gamma, int kind, float *__restrict__ ret, int32_t *__restrict__ last_term)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float acc = 0.0f;
    int lt = -1;
    for (int t = T - 1; t >= 0; --t) {
        const int i = t * N + n;
        const bool term = dones[i] != 0 && !(timeouts && timeouts[i] != 0);
        const float nt = term ? 0.0f : 1.0f;
        const float fut = acc * nt;          // returns_acc * non_terminal
        const float disc = gamma * fut;      // gamma * future (gamma as float32)
        acc = rew[i] + disc;
        ret[i] = acc;
        if (term && lt < 0) lt = t;
    }
    last_term[n] = lt;
    if (kind == GS_MC_EPISODE && T > 0) {
        float seg = ret[n];
        for (int t = 0; t < T; ++t) {
            const int i = t * N + n;
            const bool term = dones[i] != 0 && !(timeouts && timeouts[i] != 0);
            float next = seg;
            if (term && t + 1 < T) next = ret[i + N];    // the next segment's first return, not yet overwritten
            ret[i] = seg;
            seg = next;
        }
    }
}

// One workgroup: the first valid index, the prefix max over envs of each env's last valid index
// (chunks of 256 envs with a carry), the env-major index map and the valid returns' sums.
__global__ void __launch_bounds__(256)
k_mc_index(const float *__restrict__ ret, const int32_t *__restrict__ last_term, int T, int N,
           int32_t *__restrict__ idx_map, double *__restrict__ sums)
{
    __shared__ int s_scan[2][256];
    __shared__ double s_red[3 * (256 + 16)];
    const int tid = threadIdx.x;
    // the first env with a terminal: its step 0 is the rollout's first valid position
    int first = INT_MAX;
    for (int n = tid; n < N; n += 256)
        if (last_term[n] >= 0) { first = n; break; }
    s_scan[0][tid] = first;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_scan[0][tid] = min(s_scan[0][tid], s_scan[0][tid + o]);
        __syncthreads();
    }
    const int n0 = s_scan[0][0];
    __syncthreads();
    if (n0 == INT_MAX) {        // nothing valid: the reference keeps no map (identity), no baseline update
        if (idx_map)
            for (int i = tid; i < N * T; i += 256) idx_map[i] = i;
        if (tid < 3) sums[tid] = 0.0;
        return;
    }
    const int first_valid = n0 * T;
    double acc[3] = {0.0, 0.0, 0.0};
    int carry = -1;
    for (int base = 0; base < N; base += 256) {
        const int n = base + tid;
        const int lt = n < N ? last_term[n] : -1;
        int cur = 0;
        s_scan[0][tid] = lt >= 0 ? n * T + lt : -1;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {      // inclusive max scan, double-buffered
            const int v = s_scan[cur][tid];
            s_scan[cur ^ 1][tid] = tid >= o ? max(v, s_scan[cur][tid - o]) : v;
            cur ^= 1;
            __syncthreads();
        }
        const int excl = tid > 0 ? max(carry, s_scan[cur][tid - 1]) : carry;
        carry = max(carry, s_scan[cur][255]);
        if (n < N) {
            const int before = excl < 0 ? first_valid : excl;    // an env with no terminal: the previous valid index
            if (idx_map)
                for (int t = 0; t < T; ++t)
                    idx_map[n * T + t] = t <= lt ? n * T + t : (lt >= 0 ? n * T + lt : before);
            for (int t = 0; t <= lt; ++t) {
                const double x = (double)ret[t * N + n];
                acc[0] += 1.0;
                acc[1] += x;
                acc[2] += x * x;
            }
        }
        __syncthreads();
    }
    block_reduce<3, double>(acc, s_red);
    if (tid < 3) sums[tid] = acc[tid];
}

}  // namespace
}  // namespace gs

extern "C" int gs_mc_returns_f32(const float *rewards, const uint8_t *dones, const uint8_t *timeouts, int64_t T,
                                 int64_t N, double gamma, int kind, float *returns, int32_t *idx_map,
                                 int32_t *last_terminal, double *valid_sums, void *stream)
{
    using namespace gs;
    GS_REQUIRE(T > 0 && N > 0 && T * N < (int64_t)1 << 31, "gs_mc_returns_f32: T=%lld N=%lld outside 1 <= T*N < 2^31",
               (long long)T, (long long)N);
    GS_REQUIRE(kind == GS_MC_RTG || kind == GS_MC_EPISODE, "gs_mc_returns_f32: kind %d is neither GS_MC_RTG nor "
               "GS_MC_EPISODE", kind);
    GS_REQUIRE(rewards && dones && returns && last_terminal && valid_sums, "gs_mc_returns_f32: null buffer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mc_scan, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, rewards, dones, timeouts, (int)T,
                       (int)N, (float)gamma, kind, returns, last_terminal);
    GS_LAUNCH_CHECK("k_mc_scan");
    hipLaunchKernelGGL(k_mc_index, dim3(1), dim3(256), 0, s, returns, last_terminal, (int)T, (int)N, idx_map, valid_sums);
    GS_LAUNCH_CHECK("k_mc_index");
    return GS_OK;
}
