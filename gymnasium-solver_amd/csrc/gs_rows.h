// gs_rows.h — what the two row-tile updates share, gs_pg.hip (REINFORCE) and gs_ppo_rows.hip (the
// row-parallel PPO update): the pieces of a workgroup's 16-row tiles, the workspace carver, the leading
// call checks.  Only for files compiled with the default -ffp-contract; the others share gs_head.h.
#pragma once

#include "gs_common.h"

namespace gs {

constexpr int kRowsTile = 16;      // minibatch rows of one tile: one MFMA row block

// an index outside the rollout or an action outside [0, A) is clamped, never followed
__device__ __forceinline__ int rows_sample(const int32_t *idx, int i, int TN) { return min(max(idx[i], 0), TN - 1); }
__device__ __forceinline__ int rows_action(int64_t a, int A) { return a < 0 ? 0 : (a >= A ? A - 1 : (int)a); }

// mean and unbiased std from a sum and a sum of squares (utils/torch.py:97-99); normalising callers add 1e-8f
struct RowsMoments { double mean, std; };
__device__ __forceinline__ RowsMoments rows_moments(double sum, double sq, double n)
{
    return {sum / n, sqrt(fmax(0.0, (sq - sum * sum / n) / (n - 1.0)))};
}

// the tile's observations into LDS; zeros for a ragged tile's rows past the minibatch (frow[r] < 0)
__device__ __forceinline__ void rows_gather_obs(const float *obs, const int *frow, int D, float *x)
{
    for (int e = threadIdx.x; e < kRowsTile * D; e += 256) {
        const int r = e / D, d = e - r * D;
        x[e] = frow[r] >= 0 ? obs[(size_t)frow[r] * D + d] : 0.0f;
    }
}

// the workgroup's metric sums: its row threads' accumulators added in row order (rsum: 16 NS doubles of LDS)
template <int NS>
__device__ __forceinline__ void rows_store_sums(const double (&acc)[NS], double *rsum, double *out)
{
    const int tid = threadIdx.x;
    if (tid < kRowsTile)
#pragma unroll
        for (int k = 0; k < NS; ++k) rsum[tid * NS + k] = acc[k];
    __syncthreads();
    if (tid < NS) {
        double s = 0.0;
        for (int r = 0; r < kRowsTile; ++r) s += rsum[r * NS + tid];
        out[tid] = s;
    }
}

// the workspaces' bump allocation in 256-byte steps; with a null base only the size is meaningful
struct RowsCarver {
    char *base;
    size_t bytes = 0;
    template <class T> T *take(size_t count)
    {
        T *p = (T *)(base + bytes);
        bytes += (sizeof(T) * count + 255) & ~(size_t)255;
        return p;
    }
};

// the two checks that lead pg_run and rows_run alike; the others they share in text keep their places
// among each entry's own, which differ, since callers rely on which check of a bad call fails first
inline bool rows_batch_ok(int64_t batch) { return batch >= 2 && batch <= (int64_t)1 << 20; }
inline int rows_check_batch(int64_t batch, int64_t T, int64_t N, const char *what)
{
    GS_REQUIRE(rows_batch_ok(batch), "%s: batch %lld outside [2, 2^20]", what, (long long)batch);
    GS_REQUIRE(T > 0 && N > 0 && T * N < (int64_t)1 << 31, "%s: rollout shape outside 1 <= T*N < 2^31", what);
    return GS_OK;
}

}  // namespace gs
