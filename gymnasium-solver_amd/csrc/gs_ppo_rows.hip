// gs_ppo_rows.hip — the row-parallel PPO update (gs_ppo_rows_update / gs_ppo_rows_loss):
// PPOAgent.losses_for_batch (agents/ppo/ppo_agent.py:21-152) + BaseAgent._backpropagate_and_step
// (agents/base_agent.py:591-621) for the one- and two-hidden-layer actor-critics on minibatches of
// up to 2^20 rows, fp32, one GPU.  The data flow is gs_pg.hip's with the value head inside the loss.
// Launches per optimizer step:
//   k_ppo_rows_adv   (normalize_adv only) the minibatch's advantage sums in double, one part per
//                    workgroup over a contiguous range of rows; the row workgroups add the parts in
//                    part order, so all of them hold the same mean and std.  A launch of its own: at
//                    B = 2^20 every row workgroup gathering the whole minibatch again (gs_pg.hip's way)
//                    would be 256 x 2^20 dependent gathers
//   k_ppo_rows       workgroups own 16-row tiles (looping when there are more tiles than workgroups):
//                    gather by idx, obs -> h1 (-> h2) -> logits | value, loss_row, dz -> the head
//                    gradient, dh2, dW2, dh1, dW1 and the biases.  A workgroup adds its tiles' share into
//                    its own partial slot (HBM, one writer) and leaves its 14 metric sums, its
//                    activation-statistics sums and its per-neuron dead counts beside it
//   k_ppo_rows_sum   the slots summed in workgroup order into the flat gradient, the three component
//                    sums of squares per workgroup in double
//   k_ppo_rows_step  every workgroup adds the norm parts in part order (the same bits everywhere),
//                    clips and runs Adam on its share of the parameters; workgroup 0 writes the record
//                    (write_metrics, norms, GS_M_ACT) and sets the stop flag.  Spread over the grid
//                    rather than run by a ticket's last workgroup: mlp_medium has 67 k parameters, 263
//                    per thread of one workgroup, and the clip coefficient needs the whole norm first
// The H1 x H2 products of a two-layer net (h2, dh1, dW2) run on v_mfma_f32_16x16x4_f32 (exact f32);
// layer 1 (K = D <= 64) and the heads (A + 1 <= 33 columns) stay on the vector ALUs, where MFMA
// tiles would be mostly padding.  One hidden layer is the same kernel without the middle stage
// (template parameter TWO): the heads read h1.
// No float atomics and no ticket: every sum has a fixed order (rows in a tile, tiles in a workgroup,
// workgroups by index, parts by index); the per-neuron dead counts are integers.
// Under an action mask (gs_ppo_rows_update_masked / gs_ppo_rows_loss_masked) the row kernel is the
// same but for its loss row, loss_row_masked: every head column is formed, the invalid actions'
// dz is an exact 0, and so are their rows of the head gradient (no column compaction).
// Compiled with the default -ffp-contract (FMA), as gs_pg.hip: nothing here has to round as the
// chain's -ffp-contract=off files do, the MFMA products are fmaf chains anyway, and the contracted
// vector-ALU dot products carry one rounding less per term.
#include <math.h>

#include <algorithm>

#include "gs_head.h"
#include "gs_hparams.h"
#include "gs_rows.h"

namespace gs {
namespace {

constexpr int R = kRowsTile;
constexpr int kRowsMaxGroups = 256;    // row workgroups (and partial slots) at most: the MI355X's CU count
constexpr int kRowsMaxHidden = 512;
constexpr int kRowsSumGroups = 256;    // workgroups of the sum and step kernels at most
constexpr int kRowsAdvParts = 64;      // advantage-sum parts at most
constexpr int kRowsRedDoubles = 4 * (256 + 16);    // block_reduce<4, double> scratch
constexpr size_t kRowsStaticLds = 0;   // k_ppo_rows keeps all of its LDS in the dynamic part
constexpr size_t kLdsBudget = 160 * 1024;

// flat parameter layout of either net, the reference's state_dict order (Layout / Layout1 of
// gs_common.h); HK = the width the heads read (H2, or H1 with one hidden layer)
struct RowsLayout {
    int D, H1, H2, A, HK, two;
    int oW1, ob1, oW2, ob2, oWp, obp, oWv, obv, P;
    int S1, S2;                        // LDS row strides of the h1 / h2 tiles (+4: float4 reads stay aligned)
    __host__ __device__ int head_row(int c) const { return c < A ? oWp + c * HK : oWv; }
    __host__ __device__ int head_bias(int c) const { return c < A ? obp + c : obv; }
};

RowsLayout rows_layout(const gs_mlp_dims &d)
{
    RowsLayout L{};
    L.D = d.obs_dim, L.H1 = d.hidden1, L.H2 = d.hidden2, L.A = d.n_actions;
    L.two = d.hidden2 != 0 ? 1 : 0;
    L.HK = L.two ? L.H2 : L.H1;
    L.oW1 = 0;
    L.ob1 = L.H1 * L.D;
    L.oW2 = L.ob1 + L.H1;
    L.ob2 = L.oW2 + L.H2 * L.H1;
    L.oWp = L.ob2 + L.H2;
    L.obp = L.oWp + L.A * L.HK;
    L.oWv = L.obp + L.A;
    L.obv = L.oWv + L.HK;
    L.P = L.obv + 1;
    L.S1 = L.H1 + 4;
    L.S2 = L.H2 + 4;
    return L;
}

struct RowsArgs {
    const float *P;
    float *slots;               // [groups][stride] gradient partials
    double *msums;              // [groups][kNumSums] metric sums
    double *actsums;            // [groups][4] {sum z1, sum z1^2, sum z2, sum z2^2}
    uint32_t *dead;             // [groups][H1 + H2] rows with |z| < 1e-6 per neuron
    const double *advparts;     // [nparts][2] {sum adv, sum adv^2} of the minibatch
    const float *obs;
    const int64_t *actions;
    const float *logprobs, *values, *advantages, *returns;
    const int32_t *idx;
    const int32_t *stop;        // null unless target_kl is set
    int T, N, B, ntiles, stride, nparts, act_stats;
    LossArgs la;
    uint32_t valid;             // the masked head's valid actions (k_ppo_rows<.., true> only): behind every
                                // field the unmasked kernel reads, whose argument offsets so stay as they were
};

struct RowsStepArgs {
    float *P, *G, *M, *V;
    const float *slots;
    const double *msums, *actsums;
    const uint32_t *dead;
    double *normparts;          // [sum workgroups][3] {backbone, policy head, value head} sums of squares
    float *metrics;
    int32_t *stop;              // null unless target_kl is set
    int groups, stride, B, nsum, act_stats, do_step;
    LossArgs la;
    AdamArgs aa;
};

__host__ __device__ inline size_t rows_lds_bytes(const RowsLayout &L)
{
    const size_t A1 = L.A + 1;
    size_t f = (size_t)R * L.D + 2 * (size_t)R * L.S1 + (L.two ? 2 * (size_t)R * L.S2 : 0) + 2 * R * A1 + 6 * R +
               (size_t)(L.H1 + L.H2);
    return sizeof(double) * (kRowsRedDoubles + (size_t)R * kNumSums) + sizeof(float) * f;
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ppo_rows_adv(const int32_t *__restrict__ idx, const float *__restrict__ adv,
                                                      int T, int N, int B, int chunk, double *__restrict__ parts)
{
    __shared__ double red[2 * (256 + 16)];
    const int lo = blockIdx.x * chunk, hi = min(B, lo + chunk);
    double v[2] = {0.0, 0.0};
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const float t = adv[sample_row(rows_sample(idx, i, T * N), T, N)];
        v[0] += (double)t;
        v[1] += (double)t * (double)t;
    }
    block_reduce<2, double>(v, red);
    if (threadIdx.x == 0) parts[2 * blockIdx.x] = v[0], parts[2 * blockIdx.x + 1] = v[1];
}

// out[r][j] = relu(z), z = b[j] + sum_d W[j][d] x[r][d] for the tile's 16 rows; a thread owns one unit
// for 4 rows, so a weight row is read once per 4 rows.  st: the thread's share of {sum z, sum z^2}
// over the rows of the minibatch (valid[r]), cnt: the per-neuron dead counts.
__device__ __forceinline__ void rows_layer1(const float *__restrict__ W, const float *__restrict__ b,
                                            const float *__restrict__ x, int D, float *__restrict__ out, int H, int S,
                                            const int *__restrict__ frow, bool stats, double *st, unsigned *cnt)
{
    for (int e = threadIdx.x; e < 4 * H; e += 256) {
        const int rb = e / H, j = e - rb * H;
        const float *w = W + (size_t)j * D;
        const float *i0 = x + (size_t)(4 * rb) * D;
        float a[4];
        a[0] = a[1] = a[2] = a[3] = b[j];
#pragma unroll 4
        for (int d = 0; d < D; ++d) {
            const float wv = w[d];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = fmaf(wv, i0[i * D + d], a[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (stats && frow[4 * rb + i] >= 0) {
                st[0] += (double)a[i];
                st[1] += (double)a[i] * (double)a[i];
                if (act_dead(a[i])) atomicAdd(&cnt[j], 1u);     // integer: order-free
            }
            out[(size_t)(4 * rb + i) * S + j] = fmaxf(a[i], 0.0f);
        }
    }
}

// MASKED: the rows' loss is loss_row_masked over a.valid (gs_head.h), on the logits in LDS; everything
// else is the same code, so an invalid action's logit is formed and never read, and its dz is an exact 0
template <int AMAX, bool TWO, bool MASKED>
__global__ void __launch_bounds__(256) k_ppo_rows(RowsLayout L, RowsArgs a)
{
    extern __shared__ __align__(16) double lds_d[];
    if (a.stop && *a.stop != 0) return;      // the sticky KL stop: nothing is evaluated
    const int D = L.D, H1 = L.H1, H2 = TWO ? L.H2 : 0, A = L.A, A1 = A + 1, S1 = L.S1, S2 = L.S2;
    const int HK = TWO ? H2 : H1, SK = TWO ? S2 : S1;
    double *red = lds_d;
    double *rsum = red + kRowsRedDoubles;
    float *x = reinterpret_cast<float *>(rsum + R * kNumSums);
    float *h1 = x + R * D;
    float *g1 = h1 + R * S1;
    float *h2 = g1 + R * S1;
    float *g2 = h2 + (TWO ? R * S2 : 0);
    float *z = g2 + (TWO ? R * S2 : 0);
    float *dz = z + R * A1;
    float *fadv = dz + R * A1;
    float *folp = fadv + R, *fov = folp + R, *fret = fov + R;
    int *fact = reinterpret_cast<int *>(fret + R);
    int *frow = fact + R;
    unsigned *dead = reinterpret_cast<unsigned *>(frow + R);     // [H1 + H2]
    float *hk = TWO ? h2 : h1;           // what the heads read
    float *gk = TWO ? g2 : g1;           // and the gradient that flows back into it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lq = lane >> 4;
    const int TN = a.T * a.N;
    const float *P = a.P;
    const LossArgs &la = a.la;
    const bool stats = a.act_stats != 0;

    // batch normalisation of the advantages (utils/torch.py:97-99): the parts in part order
    float amean = 0.0f, aden = 1.0f;
    if (la.normalize) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < a.nparts; ++w) s0 += a.advparts[2 * w], s1 += a.advparts[2 * w + 1];
        const RowsMoments m = rows_moments(s0, s1, (double)a.B);
        amean = (float)m.mean;
        aden = (float)m.std + 1e-8f;
    }
    if (stats)
        for (int j = tid; j < H1 + H2; j += 256) dead[j] = 0u;

    double acc[kNumSums];
#pragma unroll
    for (int k = 0; k < kNumSums; ++k) acc[k] = 0.0;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    float *slot = a.slots + (size_t)blockIdx.x * a.stride;
    bool first = true;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        if (tid < R) {
            const int i = tile * R + tid;
            int row = -1, act = 0;
            float adv = 0.0f, olp = 0.0f, ov = 0.0f, ret = 0.0f;
            if (i < a.B) {
                row = sample_row(rows_sample(a.idx, i, TN), a.T, a.N);
                act = rows_action(a.actions[row], A);
                adv = a.advantages[row];
                if (la.normalize) adv = (adv - amean) / aden;
                olp = a.logprobs[row], ov = a.values[row], ret = a.returns[row];
            }
            frow[tid] = row, fact[tid] = act, fadv[tid] = adv, folp[tid] = olp, fov[tid] = ov, fret[tid] = ret;
        }
        __syncthreads();
        rows_gather_obs(a.obs, frow, D, x);
        __syncthreads();
        rows_layer1(P + L.oW1, P + L.ob1, x, D, h1, H1, S1, frow, stats, st, dead);
        __syncthreads();
        if constexpr (TWO) {
            // h2 = relu(h1 W2^T + b2): a wave owns 16-unit column tiles; a lane holds 4 consecutive k
            // of its row / unit per 16-wide chunk (one 16-byte load each), so a W2 element is read once
            // per tile of 16 rows
            for (int j0 = 16 * wave; j0 < H2; j0 += 64) {
                const float bias = P[L.ob2 + j0 + ln];
                f32x4 c0 = {bias, bias, bias, bias}, c1 = {0.0f, 0.0f, 0.0f, 0.0f};
                const float *wrow = P + L.oW2 + (size_t)(j0 + ln) * H1 + 4 * lq;
                const float *arow = h1 + ln * S1 + 4 * lq;
                // four chunks' loads in flight at a time (an L2 round trip per chunk otherwise), then
                // the chunks that are left
                int k0 = 0;
                for (; k0 + 64 <= H1; k0 += 64) {
                    float4 bv[4], av[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        bv[u] = *reinterpret_cast<const float4 *>(wrow + k0 + 16 * u);
                        av[u] = *reinterpret_cast<const float4 *>(arow + k0 + 16 * u);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        c0 = mfma4(av[u].x, bv[u].x, c0);
                        c1 = mfma4(av[u].y, bv[u].y, c1);
                        c0 = mfma4(av[u].z, bv[u].z, c0);
                        c1 = mfma4(av[u].w, bv[u].w, c1);
                    }
                }
                for (; k0 < H1; k0 += 16) {
                    const float4 bv = *reinterpret_cast<const float4 *>(wrow + k0);
                    const float4 av = *reinterpret_cast<const float4 *>(arow + k0);
                    c0 = mfma4(av.x, bv.x, c0);
                    c1 = mfma4(av.y, bv.y, c1);
                    c0 = mfma4(av.z, bv.z, c0);
                    c1 = mfma4(av.w, bv.w, c1);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 4 * lq + q;
                    const float zz = c0[q] + c1[q];
                    if (stats && frow[r] >= 0) {
                        st[2] += (double)zz;
                        st[3] += (double)zz * (double)zz;
                        if (act_dead(zz)) atomicAdd(&dead[H1 + j0 + ln], 1u);
                    }
                    h2[r * S2 + j0 + ln] = fmaxf(zz, 0.0f);
                }
            }
            __syncthreads();
        }
        // logits | value: a head column's 16 rows on 16 lanes (the weight is one broadcast load);
        // 16 (A + 1) elements are more than 256 from 16 actions on, hence the loop
        for (int e = tid; e < R * A1; e += 256) {
            const int c = e >> 4, r = e & 15;
            const float *w = P + L.head_row(c);
            const float *h = hk + r * SK;
            float s = P[L.head_bias(c)];
#pragma unroll 8
            for (int k = 0; k < HK; ++k) s = fmaf(w[k], h[k], s);
            z[r * A1 + c] = s;
        }
        __syncthreads();
        if (tid < R) {
            float *dzr = dz + tid * A1;
            if (frow[tid] >= 0) {
                if constexpr (MASKED) {      // the row's logits where they lie: the valid ones are read, no others
                    loss_row_masked(z + tid * A1, A, a.valid, fact[tid], folp[tid], fov[tid], fadv[tid], fret[tid], la,
                                    la.inv_batch, dzr, acc);
                } else {
                    float zr[AMAX + 1];
#pragma unroll
                    for (int c = 0; c < AMAX + 1; ++c) zr[c] = c < A1 ? z[tid * A1 + c] : 0.0f;
                    loss_row<AMAX>(zr, A, fact[tid], folp[tid], fov[tid], fadv[tid], fret[tid], la, la.inv_batch, dzr, acc);
                }
            } else {
                for (int c = 0; c < A1; ++c) dzr[c] = 0.0f;    // a ragged tile's rows past the minibatch
            }
        }
        __syncthreads();
        // back through the heads and the ReLU: a thread owns one unit for 4 rows
        for (int e = tid; e < 4 * HK; e += 256) {
            const int rb = e / HK, k = e - rb * HK;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
            for (int c = 0; c < A1; ++c) {
                const float wv = P[L.head_row(c) + k];
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = fmaf(dz[(4 * rb + i) * A1 + c], wv, s[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = (4 * rb + i) * SK + k;
                gk[o] = hk[o] > 0.0f ? s[i] : 0.0f;
            }
        }
        // the heads' gradient
        for (int e = tid; e < A1 * HK + A1; e += 256) {
            float s = 0.0f;
            int p;
            if (e < A1 * HK) {
                const int c = e / HK, k = e - c * HK;
#pragma unroll
                for (int r = 0; r < R; ++r) s = fmaf(dz[r * A1 + c], hk[r * SK + k], s);
                p = L.head_row(c) + k;
            } else {
                const int c = e - A1 * HK;
#pragma unroll
                for (int r = 0; r < R; ++r) s += dz[r * A1 + c];
                p = L.head_bias(c);
            }
            slot[p] = first ? s : slot[p] + s;
        }
        __syncthreads();
        if constexpr (TWO) {
            // dh1 = (dh2 W2) through h1's ReLU: a wave owns 16-unit column tiles of h1; W2 is read
            // along its rows (16 consecutive k1 per unit j), once per tile of 16 rows
            for (int k0 = 16 * wave; k0 < H1; k0 += 64) {
                f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0;
                const float *arow = g2 + ln * S2 + 4 * lq;
                const float *wcol = P + L.oW2 + (size_t)(4 * lq) * H1 + k0 + ln;
                int j0 = 0;
                for (; j0 + 64 <= H2; j0 += 64) {       // four chunks' loads in flight, as in the forward
                    float4 av[4];
                    float bw[4][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        av[u] = *reinterpret_cast<const float4 *>(arow + j0 + 16 * u);
                        const float *w = wcol + (size_t)(j0 + 16 * u) * H1;
#pragma unroll
                        for (int s = 0; s < 4; ++s) bw[u][s] = w[(size_t)s * H1];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        c0 = mfma4(av[u].x, bw[u][0], c0);
                        c1 = mfma4(av[u].y, bw[u][1], c1);
                        c0 = mfma4(av[u].z, bw[u][2], c0);
                        c1 = mfma4(av[u].w, bw[u][3], c1);
                    }
                }
                for (; j0 < H2; j0 += 16) {
                    const float4 av = *reinterpret_cast<const float4 *>(arow + j0);
                    const float *w = wcol + (size_t)j0 * H1;
                    const float b0 = w[0], b1 = w[H1], b2 = w[2 * H1], b3 = w[3 * H1];
                    c0 = mfma4(av.x, b0, c0);
                    c1 = mfma4(av.y, b1, c1);
                    c0 = mfma4(av.z, b2, c0);
                    c1 = mfma4(av.w, b3, c1);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int o = (4 * lq + q) * S1 + k0 + ln;
                    g1[o] = h1[o] > 0.0f ? c0[q] + c1[q] : 0.0f;
                }
            }
            // dW2 = dh2^T h1 into the workgroup's own slot (mlp_medium's W2 does not fit LDS): the 16
            // rows are the product's K; a wave owns 16 units j and walks h1's column tiles two at a
            // time, the slot's previous value riding in as the accumulator
            for (int j0 = 16 * wave; j0 < H2; j0 += 64) {
                float av[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) av[s] = g2[(4 * s + lq) * S2 + j0 + ln];
                for (int k0 = 0; k0 < H1; k0 += 32) {
                    const bool two_tiles = k0 + 16 < H1;
                    float *o0 = slot + L.oW2 + (size_t)(j0 + 4 * lq) * H1 + k0 + ln;
                    float *o1 = o0 + 16;
                    float b0[4], b1[4];
                    f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        b0[s] = h1[(4 * s + lq) * S1 + k0 + ln];
                        b1[s] = two_tiles ? h1[(4 * s + lq) * S1 + k0 + 16 + ln] : 0.0f;
                    }
                    if (!first) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            c0[q] = o0[(size_t)q * H1];
                            if (two_tiles) c1[q] = o1[(size_t)q * H1];
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        c0 = mfma4(av[s], b0[s], c0);
                        c1 = mfma4(av[s], b1[s], c1);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        o0[(size_t)q * H1] = c0[q];
                        if (two_tiles) o1[(size_t)q * H1] = c1[q];
                    }
                }
            }
            for (int j = tid; j < H2; j += 256) {
                float s = 0.0f;
#pragma unroll
                for (int r = 0; r < R; ++r) s += g2[r * S2 + j];
                slot[L.ob2 + j] = first ? s : slot[L.ob2 + j] + s;
            }
            __syncthreads();
        }
        // dW1 | db1
        for (int e = tid; e < H1 * D + H1; e += 256) {
            float s = 0.0f;
            int p;
            if (e < H1 * D) {
                const int j = e / D, d = e - j * D;
#pragma unroll
                for (int r = 0; r < R; ++r) s = fmaf(g1[r * S1 + j], x[r * D + d], s);
                p = L.oW1 + e;
            } else {
                const int j = e - H1 * D;
#pragma unroll
                for (int r = 0; r < R; ++r) s += g1[r * S1 + j];
                p = L.ob1 + j;
            }
            slot[p] = first ? s : slot[p] + s;
        }
        first = false;
        __syncthreads();
    }
    rows_store_sums(acc, rsum, a.msums + (size_t)blockIdx.x * kNumSums);
    if (stats) {
        block_reduce<4, double>(st, red);
        if (tid < 4) a.actsums[(size_t)blockIdx.x * 4 + tid] = st[tid];
        for (int j = tid; j < H1 + H2; j += 256) a.dead[(size_t)blockIdx.x * (H1 + H2) + j] = dead[j];
    }
}

// whether the minibatch's approx_kl passed the target: write_metrics' expression on the sums added
// in workgroup order, so the row, sum and step kernels of a step all decide alike
__device__ __forceinline__ bool rows_tripped(const double *msums, int groups, int B, float target_kl)
{
    double s = 0.0;
    for (int w = 0; w < groups; ++w) s += msums[(size_t)w * kNumSums + 6];
    return (float)(s / (double)B) > target_kl;
}

__global__ void __launch_bounds__(256) k_ppo_rows_sum(RowsLayout L, RowsStepArgs a)
{
    __shared__ double red[3 * (256 + 16)];
    __shared__ int s_trip;
    const int tid = threadIdx.x;
    if (a.stop) {
        if (*a.stop != 0) return;
        if (tid == 0) s_trip = rows_tripped(a.msums, a.groups, a.B, a.la.target_kl) ? 1 : 0;
        __syncthreads();
        if (s_trip) return;          // the gradient of the last applied step stays
    }
    double sq[3] = {0.0, 0.0, 0.0};
    for (int p = blockIdx.x * 256 + tid; p < L.P; p += gridDim.x * 256) {
        float g = 0.0f;
#pragma unroll 8
        for (int w = 0; w < a.groups; ++w) g += a.slots[(size_t)w * a.stride + p];
        a.G[p] = g;
        sq[p >= L.oWv ? 2 : (p >= L.oWp ? 1 : 0)] += (double)g * (double)g;
    }
    block_reduce<3, double>(sq, red);
    if (tid < 3) a.normparts[3 * blockIdx.x + tid] = sq[tid];
}

// OPT: the optimizer of the step (gs_head.h opt_param); SGD touches neither M nor V
template <int OPT>
__global__ void __launch_bounds__(256) k_ppo_rows_step(RowsLayout L, RowsStepArgs a)
{
    __shared__ double tot[16];
    __shared__ double nrm[4];
    __shared__ double ast[4];
    __shared__ unsigned cnt[4];      // per layer {sum, max} of the per-neuron dead counts
    __shared__ int s_trip;
    const int tid = threadIdx.x;
    float *rec = a.metrics;
    if (a.stop && *a.stop != 0) {    // stopped before this step: never evaluated
        if (blockIdx.x == 0 && tid < GS_NUM_METRICS) rec[tid] = unevaluated_slot(tid);
        return;
    }
    if (tid == 0) s_trip = a.stop && rows_tripped(a.msums, a.groups, a.B, a.la.target_kl) ? 1 : 0;
    __syncthreads();
    const bool tripped = s_trip != 0;
    if (tid < 3 && !tripped) {
        double s = 0.0;
        for (int w = 0; w < a.nsum; ++w) s += a.normparts[3 * w + tid];
        nrm[tid] = s;
    }
    if (blockIdx.x == 0) {
        if (tid >= 64 && tid < 64 + kNumSums) {
            const int k = tid - 64;
            double s = 0.0;
            for (int w = 0; w < a.groups; ++w) s += a.msums[(size_t)w * kNumSums + k];
            tot[k] = s;
        }
        if (tid >= 128 && tid < 132) {
            double s = 0.0;
            if (a.act_stats)
                for (int w = 0; w < a.groups; ++w) s += a.actsums[(size_t)w * 4 + (tid - 128)];
            ast[tid - 128] = s;
            cnt[tid - 128] = 0u;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && a.act_stats) {
        const int HH = L.H1 + L.H2;
        for (int j = tid; j < HH; j += 256) {
            unsigned c = 0u;
            for (int w = 0; w < a.groups; ++w) c += a.dead[(size_t)w * HH + j];
            const int l = j >= L.H1 ? 1 : 0;
            atomicAdd(&cnt[2 * l], c);       // integers: order-free; a layer's counts sum to B H <= 2^29
            atomicMax(&cnt[2 * l + 1], c);
        }
        __syncthreads();
    }
    const float total = tripped ? 0.0f : (float)sqrt(nrm[0] + nrm[1] + nrm[2]);
    if (blockIdx.x == 0 && tid == 0) {
        write_metrics(tot, (double)a.B, a.la, rec, true);
        write_step_tail(rec, total, tripped ? 0.0f : (float)sqrt(nrm[0]), tripped ? 0.0f : (float)sqrt(nrm[1]),
                        tripped ? 0.0f : (float)sqrt(nrm[2]));
        if (a.act_stats) {
            const int nl = L.two ? 2 : 1;
            for (int l = 0; l < nl; ++l) {
                const double n = (double)a.B * (double)(l ? L.H2 : L.H1);
                act_quad(ast[2 * l], ast[2 * l + 1], (double)cnt[2 * l], (double)cnt[2 * l + 1], n, (double)a.B,
                         rec + GS_M_ACT + 4 * l);
            }
        }
        if (tripped) *a.stop = 1;    // the other workgroups return below whichever value they read
    }
    if (!a.do_step || tripped) return;
    const float coef = clip_coef(total, a.aa);
    for (int p = blockIdx.x * 256 + tid; p < L.P; p += gridDim.x * 256) {
        float mm = 0.0f, vv = 0.0f, pp = a.P[p];
        if constexpr (OPT != kOptSGD) mm = a.M[p], vv = a.V[p];
        a.G[p] = opt_param<OPT>(a.G[p], coef, mm, vv, pp, a.aa, a.aa.neg_step_size, a.aa.inv_bc2_sqrt);
        if constexpr (OPT != kOptSGD) a.M[p] = mm, a.V[p] = vv;
        a.P[p] = pp;
    }
}

// ------------------------------------------------------------------------------------------------
struct RowsWorkspace {
    double *advparts, *normparts, *msums, *actsums;
    uint32_t *dead;
    float *slots;
    int groups, ntiles, stride, nparts, chunk, nsum;
    size_t bytes;
};

RowsWorkspace rows_carve(void *base, const RowsLayout &L, int64_t B)
{
    RowsWorkspace w{};
    w.ntiles = (int)((B + R - 1) / R);
    w.groups = std::min(w.ntiles, kRowsMaxGroups);
    w.stride = (L.P + 3) & ~3;
    w.nparts = (int)std::min<int64_t>(kRowsAdvParts, (B + 255) / 256);
    w.chunk = (int)((B + w.nparts - 1) / w.nparts);
    w.nsum = std::min(kRowsSumGroups, (L.P + 255) / 256);
    RowsCarver c{(char *)base};
    w.advparts = c.take<double>(2 * kRowsAdvParts);
    w.normparts = c.take<double>(3 * kRowsSumGroups);
    w.msums = c.take<double>(kNumSums * (size_t)w.groups);
    w.actsums = c.take<double>(4 * (size_t)w.groups);
    w.dead = c.take<uint32_t>((size_t)(L.H1 + L.H2) * w.groups);
    w.slots = c.take<float>((size_t)w.groups * w.stride);
    w.bytes = c.bytes;
    return w;
}

int rows_check_dims(const gs_mlp_dims &d, const char *what)
{
    GS_REQUIRE(d.obs_dim > 0 && d.obs_dim <= kMaxObsDim, "%s: obs_dim %d outside [1, %d]", what, d.obs_dim, kMaxObsDim);
    GS_REQUIRE(d.hidden1 >= kTile && d.hidden1 <= kRowsMaxHidden && d.hidden1 % kTile == 0,
               "%s: hidden1 %d must be a multiple of 16 in [16, %d]", what, d.hidden1, kRowsMaxHidden);
    GS_REQUIRE(d.hidden2 == 0 || (d.hidden2 >= kTile && d.hidden2 <= kRowsMaxHidden && d.hidden2 % kTile == 0),
               "%s: hidden2 %d must be 0 (one hidden layer) or a multiple of 16 in [16, %d]", what, d.hidden2,
               kRowsMaxHidden);
    GS_REQUIRE(d.n_actions > 0 && d.n_actions <= kMaxActions, "%s: n_actions %d outside [1, %d]", what, d.n_actions,
               kMaxActions);
    return GS_OK;
}

template <class F>
int rows_dispatch(const RowsLayout &L, F &&f)
{
    return with_amax(L.A, [&](auto amax) { return L.two ? f(amax, std::true_type{}) : f(amax, std::false_type{}); });
}

// valid_mask: 0 = the unmasked head (k_ppo_rows<.., false>, the code of gs_ppo_rows_update / _loss)
int rows_run(float *params, float *grads, float *adam_m, float *adam_v, const gs_mlp_dims &dims, const gs_ppo_hparams &hp,
             const gs_rollout_view &ro, const int32_t *idx, int64_t batch, int64_t n, int64_t adam_step0, float *metrics,
             int32_t *stop_flag, void *workspace, size_t workspace_bytes, bool do_step, hipStream_t s, const char *what,
             uint32_t valid_mask = 0u)
{
    if (do_step) GS_REQUIRE_OPT_FLAGS(hp.flags, what);
    int rc = rows_check_dims(dims, what);
    if (rc) return rc;
    // the shift is undefined at 32 actions, where every bit names an action
    GS_REQUIRE(dims.n_actions == 32 || (valid_mask >> dims.n_actions) == 0u, "%s: valid_mask 0x%x has bits past "
               "n_actions %d", what, valid_mask, dims.n_actions);
    GS_REQUIRE(!(hp.flags & GS_HP_BF16), "%s: precision bf16 is a mode of the fused chain; the row-parallel update is "
                                         "fp32 only", what);
    if ((rc = rows_check_batch(batch, ro.T, ro.N, what))) return rc;
    const RowsLayout L = rows_layout(dims);
    const RowsWorkspace ws = rows_carve(workspace, L, batch);
    GS_REQUIRE(workspace_bytes >= ws.bytes, "%s: workspace of %zu bytes, gs_ppo_rows_workspace_bytes asks for %zu", what,
               workspace_bytes, ws.bytes);
    GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
    const size_t lds = rows_lds_bytes(L);
    GS_REQUIRE(lds + kRowsStaticLds <= kLdsBudget, "%s: a row tile of this shape needs %zu bytes of LDS (static + dynamic), "
               "more than a workgroup's %zu", what, lds + kRowsStaticLds, kLdsBudget);
    GS_REQUIRE(ro.obs && ro.actions && ro.logprobs && ro.values && ro.advantages && ro.returns,
               "%s: the rollout view has a null buffer", what);
    GS_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && adam_step0 >= 0, "%s: bad n_minibatches / adam_step0", what);
    GS_REQUIRE(params && grads && idx && metrics && workspace && (!do_step || (adam_m && adam_v)), "%s: null buffer", what);
    GS_REQUIRE(((uintptr_t)params & 15) == 0, "%s: the parameters must be 16-byte aligned", what);
    const bool kl_on = do_step && hp.target_kl > 0.0f;
    GS_REQUIRE(!kl_on || stop_flag, "%s: target_kl needs the stop flag", what);
    const double b1 = hp.adam_beta1, b2 = hp.adam_beta2;
    GS_REQUIRE(!do_step || (b1 > 0.0 && b1 < 1.0 && b2 > 0.0 && b2 < 1.0), "%s: Adam betas must lie in (0, 1)", what);
    if (n == 0) return GS_OK;
    LossArgs la = loss_args(hp);
    la.batch_rows = (int)batch;
    la.inv_batch = 1.0f / (float)batch;
    const int act_stats = (hp.flags & GS_HP_ACT_STATS) ? 1 : 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t *idxk = idx + k * batch;
        if (la.normalize) {
            hipLaunchKernelGGL(k_ppo_rows_adv, dim3((unsigned)ws.nparts), dim3(256), 0, s, idxk, ro.advantages, (int)ro.T,
                               (int)ro.N, (int)batch, ws.chunk, ws.advparts);
            GS_LAUNCH_CHECK("k_ppo_rows_adv");
        }
        RowsArgs ra{};
        ra.P = params, ra.slots = ws.slots, ra.msums = ws.msums, ra.actsums = ws.actsums, ra.dead = ws.dead;
        ra.advparts = ws.advparts;
        ra.obs = ro.obs, ra.actions = ro.actions, ra.logprobs = ro.logprobs, ra.values = ro.values;
        ra.advantages = ro.advantages, ra.returns = ro.returns;
        ra.idx = idxk;
        ra.stop = kl_on ? stop_flag : nullptr;      // target_kl unset: the flag is neither read nor written
        ra.T = (int)ro.T, ra.N = (int)ro.N, ra.B = (int)batch, ra.ntiles = ws.ntiles, ra.stride = ws.stride;
        ra.nparts = ws.nparts, ra.act_stats = act_stats;
        ra.la = la;
        ra.valid = valid_mask;
        rc = rows_dispatch(L, [&](auto amax, auto two) {
            constexpr int AMAX = decltype(amax)::value;
            constexpr bool TWO = decltype(two)::value;
            auto launch = [&](auto masked) {
                constexpr bool MASKED = decltype(masked)::value;
                const int rl = set_lds_limit((const void *)k_ppo_rows<AMAX, TWO, MASKED>, lds);
                if (rl) return rl;
                hipLaunchKernelGGL((k_ppo_rows<AMAX, TWO, MASKED>), dim3((unsigned)ws.groups), dim3(256), lds, s, L, ra);
                GS_LAUNCH_CHECK("k_ppo_rows");
                return (int)GS_OK;
            };
            return valid_mask != 0u ? launch(std::true_type{}) : launch(std::false_type{});
        });
        if (rc) return rc;
        RowsStepArgs sa{};
        sa.P = params, sa.G = grads, sa.M = adam_m, sa.V = adam_v;
        sa.slots = ws.slots, sa.msums = ws.msums, sa.actsums = ws.actsums, sa.dead = ws.dead, sa.normparts = ws.normparts;
        sa.metrics = metrics + k * GS_NUM_METRICS;
        sa.stop = kl_on ? stop_flag : nullptr;
        sa.groups = ws.groups, sa.stride = ws.stride, sa.B = (int)batch, sa.nsum = ws.nsum, sa.act_stats = act_stats;
        sa.do_step = do_step ? 1 : 0;
        sa.la = la;
        if (do_step) sa.aa = adam_args(hp, adam_step0 + k + 1);
        hipLaunchKernelGGL(k_ppo_rows_sum, dim3((unsigned)ws.nsum), dim3(256), 0, s, L, sa);
        GS_LAUNCH_CHECK("k_ppo_rows_sum");
        rc = with_opt(sa.aa.opt, [&](auto opt) {
            hipLaunchKernelGGL(k_ppo_rows_step<decltype(opt)::value>, dim3(do_step ? (unsigned)ws.nsum : 1u), dim3(256), 0,
                               s, L, sa);
            GS_LAUNCH_CHECK("k_ppo_rows_step");
            return (int)GS_OK;
        });
        if (rc) return rc;
    }
    return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" size_t gs_ppo_rows_workspace_bytes(gs_mlp_dims dims, int64_t batch)
{
    using namespace gs;
    if (rows_check_dims(dims, "gs_ppo_rows_workspace_bytes") != GS_OK || !rows_batch_ok(batch)) return 0;
    const RowsLayout L = rows_layout(dims);
    if (rows_lds_bytes(L) + kRowsStaticLds > kLdsBudget) return 0;
    return rows_carve(nullptr, L, batch).bytes;
}

extern "C" int gs_ppo_rows_update(float *params, float *grads, float *adam_m, float *adam_v, gs_mlp_dims dims,
                                  gs_ppo_hparams hp, gs_rollout_view ro, const int32_t *idx, int64_t batch,
                                  int64_t n_minibatches, int64_t adam_step0, float *metrics, int32_t *stop_flag,
                                  void *workspace, size_t workspace_bytes, struct gs_comm *comm, void *stream)
{
    using namespace gs;
    GS_REQUIRE(comm == nullptr, "gs_ppo_rows_update: the row-parallel update has no gradient exchange, a communicator "
                                "is not supported (one GPU)");
    return rows_run(params, grads, adam_m, adam_v, dims, hp, ro, idx, batch, n_minibatches, adam_step0, metrics, stop_flag,
                    workspace, workspace_bytes, true, (hipStream_t)stream, "gs_ppo_rows_update");
}

extern "C" int gs_ppo_rows_loss(const float *params, float *grads, gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view ro,
                                const int32_t *idx, int64_t batch, float *metrics, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    using namespace gs;
    return rows_run(const_cast<float *>(params), grads, nullptr, nullptr, dims, hp, ro, idx, batch, 1, 0, metrics, nullptr,
                    workspace, workspace_bytes, false, (hipStream_t)stream, "gs_ppo_rows_loss");
}

// The masked twins (include/gsamd.h): valid_mask bit a set = action a valid, 0 = no mask (the entries above)
extern "C" int gs_ppo_rows_update_masked(float *params, float *grads, float *adam_m, float *adam_v, gs_mlp_dims dims,
                                         gs_ppo_hparams hp, gs_rollout_view ro, const int32_t *idx, int64_t batch,
                                         int64_t n_minibatches, int64_t adam_step0, float *metrics, int32_t *stop_flag,
                                         void *workspace, size_t workspace_bytes, struct gs_comm *comm, void *stream,
                                         uint32_t valid_mask)
{
    using namespace gs;
    GS_REQUIRE(comm == nullptr, "gs_ppo_rows_update_masked: the row-parallel update has no gradient exchange, a "
                                "communicator is not supported (one GPU)");
    return rows_run(params, grads, adam_m, adam_v, dims, hp, ro, idx, batch, n_minibatches, adam_step0, metrics, stop_flag,
                    workspace, workspace_bytes, true, (hipStream_t)stream, "gs_ppo_rows_update_masked", valid_mask);
}

extern "C" int gs_ppo_rows_loss_masked(const float *params, float *grads, gs_mlp_dims dims, gs_ppo_hparams hp,
                                       gs_rollout_view ro, const int32_t *idx, int64_t batch, float *metrics,
                                       void *workspace, size_t workspace_bytes, void *stream, uint32_t valid_mask)
{
    using namespace gs;
    return rows_run(const_cast<float *>(params), grads, nullptr, nullptr, dims, hp, ro, idx, batch, 1, 0, metrics, nullptr,
                    workspace, workspace_bytes, false, (hipStream_t)stream, "gs_ppo_rows_loss_masked", valid_mask);
}
