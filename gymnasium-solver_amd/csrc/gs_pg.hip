// gs_pg.hip — the REINFORCE update (gs_pg_update / gs_pg_loss): REINFORCEAgent.losses_for_batch
// (agents/reinforce/reinforce_agent.py:11-88) + BaseAgent._backpropagate_and_step on minibatches
// of up to 2^20 rows, fp32, one GPU.  Two launches per optimizer step:
//   k_pg_rows  workgroups own 16-row tiles (looping when there are more tiles than workgroups):
//              gather by idx, obs -> h1 -> h2 -> logits, the row loss, dz -> dh2, dW2, dh1, dW1 and
//              the biases; a workgroup adds its tiles' gradient share into its own partial slot
//              (HBM, one writer) and leaves its metric sums beside it
//   k_pg_step  sums the slots in workgroup order into the flat gradient, takes the backbone /
//              policy-head / total norms in a fixed order, clips and runs Adam on the backbone and
//              the policy head.  The value head is outside the loss (its gradient is None in the
//              reference): its parameters and moments are never written.
// Every reduction has a fixed order; the only atomic is the integer ticket by which the step
// kernel's last workgroup is chosen.  That one workgroup also runs Adam over all trained
// parameters (mlp_medium: 263 per thread) while the others have exited: the clip coefficient needs
// the whole norm, and spreading the step over the grid would take a grid-wide wait or a third
// launch; the slot sums before it (groups x P loads) are what the grid parallelises.
#include <math.h>

#include <algorithm>

#include "gs_hparams.h"
#include "gs_pg_head.h"
#include "gs_rows.h"

namespace gs {
namespace {

constexpr int R = kRowsTile;

struct PgRowArgs {
    const float *P;
    float *slots;            // [groups][stride] gradient partials
    double *msums;           // [groups][kPgSums] metric sums
    const float *obs;
    const int64_t *actions;
    const float *logprobs, *targets;
    const int32_t *idx;
    int T, N, B, ntiles, stride;
    int normalize;
    float ent_coef, invB;
};

struct PgStepArgs {
    float *P, *G, *M, *V;
    const float *slots;
    const double *msums;
    double *normpart;        // [step workgroups][2] {backbone, policy head} sums of squares
    unsigned *ticket;
    float *metrics;
    int groups, stride, B, normalize, do_step;
    float ent_coef;
    AdamArgs aa;
};

// out[r][j] = relu(b[j] + sum_k W[j][k] in[r][k]) for the tile's 16 rows; a thread owns one unit for
// 4 rows, so a weight row is read once per 4 rows
__device__ __forceinline__ void pg_dense_relu(const float *__restrict__ W, const float *__restrict__ b,
                                              const float *__restrict__ in, int K, float *__restrict__ out, int H)
{
    for (int e = threadIdx.x; e < 4 * H; e += 256) {
        const int rb = e / H, j = e - rb * H;
        const float *w = W + (size_t)j * K;
        const float *i0 = in + (size_t)(4 * rb) * K;
        float a0 = b[j], a1 = a0, a2 = a0, a3 = a0;
        for (int k = 0; k < K; ++k) {
            const float wv = w[k];
            a0 += wv * i0[k];
            a1 += wv * i0[K + k];
            a2 += wv * i0[2 * K + k];
            a3 += wv * i0[3 * K + k];
        }
        float *o = out + (size_t)(4 * rb) * H + j;
        o[0] = fmaxf(a0, 0.0f);
        o[H] = fmaxf(a1, 0.0f);
        o[2 * H] = fmaxf(a2, 0.0f);
        o[3 * H] = fmaxf(a3, 0.0f);
    }
}

__host__ __device__ inline size_t pg_lds_floats(const Layout &L)
{
    return (size_t)R * (L.D + 2 * L.H1 + 2 * L.H2 + 2 * L.A + 4);
}
constexpr size_t kPgLdsDoubles = 2 * (256 + 16) + (size_t)R * kPgSums;

template <int AMAX>
__global__ void __launch_bounds__(256) k_pg_rows(Layout L, PgRowArgs a)
{
    extern __shared__ double lds_d[];
    double *red = lds_d;
    double *rsum = red + 2 * (256 + 16);
    float *x = reinterpret_cast<float *>(rsum + R * kPgSums);
    const int D = L.D, H1 = L.H1, H2 = L.H2, A = L.A;
    float *h1 = x + R * D;
    float *h2 = h1 + R * H1;
    float *g1 = h2 + R * H2;
    float *g2 = g1 + R * H1;
    float *z = g2 + R * H2;
    float *dz = z + R * A;
    float *ft = dz + R * A;
    float *folp = ft + R;
    int *fact = reinterpret_cast<int *>(folp + R);
    int *frow = fact + R;
    const int tid = threadIdx.x;
    const int TN = a.T * a.N;
    const float *P = a.P;

    // batch normalisation of the targets (utils/torch.py:97-99): every workgroup takes the whole
    // minibatch's statistics itself, in the same order, so all of them hold the same bits
    float tmean = 0.0f, tden = 1.0f;
    if (a.normalize) {
        double v[2] = {0.0, 0.0};
        for (int i = tid; i < a.B; i += 256) {
            const float t = a.targets[sample_row(rows_sample(a.idx, i, TN), a.T, a.N)];
            v[0] += (double)t;
            v[1] += (double)t * (double)t;
        }
        block_reduce<2, double>(v, red);
        const RowsMoments m = rows_moments(v[0], v[1], (double)a.B);
        tmean = (float)m.mean;
        tden = (float)m.std + 1e-8f;
    }

    double acc[kPgSums];
#pragma unroll
    for (int k = 0; k < kPgSums; ++k) acc[k] = 0.0;
    float *slot = a.slots + (size_t)blockIdx.x * a.stride;
    bool first = true;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        if (tid < R) {
            const int i = tile * R + tid;
            int row = -1, act = 0;
            float t = 0.0f, olp = 0.0f;
            if (i < a.B) {
                row = sample_row(rows_sample(a.idx, i, TN), a.T, a.N);
                act = rows_action(a.actions[row], A);
                t = a.targets[row];
                if (a.normalize) t = (t - tmean) / tden;
                olp = a.logprobs[row];
            }
            frow[tid] = row, fact[tid] = act, ft[tid] = t, folp[tid] = olp;
        }
        __syncthreads();
        rows_gather_obs(a.obs, frow, D, x);
        __syncthreads();
        pg_dense_relu(P + L.oW1, P + L.ob1, x, D, h1, H1);
        __syncthreads();
        pg_dense_relu(P + L.oW2, P + L.ob2, h1, H1, h2, H2);
        __syncthreads();
        for (int e = tid; e < R * A; e += 256) {
            const int r = e / A, c = e - r * A;
            const float *w = P + L.oWp + (size_t)c * H2;
            const float *h = h2 + (size_t)r * H2;
            float s = P[L.obp + c];
            for (int k = 0; k < H2; ++k) s += w[k] * h[k];
            z[e] = s;
        }
        __syncthreads();
        if (tid < R) {
            float *dzr = dz + tid * A;
            if (frow[tid] >= 0) {
                float zr[AMAX + 1];
#pragma unroll
                for (int c = 0; c < AMAX + 1; ++c) zr[c] = c < A ? z[tid * A + c] : 0.0f;
                pg_loss_row<AMAX>(zr, A, fact[tid], folp[tid], ft[tid], a.ent_coef, a.invB, dzr, acc);
            } else {
                for (int c = 0; c < A; ++c) dzr[c] = 0.0f;     // a ragged tile's rows past the minibatch
            }
        }
        __syncthreads();
        // dh2 through the ReLU
        for (int e = tid; e < R * H2; e += 256) {
            const int r = e / H2, k = e - r * H2;
            float s = 0.0f;
            if (h2[e] > 0.0f)
                for (int c = 0; c < A; ++c) s += dz[r * A + c] * P[L.oWp + (size_t)c * H2 + k];
            g2[e] = s;
        }
        // policy head gradient
        for (int e = tid; e < A * H2 + A; e += 256) {
            float s = 0.0f;
            int64_t p;
            if (e < A * H2) {
                const int c = e / H2, k = e - c * H2;
                for (int r = 0; r < R; ++r) s += dz[r * A + c] * h2[r * H2 + k];
                p = L.oWp + e;
            } else {
                const int c = e - A * H2;
                for (int r = 0; r < R; ++r) s += dz[r * A + c];
                p = L.obp + c;
            }
            slot[p] = first ? s : slot[p] + s;
        }
        __syncthreads();
        // dh1 through the ReLU: W2 read along its rows (k across lanes), 4 rows per thread
        for (int e = tid; e < 4 * H1; e += 256) {
            const int rb = e / H1, k = e - rb * H1;
            const float *g = g2 + (size_t)(4 * rb) * H2;
            const float *w = P + L.oW2 + k;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            for (int j = 0; j < H2; ++j) {
                const float wv = w[(size_t)j * H1];
                s0 += g[j] * wv;
                s1 += g[H2 + j] * wv;
                s2 += g[2 * H2 + j] * wv;
                s3 += g[3 * H2 + j] * wv;
            }
            const float *hh = h1 + (size_t)(4 * rb) * H1 + k;
            float *o = g1 + (size_t)(4 * rb) * H1 + k;
            o[0] = hh[0] > 0.0f ? s0 : 0.0f;
            o[H1] = hh[H1] > 0.0f ? s1 : 0.0f;
            o[2 * H1] = hh[2 * H1] > 0.0f ? s2 : 0.0f;
            o[3 * H1] = hh[3 * H1] > 0.0f ? s3 : 0.0f;
        }
        // dW2 | db2: the workgroup's own slot, streamed (mlp_medium's W2 does not fit LDS)
        for (int e = tid; e < H2 * H1 + H2; e += 256) {
            float s = 0.0f;
            int64_t p;
            if (e < H2 * H1) {
                const int j = e / H1, k = e - j * H1;
                for (int r = 0; r < R; ++r) s += g2[r * H2 + j] * h1[r * H1 + k];
                p = L.oW2 + e;
            } else {
                const int j = e - H2 * H1;
                for (int r = 0; r < R; ++r) s += g2[r * H2 + j];
                p = L.ob2 + j;
            }
            slot[p] = first ? s : slot[p] + s;
        }
        __syncthreads();
        // dW1 | db1
        for (int e = tid; e < H1 * D + H1; e += 256) {
            float s = 0.0f;
            int64_t p;
            if (e < H1 * D) {
                const int j = e / D, d = e - j * D;
                for (int r = 0; r < R; ++r) s += g1[r * H1 + j] * x[r * D + d];
                p = L.oW1 + e;
            } else {
                const int j = e - H1 * D;
                for (int r = 0; r < R; ++r) s += g1[r * H1 + j];
                p = L.ob1 + j;
            }
            slot[p] = first ? s : slot[p] + s;
        }
        first = false;
        __syncthreads();
    }
    rows_store_sums(acc, rsum, a.msums + (size_t)blockIdx.x * kPgSums);
}

// OPT: the optimizer of the step (gs_head.h opt_param); SGD touches neither M nor V.  The value head
// (p >= nW) takes no step under any of them: the loss never reaches it, its .grad is None in the reference
template <int OPT>
__global__ void __launch_bounds__(256) k_pg_step(Layout L, PgStepArgs a)
{
    __shared__ double red[2 * (256 + 16)];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int nW = (int)L.oWv;       // backbone | policy head: what the loss reaches
    const int P = (int)L.P;
    double sq[2] = {0.0, 0.0};
    for (int p = blockIdx.x * 256 + tid; p < nW; p += gridDim.x * 256) {
        float g = 0.0f;
        for (int w = 0; w < a.groups; ++w) g += a.slots[(size_t)w * a.stride + p];
        a.G[p] = g;
        sq[p < (int)L.oWp ? 0 : 1] += (double)g * (double)g;
    }
    for (int p = nW + blockIdx.x * 256 + tid; p < P; p += gridDim.x * 256) a.G[p] = 0.0f;
    block_reduce<2, double>(sq, red);
    if (tid == 0) {
        a.normpart[2 * blockIdx.x] = sq[0];
        a.normpart[2 * blockIdx.x + 1] = sq[1];
    }
    // the last workgroup to arrive finishes the step; the parts it adds are in workgroup order,
    // so the result does not depend on which one that is
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double nb = 0.0, np = 0.0;
    for (unsigned w = 0; w < gridDim.x; ++w) {
        nb += a.normpart[2 * w];
        np += a.normpart[2 * w + 1];
    }
    const float total = (float)sqrt(nb + np);
    if (tid == 0) {
        *a.ticket = 0u;
        double t[kPgSums];
        for (int k = 0; k < kPgSums; ++k) {
            double s = 0.0;
            for (int w = 0; w < a.groups; ++w) s += a.msums[(size_t)w * kPgSums + k];
            t[k] = s;
        }
        const double Bd = (double)a.B;
        float *m = a.metrics;
        for (int k = 0; k < GS_NUM_METRICS; ++k) m[k] = 0.0f;
        const float pl = (float)(-t[0] / Bd);
        const float ent = (float)(t[1] / Bd);
        const RowsMoments tgt = rows_moments(t[4], t[5], Bd);
        const float tm = (float)tgt.mean, ts = (float)tgt.std;
        m[GS_M_LOSS] = pl + a.ent_coef * (-ent);
        m[GS_M_POLICY_LOSS] = pl;
        m[GS_M_ENTROPY] = ent;
        m[GS_M_KL] = (float)(t[2] / Bd);
        m[GS_M_APPROX_KL] = (float)(t[3] / Bd);
        m[GS_M_ADV_NORM_MEAN] = a.normalize ? tm : 0.0f;
        m[GS_M_ADV_NORM_STD] = a.normalize ? ts : 0.0f;
        m[GS_M_GRAD_NORM] = total;
        m[GS_M_GN_BACKBONE] = (float)sqrt(nb);
        m[GS_M_GN_POLICY_HEAD] = (float)sqrt(np);
        m[GS_M_PG_TARGET_MEAN] = tm;
        m[GS_M_PG_TARGET_STD] = ts;
    }
    if (!a.do_step) return;
    const float coef = clip_coef(total, a.aa);
    for (int p = tid; p < nW; p += 256) {
        float mm = 0.0f, vv = 0.0f, pp = a.P[p];
        if constexpr (OPT != kOptSGD) mm = a.M[p], vv = a.V[p];
        opt_param<OPT>(a.G[p], coef, mm, vv, pp, a.aa, a.aa.neg_step_size, a.aa.inv_bc2_sqrt);
        if constexpr (OPT != kOptSGD) a.M[p] = mm, a.V[p] = vv;
        a.P[p] = pp;
    }
}

struct PgWorkspace {
    unsigned *ticket;
    double *normpart, *msums;
    float *slots;
    int groups, ntiles, stride;
    size_t bytes;
};

PgWorkspace pg_carve(void *base, const Layout &L, int64_t B)
{
    PgWorkspace w{};
    w.ntiles = (int)((B + R - 1) / R);
    w.groups = w.ntiles < kPgMaxGroups ? w.ntiles : kPgMaxGroups;
    w.stride = (int)((L.P + 3) & ~(int64_t)3);
    RowsCarver c{(char *)base};
    w.ticket = c.take<unsigned>(1);
    w.normpart = c.take<double>(2 * kPgStepGroups);
    w.msums = c.take<double>(kPgSums * (size_t)w.groups);
    w.slots = c.take<float>((size_t)w.groups * w.stride);
    w.bytes = c.bytes;
    return w;
}

int pg_check_dims(const gs_mlp_dims &d)
{
    GS_REQUIRE(d.hidden2 != 0, "the REINFORCE update serves two hidden layers: one hidden layer (hidden2 == 0) is out "
                               "of scope");
    GS_REQUIRE(d.obs_dim > 0 && d.obs_dim <= kMaxObsDim, "obs_dim %d outside [1, %d]", d.obs_dim, kMaxObsDim);
    GS_REQUIRE(d.hidden1 > 0 && d.hidden1 <= kPgMaxHidden && d.hidden2 > 0 && d.hidden2 <= kPgMaxHidden,
               "hidden dims %d, %d outside [1, %d]", d.hidden1, d.hidden2, kPgMaxHidden);
    GS_REQUIRE(d.n_actions > 0 && d.n_actions <= kMaxActions, "n_actions %d outside [1, %d]", d.n_actions, kMaxActions);
    return GS_OK;
}

int pg_run(float *params, float *grads, float *adam_m, float *adam_v, const gs_mlp_dims &dims, const gs_pg_hparams &hp,
           const gs_rollout_view &ro, const int32_t *idx, int64_t batch, int64_t n, int64_t adam_step0, float *metrics,
           void *workspace, size_t workspace_bytes, bool do_step, hipStream_t s, const char *what)
{
    if (do_step) GS_REQUIRE_OPT_FLAGS(hp.flags, what);
    int rc = pg_check_dims(dims);
    if (rc) return rc;
    GS_REQUIRE(!(hp.flags & GS_HP_BF16), "%s: precision bf16 is a mode of the PPO chain; the REINFORCE update is fp32 "
                                         "only", what);
    if ((rc = rows_check_batch(batch, ro.T, ro.N, what))) return rc;
    GS_REQUIRE(ro.obs && ro.actions && ro.logprobs && ro.advantages,
               "%s: the rollout view needs obs, actions, logprobs and advantages (the policy targets)", what);
    GS_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && adam_step0 >= 0, "%s: bad n_minibatches / adam_step0", what);
    GS_REQUIRE(params && grads && idx && metrics && workspace && (!do_step || (adam_m && adam_v)), "%s: null buffer", what);
    GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
    const Layout L = Layout::make(dims.obs_dim, dims.hidden1, dims.hidden2, dims.n_actions);
    const PgWorkspace ws = pg_carve(workspace, L, batch);
    GS_REQUIRE(workspace_bytes >= ws.bytes, "%s: workspace of %zu bytes, gs_pg_update_workspace_bytes asks for %zu", what,
               workspace_bytes, ws.bytes);
    const double b1 = hp.adam_beta1, b2 = hp.adam_beta2;
    GS_REQUIRE(!do_step || (b1 > 0.0 && b1 < 1.0 && b2 > 0.0 && b2 < 1.0), "%s: Adam betas must lie in (0, 1)", what);
    if (n == 0) return GS_OK;
    const size_t lds = sizeof(double) * kPgLdsDoubles + sizeof(float) * pg_lds_floats(L);
    GS_REQUIRE(lds <= 160 * 1024, "%s: a row tile of this shape needs %zu bytes of LDS", what, lds);
    GS_HIP(hipMemsetAsync(ws.ticket, 0, sizeof(unsigned), s));
    const unsigned step_groups = (unsigned)std::min<int64_t>(kPgStepGroups, (L.oWv + 255) / 256);
    for (int64_t k = 0; k < n; ++k) {
        PgRowArgs ra{};
        ra.P = params, ra.slots = ws.slots, ra.msums = ws.msums;
        ra.obs = ro.obs, ra.actions = ro.actions, ra.logprobs = ro.logprobs, ra.targets = ro.advantages;
        ra.idx = idx + k * batch;
        ra.T = (int)ro.T, ra.N = (int)ro.N, ra.B = (int)batch, ra.ntiles = ws.ntiles, ra.stride = ws.stride;
        ra.normalize = hp.normalize_targets ? 1 : 0;
        ra.ent_coef = hp.ent_coef;
        ra.invB = 1.0f / (float)batch;
        rc = with_amax(L.A, [&](auto amax) {
            constexpr int AMAX = decltype(amax)::value;
            const int rl = set_lds_limit((const void *)k_pg_rows<AMAX>, lds);
            if (rl) return rl;
            hipLaunchKernelGGL(k_pg_rows<AMAX>, dim3((unsigned)ws.groups), dim3(256), lds, s, L, ra);
            GS_LAUNCH_CHECK("k_pg_rows");
            return (int)GS_OK;
        });
        if (rc) return rc;
        PgStepArgs sa{};
        sa.P = params, sa.G = grads, sa.M = adam_m, sa.V = adam_v;
        sa.slots = ws.slots, sa.msums = ws.msums, sa.normpart = ws.normpart, sa.ticket = ws.ticket;
        sa.metrics = metrics + k * GS_NUM_METRICS;
        sa.groups = ws.groups, sa.stride = ws.stride, sa.B = (int)batch, sa.normalize = ra.normalize;
        sa.do_step = do_step ? 1 : 0;
        sa.ent_coef = hp.ent_coef;
        if (do_step)
            sa.aa = adam_args(hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps, hp.max_grad_norm, adam_step0 + k + 1,
                              hp.flags);
        rc = with_opt(sa.aa.opt, [&](auto opt) {
            hipLaunchKernelGGL(k_pg_step<decltype(opt)::value>, dim3(step_groups), dim3(256), 0, s, L, sa);
            GS_LAUNCH_CHECK("k_pg_step");
            return (int)GS_OK;
        });
        if (rc) return rc;
    }
    return GS_OK;
}

}  // namespace
}  // namespace gs

extern "C" size_t gs_pg_update_workspace_bytes(gs_mlp_dims dims, int64_t batch)
{
    using namespace gs;
    if (pg_check_dims(dims) != GS_OK || !rows_batch_ok(batch)) return 0;
    return pg_carve(nullptr, Layout::make(dims.obs_dim, dims.hidden1, dims.hidden2, dims.n_actions), batch).bytes;
}

extern "C" int gs_pg_update(float *params, float *grads, float *adam_m, float *adam_v, gs_mlp_dims dims,
                            gs_pg_hparams hp, gs_rollout_view ro, const int32_t *idx, int64_t batch, int64_t n_minibatches,
                            int64_t adam_step0, float *metrics, void *workspace, size_t workspace_bytes,
                            struct gs_comm *comm, void *stream)
{
    using namespace gs;
    GS_REQUIRE(comm == nullptr, "gs_pg_update: the REINFORCE update has no gradient exchange, a communicator is not "
                                "supported (one GPU)");
    return pg_run(params, grads, adam_m, adam_v, dims, hp, ro, idx, batch, n_minibatches, adam_step0, metrics, workspace,
                  workspace_bytes, true, (hipStream_t)stream, "gs_pg_update");
}

extern "C" int gs_pg_loss(const float *params, float *grads, gs_mlp_dims dims, gs_pg_hparams hp, gs_rollout_view ro,
                          const int32_t *idx, int64_t batch, float *metrics, void *workspace, size_t workspace_bytes,
                          void *stream)
{
    using namespace gs;
    return pg_run(const_cast<float *>(params), grads, nullptr, nullptr, dims, hp, ro, idx, batch, 1, 0, metrics, workspace,
                  workspace_bytes, false, (hipStream_t)stream, "gs_pg_loss");
}
