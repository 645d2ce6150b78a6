// gs_mlp1.hip — the one-hidden-layer actor-critic (gs_mlp_dims.hidden2 == 0; the reference's
// mlp_tiny preset, utils/model_registry.py: one ReLU layer of 64 units) for gfx950.
//
// Reference ops replaced, as gs_mlp.hip does for two hidden layers:
//   MLPActorCritic.forward + Categorical sample / mode / log_prob   utils/models.py:328-346, policy_ops.py:14-42
//   PPOAgent.losses_for_batch                                       agents/ppo/ppo_agent.py:21-152
//   manual_backward + clip_grad_norm_ + Adam.step                   agents/base_agent.py:591-621
//
// These nets are a few hundred to a few thousand parameters, so the update is ONE launch of ONE
// 256-thread workgroup for all minibatches of a rollout: the parameters, both Adam moments and
// the gradient live in LDS from the prologue to the epilogue, and a minibatch costs barriers
// instead of kernel boundaries (no grid sync, no co-residency).  Rows are processed in tiles of
// kRows1, so the LDS footprint does not depend on the minibatch size; every sum runs in a fixed
// order (a thread owns its parameters' gradients and adds the rows in row order; the metric sums
// are added in row order by one thread per sum), so two runs of an update give the same bytes.
// The per-row head / loss / Adam arithmetic is gs_head.h's, shared with gs_mlp.hip.
#include "gs_common.h"
#include "gs_head.h"
#include "gs_hparams.h"
#include "gs_rollout1.h"
#include "gs_tabular_env.h"
#include "gs_cartpole_env.h"
#include "gs_acrobot_env.h"
#include "gs_mountaincar_env.h"
#include "gs_bandit_env.h"

namespace gs {

namespace {

constexpr int kRows1 = 32;                      // rows of one tile of the update
constexpr int kMaxBatch1 = 1024;                // largest minibatch (mlp1_update checks it)
constexpr size_t kLdsBudget1 = 160 * 1024;      // LDS of one CU (gfx950)
constexpr int kRedDoubles = 3 * (256 + 16);     // block_reduce<3, double> scratch
constexpr int kBlock1 = 8;                      // hidden units per block of the row forward (divides 16)

__host__ __device__ constexpr int round4i(int n) { return (n + 3) & ~3; }

// the update kernel's LDS carve-up (bytes): doubles first, then floats / ints
struct Lds1 {
    size_t o_red, o_rsum, o_tot, o_P, o_M, o_V, o_G, o_x, o_h, o_dh, o_z, o_f, o_dead, o_srow, o_sadv, bytes;
    size_t param_bytes, tile_bytes;
    __host__ __device__ static Lds1 make(size_t D, size_t H, size_t A)
    {
        Lds1 l{};
        const size_t P4 = (H * D + H + A * H + A + H + 1 + 3) & ~size_t(3), A1 = A + 1;
        size_t o = 0;
        l.o_red = o, o += sizeof(double) * kRedDoubles;
        l.o_rsum = o, o += sizeof(double) * kNumSums * kRows1;
        l.o_tot = o, o += sizeof(double) * 16;
        l.o_P = o, o += 4 * P4;
        l.o_M = o, o += 4 * P4;
        l.o_V = o, o += 4 * P4;
        l.o_G = o, o += 4 * P4;
        l.o_x = o, o += 4 * ((kRows1 * D + 3) & ~size_t(3));
        l.o_h = o, o += 4 * kRows1 * H;
        l.o_dh = o, o += 4 * kRows1 * H;
        l.o_z = o, o += 4 * ((kRows1 * A1 + 3) & ~size_t(3));
        l.o_f = o, o += 4 * 5 * kRows1;         // act | old logp | old value | adv | return
        l.o_dead = o, o += 4 * H;
        l.o_srow = o, o += 4 * kMaxBatch1;
        l.o_sadv = o, o += 4 * kMaxBatch1;
        l.bytes = o;
        l.param_bytes = 4 * P4;
        l.tile_bytes = o - 4 * 4 * P4;
        return l;
    }
};

struct Upd1Args {
    float *P, *G, *M, *V;
    const float *obs;
    const int64_t *actions;
    const float *logprobs, *values, *advantages, *returns;
    int T, N;
    const int32_t *idx;
    int B, n;
    int64_t step0;              // optimizer steps taken before this launch
    float *metrics;
    int32_t *stop;
    LossArgs la;
    AdamArgs aa;                // max_norm, the betas' float forms and eps; the schedule is per step, below
    double lr, ln_b1, ln_b2;    // Adam's bias corrections of step t: 1 - exp(t ln beta)
    int act_stats, loss_only;
};

// a sampler index outside the rollout reads row 0 instead of leaving the buffers
__device__ __forceinline__ int sample_row_checked(int s, int T, int N)
{
    return (unsigned)s < (unsigned)T * (unsigned)N ? sample_row(s, T, N) : 0;
}

// ------------------------------------------------------------------------------------
// The forward of one row, shared by k_act1 and k_rollout1 so their chains cannot drift: Ps the
// parameters in LDS (flat, Layout1's offsets), x the row's observation; z receives logits | value.
// h_k = relu(b1[k] + sum_d W1[k][d] x[d]) as one fmaf chain in d order from the bias;
// z[a] = bias + sum_k W[a][k] h[k] as one fmaf chain in k order: the update kernel forms the
// same chain, so a replayed row's log-prob equals the update's under the same parameters.
// ------------------------------------------------------------------------------------
template <int AMAX>
__device__ __forceinline__ void mlp1_forward_row(const float *Ps, const Layout1 &L, const float *x,
                                                 float (&z)[AMAX + 1])
{
    const int D = L.D, H = L.H, A = L.A;
    // Slots past the value head (a > A) run the value head's chain again and are never read: with
    // no condition inside the loops the head reads are plain loads the compiler batches, where a
    // guarded read became a branch per (k, a) and every fmaf waited for its own LDS round trip.
    int hr[AMAX + 1];
#pragma unroll
    for (int a = 0; a < AMAX + 1; ++a) {
        const int ac = a < A ? a : A;
        hr[a] = L.head_row(ac);
        z[a] = Ps[L.head_bias(ac)];
    }
    // kBlock1 hidden units at a time (H is a multiple of 16): their h chains are independent, so
    // the LDS reads of a block are issued together and the row waits for a read's latency once per
    // block, not once per fmaf; each h chain keeps its d order and each z[a] its k order
    for (int k0 = 0; k0 < H; k0 += kBlock1) {
        float h[kBlock1];
#pragma unroll
        for (int j = 0; j < kBlock1; ++j) h[j] = Ps[L.ob1 + k0 + j];
#pragma unroll 4
        for (int d = 0; d < D; ++d) {
            const float xd = x[d];
#pragma unroll
            for (int j = 0; j < kBlock1; ++j) h[j] = fmaf(Ps[L.oW1 + (k0 + j) * D + d], xd, h[j]);
        }
#pragma unroll
        for (int j = 0; j < kBlock1; ++j) {
            const float hj = h[j] > 0.0f ? h[j] : 0.0f;
#pragma unroll
            for (int a = 0; a < AMAX + 1; ++a) z[a] = fmaf(Ps[hr[a] + k0 + j], hj, z[a]);
        }
    }
}

// ------------------------------------------------------------------------------------
// k_act1: rollout step / value forward, one thread per env row, 256 rows per workgroup.
// LDS (floats): Ps[round4(P)] xs[256][D | 1]
// MASKED: head_act_row_masked over `valid` (gs_policy_act_masked); the unmasked kernel never reads
// its last argument.
// ------------------------------------------------------------------------------------
template <int AMAX, bool MASKED>
__global__ __launch_bounds__(256) void k_act1(const float *__restrict__ P, Layout1 L, const float *__restrict__ obs,
                                              int64_t N, int mode, uint64_t seed, uint64_t counter,
                                              int64_t *__restrict__ actions, float *__restrict__ logp,
                                              float *__restrict__ value, float *__restrict__ obs_store,
                                              const uint64_t *__restrict__ clock, uint32_t valid)
{
    extern __shared__ float lds_f[];
    float *Ps = lds_f;
    float *xs = Ps + round4i(L.P);
    const int tid = threadIdx.x, D = L.D, Dp = D | 1, A = L.A;
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    const int nr = (int)(N - row0 < 256 ? N - row0 : 256);
    for (int p = tid; p < L.P; p += 256) Ps[p] = P[p];
    for (int u = tid; u < nr * D; u += 256) {
        const int r = u / D, d = u - r * D;
        const float v = obs[row0 * D + u];
        xs[r * Dp + d] = v;
        if (obs_store) obs_store[row0 * D + u] = v;
    }
    __syncthreads();
    if (tid >= nr) return;
    float z[AMAX + 1];
    mlp1_forward_row<AMAX>(Ps, L, xs + tid * Dp, z);
    const int64_t r = row0 + tid;
    const uint64_t ctr = counter + (clock && mode == 0 ? clock[0] : 0ull);   // rollout clock (graph replay)
    if constexpr (MASKED)
        head_act_row_masked<AMAX>(z, A, valid, mode, seed, ctr, r, actions ? actions + r : nullptr,
                                  logp ? logp + r : nullptr, value ? value + r : nullptr);
    else
        head_act_row<AMAX>(z, A, mode, seed, ctr, r, actions ? actions + r : nullptr, logp ? logp + r : nullptr,
                           value ? value + r : nullptr);
}

// ------------------------------------------------------------------------------------
// k_rollout1: a whole rollout of a device env in one launch, generic over the env type E
// (gs_env_episode.h).  One thread owns one env for all T vector steps: the parameters sit in LDS,
// the env's state in the thread's registers, its observation in the thread's own LDS row, so the
// step loop has no barrier and no cross-thread arithmetic.  A workgroup is one wave
// (kRollout1Envs envs): a few dozen envs then spread over as many CUs as they can, and the result
// does not depend on the split.  The forward is k_act1's (mlp1_forward_row), the head
// head_act_row with counter0 + t and the env's row id, the env step E::step: every row, the env's
// tensors and the episode counters equal T rounds of k_act1 + k_env_step<E> bit for bit.
// LDS (floats): Ps[round4(P)] xs[kRollout1Envs][D | 1]
// ------------------------------------------------------------------------------------
template <int AMAX, class E>
__global__ __launch_bounds__(kRollout1Envs) void k_rollout1(const float *__restrict__ P, Layout1 L, int64_t N, int T,
                                                            int mode, uint64_t rng_seed, uint64_t counter0,
                                                            typename E::Args ev, RolloutRows rw)
{
    extern __shared__ float lds_f[];
    float *Ps = lds_f;
    float *xs = Ps + round4i(L.P);
    const int tid = threadIdx.x, D = L.D, Dp = D | 1, A = L.A;
    const int64_t me = (int64_t)blockIdx.x * kRollout1Envs + tid;
    const bool live = me < N;
    float *x = xs + tid * Dp;       // this env's observation: nobody else reads or writes the row
    // ---- prologue: the parameters into LDS once, the env into registers, its observation into the row
    for (int p = tid; p < L.P; p += kRollout1Envs) Ps[p] = P[p];
    E env{};
    if (live) {
        env.load(ev, me);
        for (int d = 0; d < D; ++d) x[d] = ev.obs[me * D + d];
    }
    __syncthreads();                // the parameters, staged by every lane
    if (!live) return;
    // replay reads the pre-filled action rows, one step ahead of its use
    int64_t action = mode == 2 && T > 0 ? rw.actions[me] : 0;
    for (int t = 0; t < T; ++t) {
        const int64_t o = (int64_t)t * N + me;
        float z[AMAX + 1];
        mlp1_forward_row<AMAX>(Ps, L, x, z);
        float logp, value;
        head_act_row<AMAX>(z, A, mode, rng_seed, counter0 + (uint64_t)t, me, &action, &logp, &value);
        const EnvStepOut so = env.step(ev, me, action);
        const int64_t taken = action;
        if (mode == 2 && t + 1 < T) action = rw.actions[o + N];
        // the step's rows behind the env's own loads, so no load of a step waits for its stores;
        // x is still the observation the action was taken on
        for (int d = 0; d < D; ++d) rw.obs[o * D + d] = x[d];
        if (mode != 2) rw.actions[o] = taken;
        rw.logp[o] = logp;
        rw.value[o] = value;
        rw.reward[o] = so.reward;
        rw.done[o] = so.done ? 1 : 0;
        rw.timeout[o] = so.timeout ? 1 : 0;
        env.write_obs(ev, x);
    }
    // ---- epilogue: the env's tensors and its observation back
    env.store(ev, me);
    for (int d = 0; d < D; ++d) ev.obs[me * D + d] = x[d];
}

// ------------------------------------------------------------------------------------
// k_update1: all n minibatch steps of an update in one workgroup (file header).
// ------------------------------------------------------------------------------------
// OPT: the optimizer of the steps (gs_head.h opt_param); SGD stages no moments into LDS and leaves a.M / a.V alone
template <int AMAX, int OPT = kOptAdam>
__global__ __launch_bounds__(256) void k_update1(Layout1 L, Upd1Args a)
{
    extern __shared__ double lds_d[];
    __shared__ int s_stop;
    __shared__ unsigned s_dead_max;
    const int tid = threadIdx.x, D = L.D, H = L.H, A = L.A, A1 = A + 1, NP = L.P, B = a.B;
    const Lds1 o = Lds1::make((size_t)D, (size_t)H, (size_t)A);
    char *base = reinterpret_cast<char *>(lds_d);
    double *dred = reinterpret_cast<double *>(base + o.o_red);
    double *rsum = reinterpret_cast<double *>(base + o.o_rsum);     // [kNumSums][kRows1]
    double *tot = reinterpret_cast<double *>(base + o.o_tot);       // [kNumSums]
    float *Ps = reinterpret_cast<float *>(base + o.o_P);
    float *Ms = reinterpret_cast<float *>(base + o.o_M);
    float *Vs = reinterpret_cast<float *>(base + o.o_V);
    float *Gs = reinterpret_cast<float *>(base + o.o_G);
    float *xs = reinterpret_cast<float *>(base + o.o_x);            // [kRows1][D]
    float *hs = reinterpret_cast<float *>(base + o.o_h);            // [kRows1][H] post-ReLU
    float *dhs = reinterpret_cast<float *>(base + o.o_dh);          // [kRows1][H] dLoss/d(pre-activation)
    float *zl = reinterpret_cast<float *>(base + o.o_z);            // [kRows1][A1] logits | value, then their gradient
    float *f_olp = reinterpret_cast<float *>(base + o.o_f);
    float *f_ov = f_olp + kRows1, *f_adv = f_ov + kRows1, *f_ret = f_adv + kRows1;
    int *f_act = reinterpret_cast<int *>(f_ret + kRows1);
    unsigned *dead = reinterpret_cast<unsigned *>(base + o.o_dead); // [H] rows with |z| < 1e-6 per neuron
    int *srow = reinterpret_cast<int *>(base + o.o_srow);           // [kMaxBatch1] the minibatch's buffer rows
    float *sadv = reinterpret_cast<float *>(base + o.o_sadv);       // [kMaxBatch1] and their raw advantages

    const LossArgs &la = a.la;
    const bool kl_on = la.target_kl > 0.0f && a.stop != nullptr;
    const bool train = !a.loss_only;
    constexpr bool kMoments = OPT != kOptSGD;
    // ---- prologue: the optimizer state into LDS, once
    for (int p = tid; p < NP; p += 256) {
        Ps[p] = a.P[p];
        if (kMoments && train) {
            Ms[p] = a.M[p];
            Vs[p] = a.V[p];
        }
        Gs[p] = 0.0f;
    }
    if (tid == 0) s_stop = kl_on ? (*a.stop != 0 ? 1 : 0) : 0;
    const double rows = (double)la.batch_rows;
    const float invB = la.inv_batch;

    for (int k = 0; k < a.n; ++k) {
        float *rec = a.metrics + (int64_t)k * GS_NUM_METRICS;
        __syncthreads();        // the previous step's parameters and stop decision
        if (s_stop) {           // sticky KL stop: never evaluated
            if (tid < GS_NUM_METRICS)
                rec[tid] = unevaluated_slot(tid);
            continue;
        }
        const int32_t *idxk = a.idx + (int64_t)k * B;
        // the minibatch's buffer rows and advantages, staged once: the passes and tiles below then
        // start with one global round trip (the field itself), not two (index, then field)
        for (int r = tid; r < B; r += 256) {
            const int src = sample_row_checked(idxk[r], a.T, a.N);
            srow[r] = src;
            sadv[r] = a.advantages[src];
        }
        // ---- batch advantage normalisation: (a - mean) / (std_unbiased + 1e-8), k_loss's arithmetic
        // (a thread reads back its own staged rows: no barrier needed before the one below)
        float meanf = 0.0f, stdf = 1.0f;
        if (la.normalize) {
            double m1[1] = {0.0};
            for (int r = tid; r < B; r += 256) m1[0] += (double)sadv[r];
            block_reduce<1>(m1, dred);
            const double mean = m1[0] / (double)B;
            double q[1] = {0.0};
            for (int r = tid; r < B; r += 256) {
                const double dv = (double)sadv[r] - mean;
                q[0] += dv * dv;
            }
            block_reduce<1>(q, dred);
            meanf = (float)mean;
            stdf = (float)sqrt(q[0] / (double)(B - 1));
        }
        for (int p = tid; p < NP; p += 256) Gs[p] = 0.0f;
        if (tid < kNumSums) tot[tid] = 0.0;
        if (a.act_stats)
            for (int j = tid; j < H; j += 256) dead[j] = 0u;
        if (tid == 0) s_dead_max = 0u;
        double sz = 0.0, sz2 = 0.0;     // this thread's share of sum z, sum z^2 of backbone.0
        __syncthreads();

        for (int t0 = 0; t0 < B; t0 += kRows1) {
            const int nr = B - t0 < kRows1 ? B - t0 : kRows1;
            // (a) gather the tile's rows: observations and the minibatch fields
            for (int u = tid; u < kRows1 * D; u += 256) {
                const int r = u / D, d = u - r * D;
                xs[u] = r < nr ? a.obs[(int64_t)srow[t0 + r] * D + d] : 0.0f;
            }
            if (tid < nr) {
                const int src = srow[t0 + tid];
                f_act[tid] = (int)a.actions[src];
                f_olp[tid] = a.logprobs[src];
                f_ov[tid] = a.values[src];
                float adv = sadv[t0 + tid];
                if (la.normalize) adv = (adv - meanf) / (stdf + 1e-8f);
                f_adv[tid] = adv;
                f_ret[tid] = a.returns[src];
            }
            __syncthreads();
            // (b) hidden layer: h = relu(W1 x + b1), with backbone.0's pre-activation statistics
            for (int u = tid; u < kRows1 * H; u += 256) {
                const int r = u / H, j = u - r * H;
                float h = 0.0f;
                if (r < nr) {
                    float z = Ps[L.ob1 + j];
#pragma unroll 8
                    for (int d = 0; d < D; ++d) z = fmaf(Ps[L.oW1 + j * D + d], xs[r * D + d], z);
                    if (a.act_stats) {
                        sz += (double)z;
                        sz2 += (double)z * (double)z;
                        if (act_dead(z)) atomicAdd(&dead[j], 1u);   // integer: order-free
                    }
                    h = z > 0.0f ? z : 0.0f;
                }
                hs[u] = h;
            }
            __syncthreads();
            // (c) heads: logits | value, k_act1's fmaf chain
            for (int u = tid; u < nr * A1; u += 256) {
                const int r = u / A1, c = u - r * A1;
                float z = Ps[L.head_bias(c)];
                const float *w = Ps + L.head_row(c);
#pragma unroll 16
                for (int j = 0; j < H; ++j) z = fmaf(w[j], hs[r * H + j], z);
                zl[u] = z;
            }
            __syncthreads();
            // (d) loss rows: one thread per row; dLoss/dlogits | dLoss/dvalue replace the row's logits
            if (tid < nr) {
                float z[AMAX + 1];
#pragma unroll
                for (int c = 0; c < AMAX + 1; ++c) z[c] = c < A1 ? zl[tid * A1 + c] : 0.0f;
                double acc[kNumSums];
#pragma unroll
                for (int q = 0; q < kNumSums; ++q) acc[q] = 0.0;
                loss_row<AMAX>(z, A, f_act[tid], f_olp[tid], f_ov[tid], f_adv[tid], f_ret[tid], la, invB,
                               zl + tid * A1, acc);
#pragma unroll
                for (int q = 0; q < kNumSums; ++q) rsum[q * kRows1 + tid] = acc[q];
            }
            __syncthreads();
            if (tid < kNumSums) {       // the metric sums in row order
                double s = tot[tid];
#pragma unroll 16
                for (int r = 0; r < nr; ++r) s += rsum[tid * kRows1 + r];
                tot[tid] = s;
            }
            if (train) {
                // (e) back through the heads and the ReLU
                for (int u = tid; u < kRows1 * H; u += 256) {
                    const int r = u / H, j = u - r * H;
                    float g = 0.0f;
                    if (r < nr && hs[u] > 0.0f)
#pragma unroll 4
                        for (int c = 0; c < A1; ++c) g = fmaf(zl[r * A1 + c], Ps[L.head_row(c) + j], g);
                    dhs[u] = g;
                }
                __syncthreads();
                // (f) this thread's parameters' gradients, the tile's rows added in row order
                for (int p = tid; p < NP; p += 256) {
                    float g = 0.0f;
                    if (p < L.ob1) {                        // backbone.0.weight[j][d]
                        const int j = p / D, d = p - j * D;
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g = fmaf(dhs[r * H + j], xs[r * D + d], g);
                    } else if (p < L.oWp) {                 // backbone.0.bias[j]
                        const int j = p - L.ob1;
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g += dhs[r * H + j];
                    } else if (p < L.obp) {                 // policy_head.weight[c][j]
                        const int c = (p - L.oWp) / H, j = (p - L.oWp) - c * H;
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g = fmaf(zl[r * A1 + c], hs[r * H + j], g);
                    } else if (p < L.oWv) {                 // policy_head.bias[c]
                        const int c = p - L.obp;
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g += zl[r * A1 + c];
                    } else if (p < L.obv) {                 // value_head.weight[0][j]
                        const int j = p - L.oWv;
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g = fmaf(zl[r * A1 + A], hs[r * H + j], g);
                    } else {                                // value_head.bias
#pragma unroll 16
                        for (int r = 0; r < nr; ++r) g += zl[r * A1 + A];
                    }
                    Gs[p] += g;
                }
            }
            __syncthreads();    // the tile's staging is free again; tot is complete after the last tile
        }

        // ---- KL early stop (agents/base_agent.py:330-366): decided on the whole minibatch's loss
        const float approx_kl = (float)(tot[6] / rows);
        const bool tripped = la.target_kl > 0.0f && approx_kl > la.target_kl && a.stop != nullptr;
        const bool apply = train && !tripped;
        float total = 0.0f, gn_pol = 0.0f, gn_val = 0.0f, gn_back = 0.0f;
        if (apply) {
            // ---- pre-clip norms: the total and the three components (utils/models.py:196-230)
            double ss[3] = {0.0, 0.0, 0.0};
            for (int p = tid; p < NP; p += 256) {
                const double g = (double)Gs[p];
                ss[0] += g * g;
                if (p >= L.oWv) ss[2] += g * g;
                else if (p >= L.oWp) ss[1] += g * g;
            }
            block_reduce<3>(ss, dred);
            total = (float)sqrt(ss[0]);
            gn_pol = (float)sqrt(ss[1]);
            gn_val = (float)sqrt(ss[2]);
            gn_back = (float)sqrt(fmax(0.0, ss[0] - ss[1] - ss[2]));
            const float coef = clip_coef(total, a.aa);
            // ---- Adam at step t (torch.optim.Adam's bias corrections, formed in double)
            const double t = (double)(a.step0 + k + 1);
            const double bc1 = 1.0 - exp(t * a.ln_b1), bc2 = 1.0 - exp(t * a.ln_b2);
            const float neg_step = (float)(-a.lr / bc1);
            const float inv_bc2s = (float)(1.0 / sqrt(bc2));
            for (int p = tid; p < NP; p += 256) {
                float m = 0.0f, v = 0.0f, w = Ps[p];
                if constexpr (kMoments) m = Ms[p], v = Vs[p];
                const float g = opt_param<OPT>(Gs[p], coef, m, v, w, a.aa, neg_step, inv_bc2s);
                if constexpr (kMoments) Ms[p] = m, Vs[p] = v;
                Ps[p] = w;
                Gs[p] = g;
                if (kl_on) a.G[p] = g;      // a later minibatch may trip the stop: keep the last applied one
            }
        }
        // ---- GS_HP_ACT_STATS: backbone.0's {mean, unbiased std, dead_pct, dead_max}
        double st[3] = {sz, sz2, 0.0};
        if (a.act_stats) {
            unsigned mx = 0u;
            for (int j = tid; j < H; j += 256) {
                const unsigned c = dead[j];
                st[2] += (double)c;
                mx = c > mx ? c : mx;
            }
            atomicMax(&s_dead_max, mx);
            block_reduce<3>(st, dred);
        }
        if (tid == 0) {
            write_metrics(tot, rows, la, rec, true);
            write_step_tail(rec, total, gn_back, gn_pol, gn_val);
            if (a.act_stats)
                act_quad(st[0], st[1], st[2], (double)s_dead_max, (double)B * (double)H, (double)B, rec + GS_M_ACT);
            if (tripped) s_stop = 1;
        }
    }
    __syncthreads();
    // ---- epilogue: the optimizer state back to HBM, once
    if (train) {
        for (int p = tid; p < NP; p += 256) {
            a.P[p] = Ps[p];
            if constexpr (kMoments) {
                a.M[p] = Ms[p];
                a.V[p] = Vs[p];
            }
            if (!kl_on) a.G[p] = Gs[p];     // the last minibatch's clipped gradient
        }
        if (kl_on && tid == 0 && s_stop) *a.stop = 1;
    }
}

// ------------------------------------------------------------------------------------
// k_act_stats1: gs_mlp_activation_stats for one hidden layer — per 16 rows a part of
// 2 * (2 + H) doubles: backbone.0's {sum z, sum z^2, per neuron the count of |z| < 1e-6}, then
// the (absent) second layer's part, zero.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_act_stats1(const float *__restrict__ P, Layout1 L,
                                                    const float *__restrict__ obs, const int32_t *__restrict__ idx,
                                                    int T, int N, int R, double *__restrict__ part)
{
    extern __shared__ float lds_x[];
    __shared__ double sred[2 * 272];
    const int tid = threadIdx.x, D = L.D, H = L.H;
    const int r0 = blockIdx.x * 16, nr = min(16, R - r0);
    for (int u = tid; u < 16 * D; u += 256) {
        const int r = u / D, d = u - r * D;
        const int src = r < nr ? (idx ? sample_row_checked(idx[r0 + r], T, N) : r0 + r) : -1;
        lds_x[u] = src >= 0 ? obs[(int64_t)src * D + d] : 0.0f;
    }
    __syncthreads();
    double *out = part + (int64_t)blockIdx.x * 2 * (2 + H);
    double st[2] = {0.0, 0.0};
    for (int j = tid; j < H; j += 256) {
        int cnt = 0;
        for (int r = 0; r < nr; ++r) {
            float z = P[L.ob1 + j];
            for (int d = 0; d < D; ++d) z = fmaf(P[L.oW1 + j * D + d], lds_x[r * D + d], z);
            st[0] += (double)z;
            st[1] += (double)z * (double)z;
            cnt += act_dead(z) ? 1 : 0;
        }
        out[2 + j] = (double)cnt;
    }
    block_reduce<2>(st, sred);
    if (tid == 0) out[0] = st[0], out[1] = st[1];
    for (int j = tid; j < 2 + H; j += 256) out[2 + H + j] = 0.0;
}

}  // namespace

size_t mlp1_update_lds_bytes(const gs_mlp_dims &d)
{
    return Lds1::make((size_t)d.obs_dim, (size_t)d.hidden1, (size_t)d.n_actions).bytes;
}

int mlp1_check_dims(const gs_mlp_dims &d)
{
    GS_REQUIRE(d.hidden2 == 0, "one hidden layer is hidden2 == 0, got %d", d.hidden2);
    GS_REQUIRE(d.obs_dim > 0 && d.obs_dim <= kMaxObsDim, "obs_dim %d outside [1, %d]", d.obs_dim, kMaxObsDim);
    GS_REQUIRE(d.hidden1 > 0 && d.hidden1 % kTile == 0 && d.hidden1 <= (1 << 20),
               "hidden1 %d must be a positive multiple of 16", d.hidden1);
    GS_REQUIRE(d.n_actions > 0 && d.n_actions <= kMaxActions, "n_actions %d outside [1, %d]", d.n_actions,
               kMaxActions);
    const Lds1 l = Lds1::make((size_t)d.obs_dim, (size_t)d.hidden1, (size_t)d.n_actions);
    GS_REQUIRE(l.bytes <= kLdsBudget1,
               "one hidden layer %d-%d-%d: the update keeps the parameters, both Adam moments and the gradient in LDS "
               "(4 x %zu bytes) beside %zu bytes of row-tile staging = %zu bytes, more than a workgroup's %zu",
               d.obs_dim, d.hidden1, d.n_actions, l.param_bytes, l.tile_bytes, l.bytes, kLdsBudget1);
    return GS_OK;
}

int mlp1_policy_act(const float *params, const gs_mlp_dims &d, const float *obs, int64_t N, int mode, uint64_t rng_seed,
                    uint64_t rng_counter, int64_t *actions, float *logp, float *value, float *obs_store,
                    const uint64_t *clock, hipStream_t s, uint32_t valid_mask)
{
    int rc = mlp1_check_dims(d);
    if (rc) return rc;
    GS_REQUIRE(N > 0 && (N + 255) / 256 < (int64_t)1 << 31, "one-hidden-layer act: N out of range");
    GS_REQUIRE(mode >= 0 && mode <= 2, "one-hidden-layer act: mode %d not in {0,1,2}", mode);
    GS_REQUIRE(params && obs && value && (actions != nullptr) == (logp != nullptr), "one-hidden-layer act: null buffer");
    const Layout1 L = Layout1::make(d.obs_dim, d.hidden1, d.n_actions);
    const size_t lds = sizeof(float) * ((size_t)round4i(L.P) + 256 * (size_t)(L.D | 1));
    const unsigned nb = (unsigned)((N + 255) / 256);
    return with_amax(L.A, [&](auto amax) {
        constexpr int AMAX = decltype(amax)::value;
        auto launch = [&](auto masked) {
            constexpr bool MASKED = decltype(masked)::value;
            const int rl = set_lds_limit((const void *)k_act1<AMAX, MASKED>, lds);
            if (rl) return rl;
            hipLaunchKernelGGL((k_act1<AMAX, MASKED>), dim3(nb), dim3(256), lds, s, params, L, obs, N, mode, rng_seed,
                               rng_counter, actions, logp, value, obs_store, clock, valid_mask);
            GS_LAUNCH_CHECK("k_act1");
            return (int)GS_OK;
        };
        return valid_mask != 0u ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

size_t mlp1_rollout_lds_bytes(const gs_mlp_dims &d)
{
    const Layout1 L = Layout1::make(d.obs_dim, d.hidden1, d.n_actions);
    return sizeof(float) * ((size_t)round4i(L.P) + (size_t)kRollout1Envs * (size_t)(L.D | 1));
}

bool mlp1_rollout_fits(const gs_mlp_dims &d) { return mlp1_rollout_lds_bytes(d) <= kLdsBudget1; }

int mlp1_check_rollout_entry(const char *who, const gs_mlp_dims &dims, int64_t N, int64_t T, int mode,
                             const float *params, const EnvArgs &ev, const RolloutRows &rw)
{
    GS_REQUIRE(dims.hidden2 == 0, "%s: serves a policy with one hidden layer (hidden2 == 0), got hidden2 = %d", who,
               dims.hidden2);
    int rc = mlp1_check_dims(dims);
    if (rc) return rc;
    GS_REQUIRE(N > 0 && (N + kRollout1Envs - 1) / kRollout1Envs < (int64_t)1 << 31 && T >= 0 && T < (int64_t)1 << 31,
               "%s: bad N / T", who);
    GS_REQUIRE(mode >= 0 && mode <= 2, "%s: mode %d not in {0,1,2}", who, mode);
    GS_REQUIRE(ev.max_steps > 0, "%s: max_steps must be > 0", who);
    GS_REQUIRE(params && ev.meta && ev.ep_ret && ev.obs && rw.obs && rw.actions && rw.logp && rw.value &&
                   rw.reward && rw.done && rw.timeout,
               "%s: null buffer", who);
    return GS_OK;
}

template <class E>
int mlp1_launch_rollout(const float *P, const gs_mlp_dims &d, int64_t N, int T, int mode, uint64_t rng_seed,
                        uint64_t counter0, const typename E::Args &ev, const RolloutRows &rw, hipStream_t s)
{
    const Layout1 L = Layout1::make(d.obs_dim, d.hidden1, d.n_actions);
    const size_t lds = mlp1_rollout_lds_bytes(d);
    GS_REQUIRE(lds <= kLdsBudget1, "one-hidden-layer rollout: %zu bytes of LDS do not fit", lds);
    const unsigned nb = (unsigned)((N + kRollout1Envs - 1) / kRollout1Envs);
    return with_amax(L.A, [&](auto amax) {
        constexpr int AMAX = decltype(amax)::value;
        const int rl = set_lds_limit((const void *)k_rollout1<AMAX, E>, lds);
        if (rl) return rl;
        hipLaunchKernelGGL((k_rollout1<AMAX, E>), dim3(nb), dim3(kRollout1Envs), lds, s, P, L, N, T, mode, rng_seed,
                           counter0, ev, rw);
        GS_LAUNCH_CHECK("k_rollout1");
        return (int)GS_OK;
    });
}
#define GS_ROLLOUT1_INSTANCE(E)                                                                                 \
    template int mlp1_launch_rollout<E>(const float *, const gs_mlp_dims &, int64_t, int, int, uint64_t, uint64_t, \
                                        const E::Args &, const RolloutRows &, hipStream_t)
GS_ROLLOUT1_INSTANCE(TabularEnv);
GS_ROLLOUT1_INSTANCE(CartPoleEnv);
GS_ROLLOUT1_INSTANCE(CartPoleShapedEnv);
GS_ROLLOUT1_INSTANCE(AcrobotEnv);
GS_ROLLOUT1_INSTANCE(MountainCarEnv);
GS_ROLLOUT1_INSTANCE(BanditEnv);
#undef GS_ROLLOUT1_INSTANCE

int mlp1_update(float *params, float *grads, float *adam_m, float *adam_v, const gs_mlp_dims &d,
                const gs_ppo_hparams &hp, const gs_rollout_view &ro, const int32_t *idx, int64_t batch, int64_t n,
                int64_t adam_step0, float *metrics, int32_t *stop_flag, bool loss_only, hipStream_t s)
{
    if (!loss_only) GS_REQUIRE_OPT_FLAGS(hp.flags, "one-hidden-layer update");
    int rc = mlp1_check_dims(d);
    if (rc) return rc;
    GS_REQUIRE(!(hp.flags & GS_HP_BF16), "precision bf16 is a mode of the two-hidden-layer fused chain; a policy with "
                                         "one hidden layer updates in fp32 only");
    GS_REQUIRE(batch >= 2 && batch <= 1024, "batch %lld outside [2, 1024]", (long long)batch);
    GS_REQUIRE(ro.T > 0 && ro.N > 0, "empty rollout");
    GS_REQUIRE(ro.obs && ro.actions && ro.logprobs && ro.values && ro.advantages && ro.returns,
               "rollout view has a null buffer");
    GS_REQUIRE(ro.T * ro.N < (int64_t)1 << 31, "rollout larger than 2^31 samples");
    GS_REQUIRE(n >= 0 && n < (int64_t)1 << 31 && adam_step0 >= 0, "bad n_minibatches/adam_step0");
    GS_REQUIRE(params && idx && metrics && (loss_only || (grads && adam_m && adam_v)), "one-hidden-layer update: null buffer");
    GS_REQUIRE(loss_only || !(hp.target_kl > 0.0f) || stop_flag, "target_kl needs the stop flag");
    if (n == 0) return GS_OK;
    const Layout1 L = Layout1::make(d.obs_dim, d.hidden1, d.n_actions);
    Upd1Args a{};
    a.P = params, a.G = grads, a.M = adam_m, a.V = adam_v;
    a.obs = ro.obs, a.actions = ro.actions, a.logprobs = ro.logprobs, a.values = ro.values;
    a.advantages = ro.advantages, a.returns = ro.returns;
    a.T = (int)ro.T, a.N = (int)ro.N;
    a.idx = idx, a.B = (int)batch, a.n = (int)n, a.step0 = adam_step0;
    a.metrics = metrics;
    a.stop = hp.target_kl > 0.0f && !loss_only ? stop_flag : nullptr;   // target_kl unset: neither read nor written
    a.la = loss_args(hp);
    a.la.batch_rows = (int)batch;
    a.la.inv_batch = 1.0f / (float)batch;
    const double b1 = hp.adam_beta1, b2 = hp.adam_beta2;
    GS_REQUIRE(loss_only || (b1 > 0.0 && b1 < 1.0 && b2 > 0.0 && b2 < 1.0), "Adam betas must lie in (0, 1)");
    a.aa = adam_args(hp, adam_step0 + 1);   // the kernel forms each step's schedule itself, from lr and the logs below
    a.lr = (double)hp.lr;
    a.ln_b1 = loss_only ? 0.0 : log(b1);
    a.ln_b2 = loss_only ? 0.0 : log(b2);
    a.act_stats = (hp.flags & GS_HP_ACT_STATS) && !loss_only ? 1 : 0;
    a.loss_only = loss_only ? 1 : 0;
    const size_t lds = mlp1_update_lds_bytes(d);
    return with_amax(L.A, [&](auto amax) {
        constexpr int AMAX = decltype(amax)::value;
        return with_opt(loss_only ? kOptAdam : a.aa.opt, [&](auto opt) {
            constexpr int OPT = decltype(opt)::value;
            const int rl = set_lds_limit((const void *)k_update1<AMAX, OPT>, lds);
            if (rl) return rl;
            hipLaunchKernelGGL((k_update1<AMAX, OPT>), dim3(1), dim3(256), lds, s, L, a);
            GS_LAUNCH_CHECK("k_update1");
            return (int)GS_OK;
        });
    });
}

int mlp1_activation_stats(const float *params, const gs_mlp_dims &d, const gs_rollout_view &ro, const int32_t *idx,
                          int64_t rows, double *part, hipStream_t s)
{
    int rc = mlp1_check_dims(d);
    if (rc) return rc;
    GS_REQUIRE(params && ro.obs && part && rows >= 1 && rows < (int64_t)1 << 31,
               "gs_mlp_activation_stats: null buffer or no rows");
    GS_REQUIRE(ro.T > 0 && ro.N > 0 && ro.T * ro.N < (int64_t)1 << 31, "gs_mlp_activation_stats: bad rollout shape");
    GS_REQUIRE(idx || rows <= ro.T * ro.N, "gs_mlp_activation_stats: more rows than the rollout holds");
    const Layout1 L = Layout1::make(d.obs_dim, d.hidden1, d.n_actions);
    hipLaunchKernelGGL(k_act_stats1, dim3((unsigned)((rows + 15) / 16)), dim3(256), sizeof(float) * 16 * L.D, s, params,
                       L, ro.obs, idx, (int)ro.T, (int)ro.N, (int)rows, part);
    GS_LAUNCH_CHECK("k_act_stats1");
    return GS_OK;
}

}  // namespace gs

using namespace gs;

// ---- the gs_rollout1_* entries (include/gsamd.h) of the envs with their own tensors in the
// argument list; gs_rollout1_tabular is in gs_tabular.hip beside the spec check it shares
extern "C" int gs_rollout1_supported(gs_mlp_dims dims, int *supported)
{
    GS_REQUIRE(supported, "gs_rollout1_supported: null output");
    *supported = 0;
    GS_REQUIRE(dims.hidden2 == 0, "gs_rollout1_supported: serves a policy with one hidden layer (hidden2 == 0), got "
                                  "hidden2 = %d", dims.hidden2);
    int rc = mlp1_check_dims(dims);
    if (rc) return rc;
    *supported = mlp1_rollout_fits(dims) ? 1 : 0;
    return GS_OK;
}

extern "C" int gs_rollout1_env(const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                               uint64_t rng_seed, uint64_t rng_counter0, int kind, double *env_state,
                               int32_t *env_meta, float *env_ep_ret, float *env_obs, int32_t max_steps,
                               uint64_t env_seed, int64_t env_offset, int32_t *ep_done_count, float *ep_ret_sum,
                               float *ep_len_sum, float *obs_rows, int64_t *action_rows, float *logp_rows,
                               float *value_rows, float *reward_rows, uint8_t *done_rows, uint8_t *timeout_rows,
                               void *stream)
{
    GS_REQUIRE(kind != GS_ENV_MOUNTAINCAR,
               "gs_rollout1_env: MountainCar takes its count tables and wrappers through gs_rollout1_mountaincar");
    GS_REQUIRE(kind != GS_ENV_BANDIT, "gs_rollout1_env: the bandit takes its spec through gs_rollout1_bandit");
    GS_REQUIRE(kind == GS_ENV_CARTPOLE || kind == GS_ENV_ACROBOT, "gs_rollout1_env: env kind %d has no dynamics here",
               kind);
    const DynEnvArgs ev{{env_meta, env_ep_ret, env_obs, ep_done_count, ep_ret_sum, ep_len_sum, max_steps, env_seed,
                         env_offset},
                        env_state};
    const RolloutRows rw{obs_rows, action_rows, logp_rows, value_rows, reward_rows, done_rows, timeout_rows};
    const char *bad = env_state ? nullptr : "null buffer";
    if (kind == GS_ENV_CARTPOLE)
        return rollout1_entry<CartPoleEnv>("gs_rollout1_env", params, dims, N, T, mode, rng_seed, rng_counter0, ev, rw,
                                           CartPoleEnv::kObsDim, CartPoleEnv::kActions, bad, stream);
    return rollout1_entry<AcrobotEnv>("gs_rollout1_env", params, dims, N, T, mode, rng_seed, rng_counter0, ev, rw,
                                      AcrobotEnv::kObsDim, AcrobotEnv::kActions, bad, stream);
}

extern "C" int gs_rollout1_mountaincar(const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                                       uint64_t rng_seed, uint64_t rng_counter0, double *env_state,
                                       int32_t *env_meta, float *env_ep_ret, float *env_obs, int32_t *env_counts,
                                       gs_mountaincar_wrappers wrappers, int32_t max_steps, uint64_t env_seed,
                                       int64_t env_offset, int32_t *ep_done_count, float *ep_ret_sum,
                                       float *ep_len_sum, float *obs_rows, int64_t *action_rows, float *logp_rows,
                                       float *value_rows, float *reward_rows, uint8_t *done_rows,
                                       uint8_t *timeout_rows, void *stream)
{
    const MountainCarEnv::Args ev{{{env_meta, env_ep_ret, env_obs, ep_done_count, ep_ret_sum, ep_len_sum, max_steps,
                                    env_seed, env_offset},
                                   env_state},
                                  env_counts,
                                  wrappers};
    const RolloutRows rw{obs_rows, action_rows, logp_rows, value_rows, reward_rows, done_rows, timeout_rows};
    const char *bad = env_state ? mountaincar_wrappers_error(wrappers, env_counts) : "null buffer";
    return rollout1_entry<MountainCarEnv>("gs_rollout1_mountaincar", params, dims, N, T, mode, rng_seed, rng_counter0,
                                          ev, rw, MountainCarEnv::kObsDim, MountainCarEnv::kActions, bad, stream);
}

extern "C" int gs_rollout1_cartpole_shaped(const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                                           uint64_t rng_seed, uint64_t rng_counter0, double *env_state,
                                           double *env_prev_phi, int32_t *env_meta, float *env_ep_ret,
                                           float *env_obs, gs_cartpole_wrappers wrappers, int32_t max_steps,
                                           uint64_t env_seed, int64_t env_offset, int32_t *ep_done_count,
                                           float *ep_ret_sum, float *ep_len_sum, float *obs_rows,
                                           int64_t *action_rows, float *logp_rows, float *value_rows,
                                           float *reward_rows, uint8_t *done_rows, uint8_t *timeout_rows,
                                           void *stream)
{
    const CartPoleShapedEnv::Args ev{{{env_meta, env_ep_ret, env_obs, ep_done_count, ep_ret_sum, ep_len_sum,
                                       max_steps, env_seed, env_offset},
                                      env_state},
                                     env_prev_phi,
                                     wrappers};
    const RolloutRows rw{obs_rows, action_rows, logp_rows, value_rows, reward_rows, done_rows, timeout_rows};
    return rollout1_entry<CartPoleShapedEnv>("gs_rollout1_cartpole_shaped", params, dims, N, T, mode, rng_seed,
                                             rng_counter0, ev, rw, CartPoleShapedEnv::kObsDim,
                                             CartPoleShapedEnv::kActions,
                                             env_state && env_prev_phi ? nullptr : "null buffer", stream);
}

extern "C" int gs_rollout1_bandit(const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                                  uint64_t rng_seed, uint64_t rng_counter0, int32_t *env_meta, float *env_ep_ret,
                                  float *env_obs, gs_bandit_spec spec, int32_t max_steps, uint64_t env_seed,
                                  int64_t env_offset, int32_t *ep_done_count, float *ep_ret_sum, float *ep_len_sum,
                                  float *obs_rows, int64_t *action_rows, float *logp_rows, float *value_rows,
                                  float *reward_rows, uint8_t *done_rows, uint8_t *timeout_rows, void *stream)
{
    const BanditEnv::Args ev{{env_meta, env_ep_ret, env_obs, ep_done_count, ep_ret_sum, ep_len_sum, max_steps,
                              env_seed, env_offset},
                             spec};
    const RolloutRows rw{obs_rows, action_rows, logp_rows, value_rows, reward_rows, done_rows, timeout_rows};
    return rollout1_entry<BanditEnv>("gs_rollout1_bandit", params, dims, N, T, mode, rng_seed, rng_counter0, ev, rw,
                                     spec.n_arms, spec.n_arms, bandit_spec_error(spec), stream);
}
