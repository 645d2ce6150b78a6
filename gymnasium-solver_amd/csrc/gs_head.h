// gs_head.h — the per-row arithmetic every policy's kernels share: the categorical head
// (log-softmax statistics, action select, log-prob), one row of the PPO loss in pieces (the
// categorical row, the PPO terms, their metric sums and analytic gradients), the metric record and
// its tail, the fixed-order block sum, the clip coefficient and one parameter's Adam step.
// Included by gs_mlp.hip (two hidden layers), gs_mlp1.hip (one hidden layer), gs_mc.hip, gs_cnn.hip
// (NatureCNN: the PPO terms, the record and mix64 under its own masked head), gs_ppo_rows.hip (the
// row-parallel PPO update: loss_row, write_metrics, block_reduce, clip_coef, adam_param) and, through
// gs_pg_head.h, gs_pg.hip (REINFORCE: the categorical row and the Adam step).
// "Round identically" holds between gs_mlp.hip and gs_mlp1.hip, which compile with
// -ffp-contract=off; gs_cnn.hip, gs_pg.hip and gs_ppo_rows.hip compile with the default contraction
// (FMA), so the same source there may round a mul + add once where the MLP files round twice.
#pragma once

#include <float.h>
#include <math.h>

#include "gs_common.h"

namespace gs {

// env-major sample index (utils/rollout_buffer.py:11-13) -> time-major buffer row
__device__ __forceinline__ int sample_row(int s, int T, int N)
{
    const unsigned e = (unsigned)s / (unsigned)T;
    const unsigned t = (unsigned)s - e * (unsigned)T;
    return (int)(t * (unsigned)N + e);
}

constexpr int kNumSums = 14;   // metric sums of one minibatch (loss_row)

// Sum NV per-thread values over the 256-thread block in a fixed order (deterministic),
// through LDS (two levels of 16) — __shfl would lower to ds_bpermute chains (~100+ cycles
// per step).  Every thread returns the totals.  scratch: NV*(256+16) elements of T.
// In a block wider than 256 threads only threads 0..255 contribute (the others only meet the
// barriers and read the totals), so the sum order is the 256-thread one.
template <int NV, typename T>
__device__ __forceinline__ void block_reduce(T (&v)[NV], T *scratch)
{
    const int tid = threadIdx.x;
    if (tid < 256)
#pragma unroll
        for (int k = 0; k < NV; ++k) scratch[k * 256 + tid] = v[k];
    __syncthreads();
    T *part = scratch + NV * 256;
    if (tid < NV * 16) {
        const int k = tid >> 4, j = tid & 15;
        T acc = 0;
#pragma unroll
        for (int m = 0; m < 16; ++m) acc += scratch[k * 256 + j * 16 + m];
        part[tid] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        T acc = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc += part[k * 16 + j];
        v[k] = acc;
    }
    __syncthreads();
}

// clip_grad_norm_'s coefficient (max_norm <= 0: no clip; agents/base_agent.py:591-621)
__device__ __forceinline__ float clip_coef(float total, const AdamArgs &aa)
{
    float coef = 1.0f;
    if (aa.max_norm > 0.0f) {
        coef = aa.max_norm / (total + 1e-6f);
        coef = fminf(coef, 1.0f);
    }
    return coef;
}

// One parameter of torch.optim.Adam (single-tensor path, amsgrad off) on the clipped gradient;
// shared by k_clip_adam, the lagged step in k_fwd_hidden and the one-hidden-layer update so all
// round identically.
// inv_bc2s = f32(1 / sqrt(1 - beta2^t)) (host, double), so the bias correction is a multiply.
__device__ __forceinline__ float adam_param(float graw, float coef, float &m, float &v, float &p,
                                            const AdamArgs &aa, float neg_step, float inv_bc2s)
{
    const float g = graw * coef;
    m = m + aa.one_minus_b1 * (g - m);            // exp_avg.lerp_(grad, 1 - beta1)
    v = v * aa.b2;                                // exp_avg_sq.mul_(beta2)
    v = v + (aa.one_minus_b2 * g) * g;            //   .addcmul_(grad, grad, 1 - beta2)
    // hardware sqrt and reciprocal (v_sqrt_f32, v_rcp_f32: ~1 ulp each) instead of torch's
    // correctly rounded divisions: IEEE division lowers to a v_div_scale / v_div_fmas /
    // v_div_fixup sequence serialised through VCC, ~10x the latency, and this runs 4-21 times
    // per thread on the minibatch chain's critical path
    const float denom = __builtin_amdgcn_sqrtf(v) * inv_bc2s + aa.eps;
    p = p + neg_step * (m * __builtin_amdgcn_rcpf(denom));
    return g;
}

// torch.optim.AdamW's decoupled decay of one parameter, ahead of Adam's step: p.mul_(1 - lr * weight_decay)
// with the factor formed on the host (AdamArgs::decay).  __fmul_rn: one rounding of its own in the
// files that contract a mul + add too, so a parameter with a zero gradient is p * d bit for bit everywhere.
__device__ __forceinline__ float adamw_decay(float p, const AdamArgs &aa) { return __fmul_rn(p, aa.decay); }

// One parameter of torch.optim.AdamW (single-tensor path): the decay, then exactly adam_param.
__device__ __forceinline__ float adamw_param(float graw, float coef, float &m, float &v, float &p,
                                             const AdamArgs &aa, float neg_step, float inv_bc2s)
{
    p = adamw_decay(p, aa);
    return adam_param(graw, coef, m, v, p, aa, neg_step, inv_bc2s);
}

// One parameter of torch.optim.SGD (no momentum, no decay) on the clipped gradient:
// p.add_(grad, alpha=-lr); aa.neg_step_size is f32(-lr), no moment and no schedule entry is read.
__device__ __forceinline__ float sgd_param(float graw, float coef, float &p, const AdamArgs &aa)
{
    const float g = graw * coef;
    p = p + aa.neg_step_size * g;
    return g;
}

// The step of optimizer OPT (kOptAdam / kOptAdamW / kOptSGD) on one parameter; SGD leaves m and v alone.
template <int OPT>
__device__ __forceinline__ float opt_param(float graw, float coef, float &m, float &v, float &p, const AdamArgs &aa,
                                           float neg_step, float inv_bc2s)
{
    if constexpr (OPT == kOptSGD) return sgd_param(graw, coef, p, aa);
    else if constexpr (OPT == kOptAdamW) return adamw_param(graw, coef, m, v, p, aa, neg_step, inv_bc2s);
    else return adam_param(graw, coef, m, v, p, aa, neg_step, inv_bc2s);
}

// host: call f with the optimizer of a step as a compile-time constant
template <class F>
inline int with_opt(int opt, F &&f)
{
    if (opt == kOptSGD) return f(std::integral_constant<int, kOptSGD>{});
    if (opt == kOptAdamW) return f(std::integral_constant<int, kOptAdamW>{});
    return f(std::integral_constant<int, kOptAdam>{});
}

// ------------------------------------------------------------------------------------
// per-row categorical head math shared by rollout and loss kernels
// ------------------------------------------------------------------------------------
struct HeadRow {
    float lse;    // logsumexp of raw logits
    float m2;     // max of normalised logits
    float S;      // sum exp(ln - m2)
};

// z: raw logits of one row held in registers (AMAX = compile-time bound on A).
template <int AMAX>
__device__ __forceinline__ HeadRow head_stats(const float (&z)[AMAX + 1], int A)
{
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a < A) m = fmaxf(m, z[a]);
    float se = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a < A) se += expf(z[a] - m);
    HeadRow h;
    h.lse = m + logf(se);
    float m2 = -INFINITY;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a < A) m2 = fmaxf(m2, z[a] - h.lse);
    h.m2 = m2;
    float S = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a < A) S += expf((z[a] - h.lse) - m2);
    h.S = S;
    return h;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// value, action (sampled / argmax / replayed) and its log-prob of one env row from its raw
// logits | value z; ctr = the rollout step's counter of the counter-based uniform
template <int AMAX>
__device__ __forceinline__ void head_act_row(const float (&z)[AMAX + 1], int A, int mode, uint64_t seed, uint64_t ctr,
                                             int64_t r, int64_t *__restrict__ action, float *__restrict__ logp,
                                             float *__restrict__ value)
{
    float v = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX + 1; ++a)
        if (a == A) v = z[a];
    if (value) *value = v;
    if (!action) return;
    const HeadRow h = head_stats<AMAX>(z, A);
    int act = 0;
    if (mode == 2) {            // replay recorded actions
        act = (int)*action;
    } else if (mode == 1) {     // Categorical.mode = probs.argmax(-1), first max wins
        float best = -INFINITY;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
            if (a < A) {
                const float p = expf((z[a] - h.lse) - h.m2) / h.S;
                if (p > best) { best = p; act = a; }
            }
        }
        *action = act;
    } else {                    // inverse-CDF sample with a counter-based uniform
        const uint64_t hh = mix64(mix64(mix64(seed) ^ ctr) ^ (uint64_t)r);
        const float u = (float)(hh >> 40) * (1.0f / 16777216.0f);
        float c = 0.0f;
        act = -1;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
            if (a < A) {
                c += expf((z[a] - h.lse) - h.m2) / h.S;
                if (act < 0 && u < c) act = a;
            }
        }
        if (act < 0) act = A - 1;
        *action = act;
    }
    float za = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a == act) za = z[a];
    *logp = za - h.lse;
}

// ------------------------------------------------------------------------------------
// The categorical row of a loss (Categorical: utils/distributions.py): from the raw logits z and
// the taken action, ln = normalised logits, p = softmax(ln) (Categorical.probs), the entropy H and
// the taken log-prob lp.  Shared by loss_row and pg_loss_row (gs_pg_head.h).
// ------------------------------------------------------------------------------------
template <int AMAX>
struct CatRow {
    float ln[AMAX], p[AMAX];   // normalised logits, softmax(ln) (Categorical.probs)
    float H, lp;               // entropy, the taken action's log-prob
};

template <int AMAX>
__device__ __forceinline__ CatRow<AMAX> cat_row(const float (&z)[AMAX + 1], int A, int act)
{
    const HeadRow h = head_stats<AMAX>(z, A);
    const float invS = 1.0f / h.S;
    // local arrays, copied out below: filled through the result (or through reference parameters)
    // the compiler no longer merges p's expf with head_stats' for every action (one more per row)
    float ln[AMAX], p[AMAX];
    float H = 0.0f, lp = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
        ln[a] = z[a] - h.lse;
        p[a] = a < A ? expf(ln[a] - h.m2) * invS : 0.0f;
        if (a < A) {
            H += fmaxf(ln[a], -FLT_MAX) * p[a];   // entropy: -sum clamp(ln, f32min) * p
            if (a == act) lp = ln[a];
        }
    }
    CatRow<AMAX> c;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) c.ln[a] = ln[a], c.p[a] = p[a];
    c.H = -H;
    c.lp = lp;
    return c;
}

// one row of the approx_kl estimate (r - 1) - log r, the log-ratio clamped to +-20
__device__ __forceinline__ float approx_kl_row(float lp, float olp)
{
    const float ldiff = fminf(fmaxf(lp - olp, -20.0f), 20.0f);
    const float r2 = expf(ldiff);
    return (r2 - 1.0f) - logf(r2);
}

// dLoss/dlogits of a row from dlp = dLoss/d(taken log-prob) and dH = dLoss/d(entropy)
template <int AMAX>
__device__ __forceinline__ void cat_row_grad(const CatRow<AMAX> &c, int A, int act, float dlp, float dH,
                                             float *__restrict__ dzr)
{
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
        if (a < A) {
            const float pe = expf(c.ln[a]);   // softmax(z) as seen by logsumexp backward
            float g = dlp * ((a == act ? 1.0f : 0.0f) - pe);
            g += dH * (-c.p[a] * (c.ln[a] + c.H));
            dzr[a] = g;
        }
    }
}

// ------------------------------------------------------------------------------------
// The PPO terms of one minibatch row (PPOAgent.losses_for_batch, agents/ppo/ppo_agent.py:21-152)
// from its taken log-prob lp, value v and (normalised) advantage: the clipped surrogate, the
// clipped value loss, the row's 13 metric sums and the gradients with respect to lp and v.  The
// distribution (how lp and the entropy H come from the logits) is the caller's: loss_row below,
// the (Masked)Categorical rows of gs_cnn.hip.
// ------------------------------------------------------------------------------------
struct PpoRowTerms {
    float ratio, s1, s2, mn;   // exp(lp - olp), adv ratio, adv clamp(ratio), min(s1, s2)
    float vdelta;              // v - ov
    float du, vu, dc, vc;      // v - ret and its square; the same of the clipped value
};

__device__ __forceinline__ PpoRowTerms ppo_row_terms(float lp, float olp, float v, float ov, float adv, float ret,
                                                     const LossArgs &la)
{
    PpoRowTerms t;
    t.ratio = expf(lp - olp);
    const float rc = fminf(fmaxf(t.ratio, la.clip_lo), la.clip_hi);
    t.s1 = adv * t.ratio, t.s2 = adv * rc;
    t.mn = fminf(t.s1, t.s2);
    t.vdelta = v - ov;
    t.du = v - ret;
    t.vu = t.du * t.du;
    const float vcl = ov + fminf(fmaxf(t.vdelta, -la.clip_vf), la.clip_vf);
    t.dc = vcl - ret;
    t.vc = t.dc * t.dc;
    return t;
}

// adds the row's terms to the metric sums 0..12 (write_metrics reads them)
template <int NS>
__device__ __forceinline__ void ppo_row_sums(const PpoRowTerms &t, float H, float lp, float olp, float v, float adv,
                                             float ret, const LossArgs &la, double (&acc)[NS])
{
    static_assert(NS >= 13, "the PPO row has 13 metric sums");
    const float vmax = fmaxf(t.vu, t.vc);
    const float akl = approx_kl_row(lp, olp);
    const float rv = ret - v;
    acc[0] += (double)t.mn;
    acc[1] += (double)vmax;
    acc[2] += (double)H;
    acc[3] += (t.ratio < la.clip_lo || t.ratio > la.clip_hi) ? 1.0 : 0.0;
    acc[4] += (t.vdelta < -la.clip_vf || t.vdelta > la.clip_vf) ? 1.0 : 0.0;
    acc[5] += (double)(olp - lp);
    acc[6] += (double)akl;
    acc[7] += (double)rv;
    acc[8] += (double)rv * (double)rv;
    acc[9] += (double)ret;
    acc[10] += (double)ret * (double)ret;
    acc[11] += (double)adv;
    acc[12] += (double)adv * (double)adv;
}

// dLoss/dlp of the clipped surrogate (torch autograd tie rules: min/max ties split halves)
__device__ __forceinline__ float ppo_row_dlp(const PpoRowTerms &t, float adv, const LossArgs &la, float invB)
{
    const float ga = t.s1 < t.s2 ? 1.0f : (t.s1 == t.s2 ? 0.5f : 0.0f);
    const float gb = t.s2 < t.s1 ? 1.0f : (t.s1 == t.s2 ? 0.5f : 0.0f);
    const float inclip = (t.ratio >= la.clip_lo && t.ratio <= la.clip_hi) ? 1.0f : 0.0f;
    const float g_mn = -invB;
    const float dratio = adv * (g_mn * ga) + adv * (g_mn * gb) * inclip;
    return dratio * t.ratio;
}

// dLoss/dvalue of the clipped value loss (the same tie rule)
__device__ __forceinline__ float ppo_row_dvalue(const PpoRowTerms &t, const LossArgs &la, float invB)
{
    const float hu = t.vu > t.vc ? 1.0f : (t.vu == t.vc ? 0.5f : 0.0f);
    const float hc = t.vc > t.vu ? 1.0f : (t.vu == t.vc ? 0.5f : 0.0f);
    const float invc = (t.vdelta >= -la.clip_vf && t.vdelta <= la.clip_vf) ? 1.0f : 0.0f;
    const float gv = la.vf_coef * invB;
    return (gv * hu) * (2.0f * t.du) + (gv * hc) * (2.0f * t.dc) * invc;
}

// ------------------------------------------------------------------------------------
// One minibatch row of the MLP policies' PPO loss with its analytic gradients: z = raw logits |
// value, adv already batch-normalised.  Writes dLoss/dlogits | dLoss/dvalue to dzr and adds the
// row's terms to the 14 metric sums.
// ------------------------------------------------------------------------------------
template <int AMAX>
__device__ __forceinline__ void loss_row(const float (&z)[AMAX + 1], int A, int act, float olp, float ov, float adv,
                                         float ret, const LossArgs &la, float invB, float *__restrict__ dzr,
                                         double (&acc)[kNumSums])
{
    float v = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX + 1; ++a)
        if (a == A) v = z[a];
    const CatRow<AMAX> c = cat_row<AMAX>(z, A, act);
    const PpoRowTerms t = ppo_row_terms(c.lp, olp, v, ov, adv, ret, la);
    ppo_row_sums(t, c.H, c.lp, olp, v, adv, ret, la, acc);
    cat_row_grad<AMAX>(c, A, act, ppo_row_dlp(t, adv, la, invB), -la.ent_coef * invB, dzr);
    dzr[A] = ppo_row_dvalue(t, la, invB);
}

// ------------------------------------------------------------------------------------
// The masked head of the MLP policies (MaskedCategorical, utils/distributions.py:8-82; the policy is
// built with valid_actions = spec.action_space.valid, utils/models.py:285-346): the counterparts of
// head_stats / head_act_row / cat_row / cat_row_grad / loss_row over the valid actions only.
// valid: bit a set = action a valid, never 0 here (the entries send a zero mask to the functions
// above).  The mask is uniform over the grid, so an invalid action costs a scalar branch: its
// exponentials are never formed.  The act works on the row's logits in registers (head_stats_masked,
// head_act_row_masked), the loss row on the logits in memory (cat_row_masked and what follows it).
// The semantics are gs_cnn.hip's (mrow_stats, act_select, cnn_loss_row).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ bool head_valid(uint32_t valid, int a, int A) { return a < A && ((valid >> a) & 1u) != 0u; }

template <int AMAX>
__device__ __forceinline__ HeadRow head_stats_masked(const float (&z)[AMAX + 1], int A, uint32_t valid)
{
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (head_valid(valid, a, A)) m = fmaxf(m, z[a]);
    float se = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (head_valid(valid, a, A)) se += expf(z[a] - m);
    HeadRow h;
    h.lse = m + logf(se);
    float m2 = -INFINITY;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (head_valid(valid, a, A)) m2 = fmaxf(m2, z[a] - h.lse);
    h.m2 = m2;
    float S = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (head_valid(valid, a, A)) S += expf((z[a] - h.lse) - m2);
    h.S = S;
    return h;
}

// head_act_row over the valid actions: mode 1 takes the first maximum among them, mode 0 runs the
// inverse CDF over them in index order under the same counter-based uniform (the fallback is the last
// valid action), mode 2 replays the recorded action (one outside the valid set is the caller's error:
// its log-prob is unspecified, and nothing is read out of range)
template <int AMAX>
__device__ __forceinline__ void head_act_row_masked(const float (&z)[AMAX + 1], int A, uint32_t valid, int mode,
                                                    uint64_t seed, uint64_t ctr, int64_t r,
                                                    int64_t *__restrict__ action, float *__restrict__ logp,
                                                    float *__restrict__ value)
{
    float v = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX + 1; ++a)
        if (a == A) v = z[a];
    if (value) *value = v;
    if (!action) return;
    const HeadRow h = head_stats_masked<AMAX>(z, A, valid);
    int act = -1;
    if (mode == 2) {
        act = (int)*action;
    } else if (mode == 1) {
        float best = -INFINITY;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
            if (head_valid(valid, a, A)) {
                const float p = expf((z[a] - h.lse) - h.m2) / h.S;
                if (p > best) { best = p; act = a; }
            }
        }
        *action = act;
    } else {
        const uint64_t hh = mix64(mix64(mix64(seed) ^ ctr) ^ (uint64_t)r);
        const float u = (float)(hh >> 40) * (1.0f / 16777216.0f);
        float c = 0.0f;
        int last = 0;
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
            if (head_valid(valid, a, A)) {
                last = a;
                c += expf((z[a] - h.lse) - h.m2) / h.S;
                if (act < 0 && u < c) act = a;
            }
        }
        if (act < 0) act = last;
        *action = act;
    }
    float za = 0.0f;
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
        if (a == act) za = z[a];
    *logp = za - h.lse;
}

// The masked categorical row of a loss.  Unlike cat_row it reads the logits from memory (z: the row's
// logits | value, in LDS in k_ppo_rows) and walks the mask's set bits in index order, so it touches
// the valid actions only and holds no per-action array: with 3 of 18 actions valid the row forms 3
// exponentials per pass where an unrolled 32-action form held ~100 registers live across the row
// and measured 6 % slower per optimizer step than the unmasked kernel.
// p = softmax over the valid actions, lp = z[act] - lse_valid (0 for an action outside the set),
// H = -sum_valid p logf(p + 1e-8f) (MaskedCategorical.entropy, not Categorical's clamp form), and what
// its gradient needs: g_a = logf(p_a + 1e-8f) + p_a / (p_a + 1e-8f) (= -dH/dp_a), pg = sum_b p_b g_b.
struct MaskedCatRow {
    float lse, m2, invS;       // head_stats over the valid actions
    float H, lp, pg;
};

// one valid action's terms, formed alike by the row and by its gradient
struct MaskedTerm { float ln, p, g, plq; };
__device__ __forceinline__ MaskedTerm masked_term(float za, const MaskedCatRow &c)
{
    MaskedTerm t;
    t.ln = za - c.lse;
    t.p = expf(t.ln - c.m2) * c.invS;
    const float lq = logf(t.p + 1e-8f);
    t.g = lq + t.p / (t.p + 1e-8f);
    t.plq = t.p * lq;
    return t;
}

__device__ __forceinline__ MaskedCatRow cat_row_masked(const float *__restrict__ z, uint32_t valid, int act)
{
    float m = -INFINITY;
    for (uint32_t b = valid; b; b &= b - 1u) m = fmaxf(m, z[__builtin_ctz(b)]);
    float se = 0.0f;
    for (uint32_t b = valid; b; b &= b - 1u) se += expf(z[__builtin_ctz(b)] - m);
    MaskedCatRow c;
    c.lse = m + logf(se);
    float m2 = -INFINITY;
    for (uint32_t b = valid; b; b &= b - 1u) m2 = fmaxf(m2, z[__builtin_ctz(b)] - c.lse);
    c.m2 = m2;
    float S = 0.0f;
    for (uint32_t b = valid; b; b &= b - 1u) S += expf((z[__builtin_ctz(b)] - c.lse) - m2);
    c.invS = 1.0f / S;
    float H = 0.0f, lp = 0.0f, pg = 0.0f;
    for (uint32_t b = valid; b; b &= b - 1u) {
        const int a = __builtin_ctz(b);
        const MaskedTerm t = masked_term(z[a], c);
        H += t.plq;
        pg += t.p * t.g;
        if (a == act) lp = t.ln;
    }
    c.H = -H;
    c.lp = lp;
    c.pg = pg;
    return c;
}

// dLoss/dlogits of a masked row: dH/dz_a = -p_a (g_a - pg); exactly 0 for an invalid action
// (masked_fill blocks its gradient), so the invalid rows of the policy head never move
__device__ __forceinline__ void cat_row_grad_masked(const float *__restrict__ z, const MaskedCatRow &c, int A,
                                                    uint32_t valid, int act, float dlp, float dH,
                                                    float *__restrict__ dzr)
{
    for (int a = 0; a < A; ++a) dzr[a] = 0.0f;
    for (uint32_t b = valid; b; b &= b - 1u) {
        const int a = __builtin_ctz(b);
        const MaskedTerm t = masked_term(z[a], c);
        const float pe = expf(t.ln);   // softmax(z) as seen by logsumexp backward
        dzr[a] = dlp * ((a == act ? 1.0f : 0.0f) - pe) + dH * (t.p * (c.pg - t.g));
    }
}

// loss_row under a mask; z[A] = the value.  Every set bit of valid is below A (the entries check)
__device__ __forceinline__ void loss_row_masked(const float *__restrict__ z, int A, uint32_t valid, int act, float olp,
                                                float ov, float adv, float ret, const LossArgs &la, float invB,
                                                float *__restrict__ dzr, double (&acc)[kNumSums])
{
    const float v = z[A];
    const MaskedCatRow c = cat_row_masked(z, valid, act);
    const PpoRowTerms t = ppo_row_terms(c.lp, olp, v, ov, adv, ret, la);
    ppo_row_sums(t, c.H, c.lp, olp, v, adv, ret, la, acc);
    cat_row_grad_masked(z, c, A, valid, act, ppo_row_dlp(t, adv, la, invB), -la.ent_coef * invB, dzr);
    dzr[A] = ppo_row_dvalue(t, la, invB);
}

// metrics record from the sums 0..12 (shared by k_loss, the fused path's k_metrics_all, the
// one-hidden-layer update and the NatureCNN's cnn_write_metrics); GS_M_GRAD_NORM is the caller's.
// Returns whether approx_kl passed target_kl (the KL early stop)
__device__ __forceinline__ bool write_metrics(const double *t, double Bd, const LossArgs &la, float *metrics,
                                              bool adv_stats)
{
    const float pl = (float)(-t[0] / Bd);
    const float vl = (float)(t[1] / Bd);
    const float ent = (float)(t[2] / Bd);
    const float loss = pl + la.vf_coef * vl + la.ent_coef * (-ent);
    const double var_rv = (t[8] - t[7] * t[7] / Bd) / (Bd - 1.0);
    const double var_r = (t[10] - t[9] * t[9] / Bd) / (Bd - 1.0);
    const float approx_kl = (float)(t[6] / Bd);
    const bool kl_stop = la.target_kl > 0.0f && approx_kl > la.target_kl;
    metrics[GS_M_LOSS] = loss;
    metrics[GS_M_POLICY_LOSS] = pl;
    metrics[GS_M_VALUE_LOSS] = vl;
    metrics[GS_M_ENTROPY] = ent;
    metrics[GS_M_CLIP_FRAC] = (float)(t[3] / Bd);
    metrics[GS_M_CLIP_FRAC_VF] = (float)(t[4] / Bd);
    metrics[GS_M_EXPLAINED_VAR] = (float)(1.0 - var_rv / var_r);
    metrics[GS_M_KL] = (float)(t[5] / Bd);
    metrics[GS_M_APPROX_KL] = approx_kl;
    if (adv_stats) {
        const double amean = t[11] / Bd;
        const double astd = sqrt(fmax(0.0, (t[12] - t[11] * t[11] / Bd) / (Bd - 1.0)));
        metrics[GS_M_ADV_NORM_MEAN] = la.normalize ? (float)amean : 0.0f;
        metrics[GS_M_ADV_NORM_STD] = la.normalize ? (float)astd : 0.0f;
    }
    metrics[GS_M_KL_STOP] = kl_stop ? 1.0f : 0.0f;
    metrics[GS_M_SKIPPED] = kl_stop ? 1.0f : 0.0f;
    metrics[GS_M_UNEVALUATED] = 0.0f;
    metrics[GS_M_RES1] = 0.0f;
    return kl_stop;
}

// the record of a minibatch after the sticky KL stop (never evaluated): every slot 0 but these three
__device__ __forceinline__ float unevaluated_slot(int q)
{
    return (q == GS_M_SKIPPED || q == GS_M_KL_STOP || q == GS_M_UNEVALUATED) ? 1.0f : 0.0f;
}

// behind write_metrics in k_update1 and k_ppo_rows_step: the pre-clip norms, then zeros to the record's end
__device__ __forceinline__ void write_step_tail(float *rec, float total, float gn_back, float gn_pol, float gn_val)
{
    rec[GS_M_GRAD_NORM] = total;
    rec[GS_M_GN_BACKBONE] = gn_back;
    rec[GS_M_GN_POLICY_HEAD] = gn_pol;
    rec[GS_M_GN_VALUE_HEAD] = gn_val;
    rec[GS_M_GN_MLP] = 0.0f;
    for (int q = GS_M_RES20; q < GS_NUM_METRICS; ++q) rec[q] = 0.0f;
}

// A layer's GS_M_ACT quadruple out[4] = {mean, unbiased std, dead_pct, dead_max} (float in a record, double
// for gs_cnn_activation_stats) from the double sums over its n = rows x neurons pre-activation values:
// s1 = sum z, s2 = sum z^2, dead_sum / dead_max = the sum / the largest of the per-neuron act_dead counts
template <class T>
__device__ __forceinline__ void act_quad(double s1, double s2, double dead_sum, double dead_max, double n, double rows,
                                         T *out)
{
    const double var = (s2 - s1 * s1 / n) / (n - 1.0);
    out[0] = (T)(s1 / n);
    out[1] = (T)sqrt(var > 0.0 ? var : 0.0);
    out[2] = (T)(dead_sum / n);
    out[3] = (T)(dead_max / rows);
}

}  // namespace gs
