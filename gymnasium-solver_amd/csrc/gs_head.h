// gs_head.h — the per-row arithmetic the MLP kernels of gs_mlp.hip (two hidden layers) and
// gs_mlp1.hip (one hidden layer) share, so both round identically: the categorical head
// (log-softmax statistics, action select, log-prob), one row of the PPO loss with its analytic
// gradients, the metric record, the fixed-order block sum, the clip coefficient and one
// parameter's Adam step.  Both files compile with -ffp-contract=off.
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
// One minibatch row of PPOAgent.losses_for_batch (agents/ppo/ppo_agent.py:21-152) with its
// analytic gradients: z = raw logits | value, adv already batch-normalised.  Writes
// dLoss/dlogits | dLoss/dvalue to dzr and adds the row's terms to the 14 metric sums.
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
    const HeadRow h = head_stats<AMAX>(z, A);
    const float invS = 1.0f / h.S;
    // ln = normalised logits, p = softmax(ln) (Categorical.probs), pe = exp(ln)
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
    H = -H;
    const float ratio = expf(lp - olp);
    const float rc = fminf(fmaxf(ratio, la.clip_lo), la.clip_hi);
    const float s1 = adv * ratio, s2 = adv * rc;
    const float mn = fminf(s1, s2);
    const float vdelta = v - ov;
    const float du = v - ret;
    const float vu = du * du;
    const float vcl = ov + fminf(fmaxf(vdelta, -la.clip_vf), la.clip_vf);
    const float dc = vcl - ret;
    const float vc = dc * dc;
    const float vmax = fmaxf(vu, vc);
    const float ldiff = fminf(fmaxf(lp - olp, -20.0f), 20.0f);
    const float r2 = expf(ldiff);
    const float akl = (r2 - 1.0f) - logf(r2);
    const float rv = ret - v;
    acc[0] += (double)mn;
    acc[1] += (double)vmax;
    acc[2] += (double)H;
    acc[3] += (ratio < la.clip_lo || ratio > la.clip_hi) ? 1.0 : 0.0;
    acc[4] += (vdelta < -la.clip_vf || vdelta > la.clip_vf) ? 1.0 : 0.0;
    acc[5] += (double)(olp - lp);
    acc[6] += (double)akl;
    acc[7] += (double)rv;
    acc[8] += (double)rv * (double)rv;
    acc[9] += (double)ret;
    acc[10] += (double)ret * (double)ret;
    acc[11] += (double)adv;
    acc[12] += (double)adv * (double)adv;
    // ---- analytic gradients (torch autograd tie rules: min/max ties split halves)
    const float ga = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float gb = s2 < s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float inclip = (ratio >= la.clip_lo && ratio <= la.clip_hi) ? 1.0f : 0.0f;
    const float g_mn = -invB;
    const float dratio = adv * (g_mn * ga) + adv * (g_mn * gb) * inclip;
    const float dlp = dratio * ratio;
    const float dH = -la.ent_coef * invB;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
        if (a < A) {
            const float pe = expf(ln[a]);   // softmax(z) as seen by logsumexp backward
            float g = dlp * ((a == act ? 1.0f : 0.0f) - pe);
            g += dH * (-p[a] * (ln[a] + H));
            dzr[a] = g;
        }
    }
    const float hu = vu > vc ? 1.0f : (vu == vc ? 0.5f : 0.0f);
    const float hc = vc > vu ? 1.0f : (vu == vc ? 0.5f : 0.0f);
    const float invc = (vdelta >= -la.clip_vf && vdelta <= la.clip_vf) ? 1.0f : 0.0f;
    const float gv = la.vf_coef * invB;
    dzr[A] = (gv * hu) * (2.0f * du) + (gv * hc) * (2.0f * dc) * invc;
}

// metrics record from the 14 sums (shared by k_loss, the fused path's k_metrics_all and the
// one-hidden-layer update)
__device__ __forceinline__ void write_metrics(const double *t, double Bd, const LossArgs &la, float *metrics,
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
}

}  // namespace gs
