// gs_pg_head.h — the per-row arithmetic of the REINFORCE update (gs_pg.hip) on top of the shared
// categorical head of gs_head.h: one minibatch row of REINFORCEAgent.losses_for_batch
// (agents/reinforce/reinforce_agent.py:11-88) with its analytic gradient.
// Unlike gs_mlp.hip / gs_mlp1.hip, gs_pg.hip compiles with the default -ffp-contract (FMA): its
// head_stats / adam_param calls need not round as the PPO path's do (no result is shared between
// the two), and the contracted dot products carry one rounding less per term.
#pragma once

#include "gs_head.h"

namespace gs {

constexpr int kPgRows = 16;        // minibatch rows of one tile
constexpr int kPgMaxGroups = 256;  // row workgroups (and partial slots) at most: the MI355X's CU count
constexpr int kPgMaxHidden = 512;
constexpr int kPgStepGroups = 64;  // step workgroups at most
// metric sums of one minibatch: logp * t, entropy, old logp - logp, approx kl, t, t^2
constexpr int kPgSums = 6;

// z: the row's raw policy logits (z[A] unused: the value head is outside the loss); t: its policy
// target, already normalised.  loss = -mean(lp t) - ent_coef mean(H): writes dLoss/dlogits to dzr
// (entropy term as loss_row's) and adds the row's terms to the sums.
template <int AMAX>
__device__ __forceinline__ void pg_loss_row(const float (&z)[AMAX + 1], int A, int act, float olp, float t,
                                            float ent_coef, float invB, float *__restrict__ dzr,
                                            double (&acc)[kPgSums])
{
    const HeadRow h = head_stats<AMAX>(z, A);
    const float invS = 1.0f / h.S;
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
    const float ldiff = fminf(fmaxf(lp - olp, -20.0f), 20.0f);
    const float r2 = expf(ldiff);
    const float akl = (r2 - 1.0f) - logf(r2);
    acc[0] += (double)(lp * t);
    acc[1] += (double)H;
    acc[2] += (double)(olp - lp);
    acc[3] += (double)akl;
    acc[4] += (double)t;
    acc[5] += (double)t * (double)t;
    const float dlp = -t * invB;
    const float dH = -ent_coef * invB;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
        if (a < A) {
            const float pe = expf(ln[a]);   // softmax(z) as seen by logsumexp backward
            float g = dlp * ((a == act ? 1.0f : 0.0f) - pe);
            g += dH * (-p[a] * (ln[a] + H));
            dzr[a] = g;
        }
    }
}

}  // namespace gs
