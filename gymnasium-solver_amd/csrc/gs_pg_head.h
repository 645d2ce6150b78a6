// gs_pg_head.h — the per-row arithmetic of the REINFORCE update (gs_pg.hip) on top of gs_head.h's
// categorical row (cat_row, cat_row_grad): one minibatch row of REINFORCEAgent.losses_for_batch
// (agents/reinforce/reinforce_agent.py:11-88) with its analytic gradient.
// Unlike gs_mlp.hip / gs_mlp1.hip, gs_pg.hip compiles with the default -ffp-contract (FMA): the
// shared source need not round as the PPO path's does (no result is shared between the two), and
// the contracted dot products carry one rounding less per term.
#pragma once

#include "gs_head.h"

namespace gs {

constexpr int kPgMaxGroups = 256;  // row workgroups (and partial slots) at most: the MI355X's CU count
constexpr int kPgMaxHidden = 512;
constexpr int kPgStepGroups = 64;  // step workgroups at most
// metric sums of one minibatch: logp * t, entropy, old logp - logp, approx kl, t, t^2
constexpr int kPgSums = 6;

// z: the row's raw policy logits (z[A] unused: the value head is outside the loss); t: its policy
// target, already normalised.  loss = -mean(lp t) - ent_coef mean(H): writes dLoss/dlogits to dzr
// and adds the row's terms to the sums.
template <int AMAX>
__device__ __forceinline__ void pg_loss_row(const float (&z)[AMAX + 1], int A, int act, float olp, float t,
                                            float ent_coef, float invB, float *__restrict__ dzr,
                                            double (&acc)[kPgSums])
{
    const CatRow<AMAX> c = cat_row<AMAX>(z, A, act);
    acc[0] += (double)(c.lp * t);
    acc[1] += (double)c.H;
    acc[2] += (double)(olp - c.lp);
    acc[3] += (double)approx_kl_row(c.lp, olp);
    acc[4] += (double)t;
    acc[5] += (double)t * (double)t;
    cat_row_grad<AMAX>(c, A, act, -t * invB, -ent_coef * invB, dzr);
}

}  // namespace gs
