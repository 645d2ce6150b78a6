// gs_hparams.h — host side: the LossArgs / AdamArgs constants (gs_common.h) formed from the
// hyper-parameters, in one place for every update path (gs_ppo.hip, gs_mlp1.hip, gs_cnn.hip,
// gs_pg.hip), so each value a kernel reads comes from one double-precision expression and one
// cast.  The callers add what is theirs: batch rows, global-mode pointers, bf16, the slot and
// partial counts, an exchange's grad_scale.
#pragma once

#include <math.h>

#include "gs_common.h"

namespace gs {

inline LossArgs loss_args(const gs_ppo_hparams &hp)
{
    LossArgs la{};
    la.clip_lo = (float)(1.0 - (double)hp.clip_range);
    la.clip_hi = (float)(1.0 + (double)hp.clip_range);
    la.clip_vf = hp.clip_range_vf;
    la.vf_coef = hp.vf_coef;
    la.ent_coef = hp.ent_coef;
    la.target_kl = hp.target_kl;
    la.normalize = hp.normalize_adv;
    return la;
}

// the optimizer a flags word asks for (GS_HP_OPT_*; both bits: opt_flags_ok refuses them first)
inline int opt_kind(int32_t flags)
{
    return (flags & GS_HP_OPT_ADAMW) ? kOptAdamW : (flags & GS_HP_OPT_SGD) ? kOptSGD : kOptAdam;
}
inline bool opt_flags_ok(int32_t flags)
{
    return (flags & (GS_HP_OPT_ADAMW | GS_HP_OPT_SGD)) != (GS_HP_OPT_ADAMW | GS_HP_OPT_SGD);
}
// the first check of every entry that takes an optimizer step
#define GS_REQUIRE_OPT_FLAGS(flags, what)                                                                       \
    GS_REQUIRE(gs::opt_flags_ok(flags), "%s: the optimizer bits GS_HP_OPT_ADAMW and GS_HP_OPT_SGD are both set " \
                                        "(flags 0x%x): one optimizer per update", what, (unsigned)(flags))

// torch.optim.Adam's constants of step t (1-based); grad_scale 1: no exchange.  flags' optimizer
// bits: AdamW adds the decay factor of this call's lr; SGD's step size is f32(-lr), for every t
inline AdamArgs adam_args(float lr, float beta1, float beta2, float eps, float max_grad_norm, int64_t t,
                          int32_t flags = 0)
{
    AdamArgs a{};
    const double b1 = beta1, b2 = beta2;
    const double bc1 = 1.0 - pow(b1, (double)t);
    const double bc2 = 1.0 - pow(b2, (double)t);
    a.max_norm = max_grad_norm;
    a.one_minus_b1 = (float)(1.0 - b1);
    a.b2 = (float)b2;
    a.one_minus_b2 = (float)(1.0 - b2);
    a.neg_step_size = (float)(-(double)lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    a.eps = eps;
    a.grad_scale = 1.0f;
    a.opt = opt_kind(flags);
    a.decay = a.opt == kOptAdamW ? (float)(1.0 - (double)lr * GS_ADAMW_WEIGHT_DECAY) : 1.0f;
    if (a.opt == kOptSGD) a.neg_step_size = (float)(-(double)lr);
    return a;
}

inline AdamArgs adam_args(const gs_ppo_hparams &hp, int64_t t)
{
    return adam_args(hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps, hp.max_grad_norm, t, hp.flags);
}

}  // namespace gs
