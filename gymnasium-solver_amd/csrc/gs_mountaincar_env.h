// gs_mountaincar_env.h — device MountainCar-v0 and its two reward wrappers: the env type
// MountainCarEnv behind the step kernels (gs_mountaincar.hip) and the one-launch rollout
// (gs_mlp.hip k_rollout_env), see gs_env_episode.h.  Twin: tests/mountaincar_twin.py.
//
// gymnasium is not vendored and not installed, so the dynamics are restated from the published
// gymnasium 1.x MountainCarEnv and parity with gymnasium's own episodes is UNPINNED, exactly as
// for CartPole and Acrobot: in double precision, v += (a - 1) 0.001 + cos(3 p) (-0.0025), v
// clipped to +-0.07, p += v, p clipped to [-1.2, 0.6], v = 0 at the left wall, terminated when
// p >= 0.5 and v >= 0, reward -1 on every step (the terminating one included), TimeLimit
// truncation, NEXT_STEP autoreset.  The reset position is uniform in [-0.6, -0.4) from the counter
// hash and stays a double (gymnasium keeps this env's state in float64), the reset velocity is 0.
//
// The wrappers restate the reference's gym_wrappers/MountainCarV0/{reward_shaper,
// state_count_bonus}.py, which read only the float32 observation: they work in double on
// (double)(float)p and (double)(float)v (numpy 1.x promotes float32 scalar x Python float to
// float64), in the config's list order (first entry innermost, its addend first).
#pragma once

#include "gs_env_episode.h"

namespace gs {

struct MCState {      // per env: position, velocity, and the float32 observation the shaper last saw
    double p, v, prev_p, prev_v;
};

constexpr double kMcMinP = -1.2, kMcMaxP = 0.6, kMcGoalP = 0.5, kMcMaxV = 0.07, kMcGoalV = 0.0;
constexpr double kMcForce = 0.001, kMcGravity = 0.0025;
constexpr int kMcMaxCells = 16384;     // position_bins * velocity_bins of one env's count table

__device__ __forceinline__ void mountaincar_reset_state(MCState &s, uint64_t seed, uint64_t ge, uint64_t episode)
{
    s.p = -0.6 + 0.2 * env_reset_unit(seed, ge, episode, 0);
    s.v = 0.0;
    s.prev_p = (double)(float)s.p;     // the shaper's reset(): the reset observation is its prev
    s.prev_v = (double)(float)s.v;
}

__device__ __forceinline__ void mountaincar_write_obs(const MCState &s, float *o)
{
    o[0] = (float)s.p;
    o[1] = (float)s.v;
}

// MountainCarV0_RewardShaper.step: potential differences of position, velocity and height
// between the observation and the previous one
__device__ __forceinline__ double mountaincar_shaping(const gs_mountaincar_wrappers &w, double p, double v, double p0,
                                                      double v0)
{
    const double pos = w.position_reward_scale *
                       ((p - kMcMinP) / (kMcGoalP - kMcMinP) - (p0 - kMcMinP) / (kMcGoalP - kMcMinP));
    const double vel = w.velocity_reward_scale *
                       ((v - (-kMcMaxV)) / (kMcMaxV - (-kMcMaxV)) - (v0 - (-kMcMaxV)) / (kMcMaxV - (-kMcMaxV)));
    const double hgt = w.height_reward_scale * ((sin(3.0 * p) + 1.0) / 2.0 - (sin(3.0 * p0) + 1.0) / 2.0);
    return pos + vel + hgt;
}

__device__ __forceinline__ double mountaincar_clip01(double x) { return x < 0.0 ? 0.0 : (x > 0.999999 ? 0.999999 : x); }

// MountainCarV0_StateCountBonus.step on this env's table: the bonus of the cell's count before
// the visit, then the visit.  The integer clamps keep a non-finite observation inside the table.
__device__ __forceinline__ double mountaincar_bonus(const gs_mountaincar_wrappers &w, int32_t *table, double p, double v)
{
    const double pn = mountaincar_clip01((p - kMcMinP) / (kMcMaxP - kMcMinP));
    const double vn = mountaincar_clip01((v - (-kMcMaxV)) / (kMcMaxV - (-kMcMaxV)));
    int pb = (int)(pn * (double)w.position_bins), vb = (int)(vn * (double)w.velocity_bins);
    pb = pb < 0 ? 0 : (pb >= w.position_bins ? w.position_bins - 1 : pb);
    vb = vb < 0 ? 0 : (vb >= w.velocity_bins ? w.velocity_bins - 1 : vb);
    int32_t *cell = table + (pb * w.velocity_bins + vb);
    const int32_t c = *cell;
    const double eff = (double)(c > w.min_count ? c : w.min_count);
    double bonus;
    if (w.bonus_type == GS_MC_BONUS_COUNT) bonus = 1.0 / sqrt(eff);
    else if (w.bonus_type == GS_MC_BONUS_INVERSE) bonus = 1.0 / eff;
    else bonus = 1.0 / log(eff + 1.0);
    *cell = c + 1;
    return w.bonus_scale * bonus;
}

// null, or what is wrong with the wrappers (their order, the bonus' table and parameters): every
// MountainCar entry checks this before a launch, so no index leaves an env's table (gs_mountaincar.hip)
const char *mountaincar_wrappers_error(const gs_mountaincar_wrappers &w, const void *counts);

// The count tables are int32 [N][position_bins * velocity_bins] in HBM (null without a count
// bonus): thread `me` reads and bumps one cell of local env me's table per step.
struct MountainCarEnv : DynEnv<MCState, 2, 3, mountaincar_reset_state, mountaincar_write_obs> {
    struct Args : DynEnvArgs {
        int32_t *counts;
        gs_mountaincar_wrappers w;
    };
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (reset_row(ev, me)) return EnvStepOut{};        // no wrapper adds anything to the reset row
        const gs_mountaincar_wrappers &w = ev.w;
        int32_t *table = ev.counts ? ev.counts + me * ((int64_t)w.position_bins * w.velocity_bins) : nullptr;
        // gymnasium MountainCarEnv.step
        double v = s.v + ((double)(action - 1) * kMcForce + cos(3.0 * s.p) * (-kMcGravity));
        v = v < -kMcMaxV ? -kMcMaxV : (v > kMcMaxV ? kMcMaxV : v);
        double p = s.p + v;
        p = p < kMcMinP ? kMcMinP : (p > kMcMaxP ? kMcMaxP : p);
        if (p == kMcMinP && v < 0.0) v = 0.0;
        s.p = p;
        s.v = v;
        const bool terminated = p >= kMcGoalP && v >= kMcGoalV;
        // the wrappers, innermost first, on the float32 observation
        const double po = (double)(float)p, vo = (double)(float)v;
        double r = -1.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (w.order[i] == GS_MC_WRAP_SHAPER) r = r + mountaincar_shaping(w, po, vo, s.prev_p, s.prev_v);
            else if (w.order[i] == GS_MC_WRAP_BONUS) r = r + mountaincar_bonus(w, table, po, vo);
        }
        s.prev_p = po;
        s.prev_v = vo;
        return finish_step(ev, me, (float)r, terminated);
    }
};

}  // namespace gs
