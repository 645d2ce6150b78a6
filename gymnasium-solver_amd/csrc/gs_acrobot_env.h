// gs_acrobot_env.h — device Acrobot-v1: the env type AcrobotEnv behind its step kernels
// (gs_acrobot.hip) and the one-launch rollout (gs_mlp.hip k_rollout_env), see gs_env_episode.h.
// Twin: tests/acrobot_twin.py.
//
// gymnasium is not vendored and not installed, so the dynamics are restated from the published
// gymnasium 1.x AcrobotEnv ("book" variant, no torque noise) and parity with gymnasium's own
// episodes is UNPINNED, exactly as for CartPole: one classical RK4 step of dt = 0.2 in double
// precision, angles wrapped into [-pi, pi], velocities clamped to 4 pi / 9 pi, termination when
// the tip is above the line (-cos t1 - cos(t1 + t2) > 1), reward -1 (0 on the terminating step),
// TimeLimit truncation, NEXT_STEP autoreset.  Reset draws are uniform in [-0.1, 0.1) from the
// counter hash, rounded to float32 (gymnasium's reset casts its state to float32).
#pragma once

#include "gs_env_episode.h"

namespace gs {

struct ACState {      // per env: theta1, theta2, omega1, omega2
    double t1, t2, w1, w2;
};

constexpr double kAcDt = 0.2;
constexpr double kAcMaxVel1 = 4.0 * M_PI, kAcMaxVel2 = 9.0 * M_PI;
// The wrap loops are bounded, so that a non-finite state cannot spin a wave forever.  Why 16
// turns are never needed from a state in the box (|t| <= pi, |w1| <= 4 pi, |w2| <= 9 pi):
//  - the exact flow: the mass matrix M(t2) = [[d1, d2], [d2, 1.25]] has d1 = 3.5 + cos t2 in
//    [2.5, 4.5], trace <= 5.75 and det = 1.25 d1 - d2^2 >= 2.56, so its eigenvalues lie in
//    [0.445, 5.75].  The kinetic energy starts below 5.75 / 2 * (16 + 81) pi^2 = 2753; gravity
//    adds at most 39.2 (twice 4.9 + 14.7) and the torque |a| <= 1 at most |delta t2|, so
//    |w|^2 <= 2 * 2800 / 0.445 along the step: |w| <= 113 rad/s, and 0.2 s move an angle by at
//    most 22.5 rad = 3.6 turns;
//  - the RK4 step is not the exact flow (at the velocity caps it is far from converged), and a
//    stage-by-stage worst-case bound of the quadratic velocity terms is useless (it grows to
//    1e6 rad), so the step itself was evaluated: over 3e7 states, uniform over the box and on
//    its velocity faces, with every action, an angle moved by at most 27.3 rad = 4.4 turns, so
//    it ends at most 4.9 turns out and wraps in 5 iterations.
// The cap is three times that.  The twin has the same cap; past it the angle stays as it is.
constexpr int kAcWrapCap = 16;

__device__ __forceinline__ double acrobot_reset_uniform(uint64_t seed, uint64_t env, uint64_t episode, int c)
{
    return (double)(float)(-0.1 + 0.2 * env_reset_unit(seed, env, episode, c));
}

__device__ __forceinline__ void acrobot_reset_state(ACState &s, uint64_t seed, uint64_t ge, uint64_t episode)
{
    s.t1 = acrobot_reset_uniform(seed, ge, episode, 0);
    s.t2 = acrobot_reset_uniform(seed, ge, episode, 1);
    s.w1 = acrobot_reset_uniform(seed, ge, episode, 2);
    s.w2 = acrobot_reset_uniform(seed, ge, episode, 3);
}

// the observation {cos t1, sin t1, cos t2, sin t2, w1, w2}
__device__ __forceinline__ void acrobot_write_obs(const ACState &s, float *o)
{
    o[0] = (float)cos(s.t1);
    o[1] = (float)sin(s.t1);
    o[2] = (float)cos(s.t2);
    o[3] = (float)sin(s.t2);
    o[4] = (float)s.w1;
    o[5] = (float)s.w2;
}

// AcrobotEnv._dsdt, "book" variant: the time derivative of {t1, t2, w1, w2} under torque a
__device__ __forceinline__ ACState acrobot_dsdt(const ACState &y, double a)
{
    const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
    const double c2 = cos(y.t2), s2 = sin(y.t2);
    const double d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * c2) + I1 + I2;
    const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    const double phi2 = m2 * lc2 * g * cos(y.t1 + y.t2 - M_PI / 2.0);
    const double phi1 = -m2 * l1 * lc2 * (y.w2 * y.w2) * s2 - 2.0 * m2 * l1 * lc2 * y.w2 * y.w1 * s2 +
                        (m1 * lc1 + m2 * l1) * g * cos(y.t1 - M_PI / 2.0) + phi2;
    const double dw2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (y.w1 * y.w1) * s2 - phi2) /
                       (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1);
    const double dw1 = -(d2 * dw2 + phi1) / d1;
    return ACState{y.w1, y.w2, dw1, dw2};
}

__device__ __forceinline__ double acrobot_wrap(double x)
{
    for (int i = 0; i < kAcWrapCap && x > M_PI; ++i) x -= 2.0 * M_PI;
    for (int i = 0; i < kAcWrapCap && x < -M_PI; ++i) x += 2.0 * M_PI;
    return x;
}

__device__ __forceinline__ double acrobot_clamp(double x, double lim)
{
    return x < -lim ? -lim : (x > lim ? lim : x);
}

// AcrobotEnv.step: one RK4 step, wrap and clamp; returns terminated
__device__ __forceinline__ bool acrobot_dynamics(ACState &s, int64_t action)
{
    const double a = (double)(action - 1);
    // classical RK4, y' = y + dt/6 (k1 + 2 k2 + 2 k3 + k4); the stages share one copy of the
    // derivative's code (stage 0 reads y + 0 * 0 = y)
    const double cs[4] = {0.0, kAcDt / 2.0, kAcDt / 2.0, kAcDt}, ws[4] = {1.0, 2.0, 2.0, 1.0};
    ACState k{0.0, 0.0, 0.0, 0.0}, acc{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const ACState y{s.t1 + cs[i] * k.t1, s.t2 + cs[i] * k.t2, s.w1 + cs[i] * k.w1, s.w2 + cs[i] * k.w2};
        k = acrobot_dsdt(y, a);
        acc.t1 += ws[i] * k.t1;
        acc.t2 += ws[i] * k.t2;
        acc.w1 += ws[i] * k.w1;
        acc.w2 += ws[i] * k.w2;
    }
    s.t1 = acrobot_wrap(s.t1 + kAcDt / 6.0 * acc.t1);
    s.t2 = acrobot_wrap(s.t2 + kAcDt / 6.0 * acc.t2);
    s.w1 = acrobot_clamp(s.w1 + kAcDt / 6.0 * acc.w1, kAcMaxVel1);
    s.w2 = acrobot_clamp(s.w2 + kAcDt / 6.0 * acc.w2, kAcMaxVel2);
    return -cos(s.t1) - cos(s.t1 + s.t2) > 1.0;
}

struct AcrobotEnv : DynEnv<ACState, 6, 3, acrobot_reset_state, acrobot_write_obs> {
    using Args = DynEnvArgs;
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (reset_row(ev, me)) return EnvStepOut{};
        const bool terminated = acrobot_dynamics(s, action);
        return finish_step(ev, me, terminated ? 0.0f : -1.0f, terminated);
    }
};

}  // namespace gs
