// gs_cartpole_env.h — device CartPole-v1: the env type CartPoleEnv behind its step kernels
// (gs_cartpole.hip) and the one-launch rollout (gs_mlp.hip k_rollout_env), see gs_env_episode.h.
// Twin: oracle/cartpole_ref.py.  At the end: the reference's CartPoleV1_RewardShaper on top of the
// same dynamics (cartpole_phi, CartPoleShapedEnv; twin tests/cartpole_shaper_twin.py).
#pragma once

#include "gs_env_episode.h"

namespace gs {

struct CPState {      // per env, double precision like gymnasium's Python-float state
    double x, x_dot, theta, theta_dot;
};

// uniform in [-0.05, 0.05)
__device__ __forceinline__ double cartpole_reset_uniform(uint64_t seed, uint64_t env, uint64_t episode, int c)
{
    return -0.05 + 0.1 * env_reset_unit(seed, env, episode, c);
}

__device__ __forceinline__ void cartpole_reset_state(CPState &s, uint64_t seed, uint64_t ge, uint64_t episode)
{
    s.x = cartpole_reset_uniform(seed, ge, episode, 0);
    s.x_dot = cartpole_reset_uniform(seed, ge, episode, 1);
    s.theta = cartpole_reset_uniform(seed, ge, episode, 2);
    s.theta_dot = cartpole_reset_uniform(seed, ge, episode, 3);
}

__device__ __forceinline__ void cartpole_write_obs(const CPState &s, float *o)
{
    o[0] = (float)s.x;
    o[1] = (float)s.x_dot;
    o[2] = (float)s.theta;
    o[3] = (float)s.theta_dot;
}

// gymnasium CartPoleEnv.step (euler): the state advances; returns terminated
__device__ __forceinline__ bool cartpole_dynamics(CPState &s, int64_t action)
{
    const double gravity = 9.8, masscart = 1.0, masspole = 0.1, total_mass = masspole + masscart;
    const double length = 0.5, polemass_length = masspole * length, force_mag = 10.0, tau = 0.02;
    const double theta_threshold = 12.0 * 2.0 * M_PI / 360.0, x_threshold = 2.4;
    const double force = action == 1 ? force_mag : -force_mag;
    const double costheta = cos(s.theta), sintheta = sin(s.theta);
    const double temp = (force + polemass_length * (s.theta_dot * s.theta_dot) * sintheta) / total_mass;
    const double thetaacc = (gravity * sintheta - costheta * temp) /
                            (length * (4.0 / 3.0 - masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    s.x = s.x + tau * s.x_dot;
    s.x_dot = s.x_dot + tau * xacc;
    s.theta = s.theta + tau * s.theta_dot;
    s.theta_dot = s.theta_dot + tau * thetaacc;
    return s.x < -x_threshold || s.x > x_threshold || s.theta < -theta_threshold || s.theta > theta_threshold;
}

struct CartPoleEnv : DynEnv<CPState, 4, 2, cartpole_reset_state, cartpole_write_obs> {
    using Args = DynEnvArgs;
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (reset_row(ev, me)) return EnvStepOut{};
        const bool terminated = cartpole_dynamics(s, action);
        return finish_step(ev, me, 1.0f, terminated);
    }
};

// CartPoleV1_RewardShaper._phi (the reference's gym_wrappers/CartPoleV1/reward_shaper.py) on the
// float32 observation's x and theta, in double as the class's float(obs[i]) arithmetic; the
// thresholds are the env's own (x_threshold, theta_threshold_radians).  No shaper: 0.
__device__ __forceinline__ double cartpole_phi(const gs_cartpole_wrappers &w, float x_obs, float theta_obs)
{
    if (!w.shaper) return 0.0;
    const double theta_threshold = 12.0 * 2.0 * M_PI / 360.0, x_threshold = 2.4;
    const double x = (double)x_obs, theta = (double)theta_obs;
    double pos = 1.0 - fabs(x) / fmax(x_threshold, 1e-6);
    double ang = 1.0 - fabs(theta) / fmax(theta_threshold, 1e-6);
    if (w.clip_potential) {
        pos = pos < 0.0 ? 0.0 : (pos > 1.0 ? 1.0 : pos);
        ang = ang < 0.0 ? 0.0 : (ang > 1.0 ? 1.0 : ang);
    }
    return w.angle_reward_scale * ang + w.position_reward_scale * pos;
}

__device__ __forceinline__ double cartpole_phi(const gs_cartpole_wrappers &w, const CPState &s)
{
    return cartpole_phi(w, (float)s.x, (float)s.theta);
}

// The env under the shaper: CartPoleEnv's dynamics, flags, meta and reset hash, with reward =
// (float)(1.0 + (phi - prev_phi)) and the running return adding that reward.  The wrapper's
// reset() takes the reset observation's potential, so a NEXT_STEP autoreset row stays reward 0
// and re-arms prev_phi.  The previous potentials are an (N) f64 tensor of their own; thread `me`
// keeps its env's in a register.
struct CartPoleShapedEnv : CartPoleEnv {
    struct Args : DynEnvArgs {
        double *prev_phi;
        gs_cartpole_wrappers w;
    };
    double prev_phi;
    __device__ __forceinline__ void load(const Args &ev, int64_t me)
    {
        CartPoleEnv::load(ev, me);
        prev_phi = ev.prev_phi[me];
    }
    __device__ __forceinline__ void store(const Args &ev, int64_t me) const
    {
        CartPoleEnv::store(ev, me);
        ev.prev_phi[me] = prev_phi;
    }
    __device__ __forceinline__ void reset(const Args &ev, int64_t me)
    {
        CartPoleEnv::reset(ev, me);
        prev_phi = cartpole_phi(ev.w, s);
    }
    __device__ __forceinline__ EnvStepOut step(const Args &ev, int64_t me, int64_t action)
    {
        if (reset_row(ev, me)) {
            prev_phi = cartpole_phi(ev.w, s);
            return EnvStepOut{};
        }
        const bool terminated = cartpole_dynamics(s, action);
        const double phi = cartpole_phi(ev.w, s);
        const float reward = (float)(1.0 + (phi - prev_phi));
        prev_phi = phi;
        return finish_step(ev, me, reward, terminated);
    }
};

}  // namespace gs
