// gs_cartpole_env.h — device CartPole-v1's per-env arithmetic, shared by its step kernels
// (gs_cartpole.hip) and the one-launch rollout (gs_mlp.hip k_rollout_env), so both produce the
// same bits.  Both files compile with -ffp-contract=off.  Twin: oracle/cartpole_ref.py.
// Also the pieces every device env with real dynamics shares: the counter hash of the reset
// draws and the step's result.  At the end: the reference's CartPoleV1_RewardShaper on top of the
// same step (cartpole_phi, cartpole_shaped_env_step; twin tests/cartpole_shaper_twin.py).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/gsamd.h"   // gs_cartpole_wrappers

namespace gs {

__device__ __forceinline__ uint64_t env_mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// uniform in [0, 1): 53-bit mantissa from the hash of (seed, env, episode, component)
__device__ __forceinline__ double env_reset_unit(uint64_t seed, uint64_t env, uint64_t episode, int c)
{
    const uint64_t h = env_mix64(env_mix64(env_mix64(env_mix64(seed) ^ env) ^ episode) ^ (uint64_t)(0xC0 + c));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// what one env step writes into the rollout rows
struct EnvStepOut {
    float reward;
    bool done, timeout;
};

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

// One env's step: state, meta {steps, episodes, pending} and the running return advance; on a
// done the (null-tolerant) episode counters add the finished episode.  ge = the global env index.
__device__ __forceinline__ EnvStepOut cartpole_env_step(CPState &s, int32_t (&meta)[3], float &er, int64_t action,
                                                        int max_steps, uint64_t seed, uint64_t ge, int32_t *ep_cnt,
                                                        float *ep_ret_sum, float *ep_len_sum)
{
    if (meta[2] != 0) {        // NEXT_STEP autoreset: this step only resets
        cartpole_reset_state(s, seed, ge, (uint64_t)meta[1]);
        meta[0] = 0;
        meta[2] = 0;
        er = 0.0f;
        return EnvStepOut{0.0f, false, false};
    }
    // gymnasium CartPoleEnv.step (euler)
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
    const bool terminated = s.x < -x_threshold || s.x > x_threshold || s.theta < -theta_threshold ||
                            s.theta > theta_threshold;
    const int steps = meta[0] + 1;
    const bool truncated = !terminated && steps >= max_steps;
    er = er + 1.0f;
    if (terminated || truncated) {
        if (ep_cnt) *ep_cnt += 1;
        if (ep_ret_sum) *ep_ret_sum += er;
        if (ep_len_sum) *ep_len_sum += (float)steps;
        meta[1] += 1;
        meta[2] = 1;
    }
    meta[0] = steps;
    return EnvStepOut{1.0f, terminated || truncated, truncated};
}

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

// One env's step under the shaper: cartpole_env_step's dynamics, flags, meta and reset hash, with
// reward = (float)(1.0 + (phi - prev_phi)) and the running return adding that reward.  The
// wrapper's reset() takes the reset observation's potential, so a NEXT_STEP autoreset row stays
// reward 0 and re-arms prev_phi.
__device__ __forceinline__ EnvStepOut cartpole_shaped_env_step(CPState &s, double &prev_phi, int32_t (&meta)[3],
                                                               float &er, int64_t action, int max_steps,
                                                               uint64_t seed, uint64_t ge,
                                                               const gs_cartpole_wrappers &w, int32_t *ep_cnt,
                                                               float *ep_ret_sum, float *ep_len_sum)
{
    const bool reset_row = meta[2] != 0;
    float unshaped = 0.0f;     // the dynamics' own return accumulator is not this env's
    const EnvStepOut so = cartpole_env_step(s, meta, unshaped, action, max_steps, seed, ge, nullptr, nullptr, nullptr);
    const double phi = cartpole_phi(w, s);
    if (reset_row) {
        prev_phi = phi;
        er = 0.0f;
        return so;
    }
    const float reward = (float)(1.0 + (phi - prev_phi));
    prev_phi = phi;
    er = er + reward;
    if (so.done) {
        if (ep_cnt) *ep_cnt += 1;
        if (ep_ret_sum) *ep_ret_sum += er;
        if (ep_len_sum) *ep_len_sum += (float)meta[0];
    }
    return EnvStepOut{reward, so.done, so.timeout};
}

}  // namespace gs
