// gs_cartpole.hip — device-resident CartPole-v1 dynamics.
//
// The reference trains on gymnasium 1.x `CartPole-v1` (not vendored: gymnasium is absent
// offline, so parity with its trajectories is UNPINNED).  This kernel restates its published
// dynamics: cart-pole constants, Euler integration with tau = 0.02 in double precision (the
// environment keeps its state as Python floats), termination at |x| > 2.4 or |theta| > 12 deg,
// TimeLimit truncation at 500 steps, reward 1, and the vector env's NEXT_STEP autoreset: the
// step after a done resets that env, ignores its action and returns the reset observation
// with reward 0 and no done flag (the zero-reward transition the reference trains on,
// SURVEY §8 a4).  Reset states are uniform in [-0.05, 0.05) from a counter-based hash
// (numpy's PCG64 stream is not reproduced).  The numpy twin is oracle/cartpole_ref.py.
// The env type lives in gs_cartpole_env.h, the kernels in gs_env_kernels.h.
// gs_cartpole_shaped_*: the same env under the reference's CartPoleV1_RewardShaper
// (CartPole-v1:ppo_rewardshaped), with the wrapper's previous potential in an (N) f64 tensor of
// its own; the (N, 4) state and the unshaped entries are unchanged.  The shaper's arithmetic is
// pinned to the reference's class by tests/golden/cartpole_shaper.npz.
#include "gs_env_kernels.h"
#include "gs_cartpole_env.h"

using namespace gs;

extern "C" int gs_cartpole_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int64_t N,
                                 uint64_t seed, int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev, "gs_cartpole_reset: bad argument");
    const CartPoleEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, seed, env_offset},
                               state_dev};
    return launch_env_reset<CartPoleEnv>(ev, N, stream);
}

extern "C" int gs_cartpole_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                                const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                                int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                                uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                                float *ep_len_sum_dev, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_cartpole_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_cartpole_step: null output row");
    const CartPoleEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                                max_steps, seed, env_offset},
                               state_dev};
    return launch_env_step<CartPoleEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev, stream);
}

extern "C" int gs_cartpole_shaped_reset(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                                        float *obs_dev, gs_cartpole_wrappers wrappers, int64_t N, uint64_t seed,
                                        int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && prev_phi_dev && meta_dev && ep_ret_dev && obs_dev,
               "gs_cartpole_shaped_reset: bad argument");
    const CartPoleShapedEnv::Args ev{
        {{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, seed, env_offset}, state_dev},
        prev_phi_dev,
        wrappers};
    return launch_env_reset<CartPoleShapedEnv>(ev, N, stream);
}

extern "C" int gs_cartpole_shaped_step(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                                       float *obs_dev, gs_cartpole_wrappers wrappers, const int64_t *actions_dev,
                                       int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                                       float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                                       int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                                       void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && prev_phi_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_cartpole_shaped_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_cartpole_shaped_step: null output row");
    const CartPoleShapedEnv::Args ev{{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                                       max_steps, seed, env_offset},
                                      state_dev},
                                     prev_phi_dev,
                                     wrappers};
    return launch_env_step<CartPoleShapedEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev,
                                              stream);
}
