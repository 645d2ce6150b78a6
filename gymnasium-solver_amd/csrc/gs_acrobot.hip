// gs_acrobot.hip — device-resident Acrobot-v1 dynamics.
//
// The reference trains `Acrobot-v1:ppo` on gymnasium 1.x's AcrobotEnv (not vendored: gymnasium is
// absent offline, so parity with its trajectories is UNPINNED, exactly as for CartPole).  The
// published dynamics are restated in gs_acrobot_env.h (the env type, shared with the
// one-launch rollout; the kernels are gs_env_kernels.h's): "book" equations, one RK4 step of dt = 0.2 in double precision, bounded
// angle wraps, velocity clamps, termination above the line, reward -1 (0 on the terminating
// step), TimeLimit truncation at 500 steps, and the vector env's NEXT_STEP autoreset: the step
// after a done resets that env, ignores its action and returns the reset observation with
// reward 0 and no done flag.  Reset states are uniform in [-0.1, 0.1) from a counter-based hash,
// rounded to float32 (numpy's PCG64 stream is not reproduced).  The numpy twin is
// tests/acrobot_twin.py.
#include "gs_env_kernels.h"
#include "gs_acrobot_env.h"

using namespace gs;

extern "C" int gs_acrobot_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int64_t N,
                                uint64_t seed, int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev, "gs_acrobot_reset: bad argument");
    const AcrobotEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, seed, env_offset},
                              state_dev};
    return launch_env_reset<AcrobotEnv>(ev, N, stream);
}

extern "C" int gs_acrobot_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                               const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                               int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                               uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                               float *ep_len_sum_dev, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_acrobot_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_acrobot_step: null output row");
    const AcrobotEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                               max_steps, seed, env_offset},
                              state_dev};
    return launch_env_step<AcrobotEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev, stream);
}
