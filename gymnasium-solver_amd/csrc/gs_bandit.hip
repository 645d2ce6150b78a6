// gs_bandit.hip — device-resident Bandit-v0, the reference's algorithm-correctness environment
// (gym_envs/mab_env.py MultiArmedBanditEnv).
//
// A stateless Gaussian multi-armed bandit: the observation is zeros(n_arms) on reset and after
// every step, the reward of arm a is mean[a] + std[a] z, the episode terminates after
// episode_length steps.  The env type and the normal draw are in gs_bandit_env.h (shared with
// the one-launch rollout), the kernels in gs_env_kernels.h.  numpy's PCG64 ziggurat stream is not
// reproduced: the draw is Box-Muller on the counter hash, so parity with the reference's own
// reward stream is UNPINNED, as parity with gymnasium's streams is for the other device envs.
// The arms' float32 means and stds travel by value in gs_bandit_spec.  The numpy twin is
// tests/bandit_twin.py.
#include "gs_env_kernels.h"
#include "gs_bandit_env.h"

namespace gs {

// what the entries check before a launch: the arm count keeps every index inside the spec's arrays
const char *bandit_spec_error(const gs_bandit_spec &sp)
{
    if (sp.n_arms < 2 || sp.n_arms > GS_BANDIT_MAX_ARMS) return "n_arms must be in [2, 32]";
    if (sp.episode_length < 1) return "episode_length must be >= 1";
    for (int a = 0; a < sp.n_arms; ++a) {
        if (!(fabsf(sp.means[a]) <= 3.4028234e38f)) return "means must be finite";
        if (!(sp.stds[a] >= 0.0f && sp.stds[a] <= 3.4028234e38f)) return "stds must be finite and >= 0";
    }
    return nullptr;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_bandit_reset(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec, int64_t N,
                               void *stream)
{
    GS_REQUIRE(N > 0 && meta_dev && ep_ret_dev && obs_dev, "gs_bandit_reset: bad argument");
    const char *bad = bandit_spec_error(spec);
    GS_REQUIRE(!bad, "gs_bandit_reset: %s", bad);
    const BanditEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, 0, 0}, spec};
    return launch_env_reset<BanditEnv>(ev, N, stream);
}

extern "C" int gs_bandit_step(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec,
                              const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                              int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                              uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                              float *ep_len_sum_dev, void *stream)
{
    GS_REQUIRE(N > 0 && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_bandit_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_bandit_step: null output row");
    const char *bad = bandit_spec_error(spec);
    GS_REQUIRE(!bad, "gs_bandit_step: %s", bad);
    const BanditEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                              max_steps, seed, env_offset},
                             spec};
    return launch_env_step<BanditEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev, stream);
}
