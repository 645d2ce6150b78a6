// gs_mountaincar.hip — device-resident MountainCar-v0 dynamics with the reference's reward
// shaper and state-count bonus wrappers.
//
// The reference ships three PPO configs for MountainCar-v0 and every one carries env_wrappers
// (gym_wrappers/MountainCarV0/reward_shaper.py, state_count_bonus.py), so the wrappers run here
// too, on the env's own thread right after the dynamics.  The env type is in
// gs_mountaincar_env.h (shared with the one-launch rollout), the kernels in gs_env_kernels.h.
// The dynamics restate gymnasium 1.x's MountainCarEnv (not vendored: parity with its trajectories
// is UNPINNED, as for CartPole and Acrobot); the wrappers' arithmetic is pinned to the
// reference's own classes by tests/golden/mountaincar_wrappers.npz.  The count tables are int32
// [N][position_bins * velocity_bins] in HBM; only env e's thread touches env e's table, so there
// are no atomics.  The numpy twin is tests/mountaincar_twin.py.
#include "gs_env_kernels.h"
#include "gs_mountaincar_env.h"

namespace gs {

// what the entries check before a launch: the order names each wrapper at most once with no gap,
// and a count bonus comes with its table and parameters that keep every index inside it
const char *mountaincar_wrappers_error(const gs_mountaincar_wrappers &w, const void *counts)
{
    bool bonus = false;
    for (int i = 0; i < 2; ++i) {
        const int o = w.order[i];
        if (o != GS_MC_WRAP_NONE && o != GS_MC_WRAP_SHAPER && o != GS_MC_WRAP_BONUS) return "unknown wrapper id";
        bonus = bonus || o == GS_MC_WRAP_BONUS;
    }
    if (w.order[0] == GS_MC_WRAP_NONE && w.order[1] != GS_MC_WRAP_NONE) return "a wrapper after an empty slot";
    if (w.order[0] != GS_MC_WRAP_NONE && w.order[0] == w.order[1]) return "a wrapper listed twice";
    if (bonus) {
        if (!counts) return "the count bonus needs its table";
        if (w.position_bins <= 0 || w.velocity_bins <= 0 ||
            (int64_t)w.position_bins * w.velocity_bins > kMcMaxCells)
            return "bins must be positive with position_bins * velocity_bins <= 16384";
        if (w.bonus_type != GS_MC_BONUS_COUNT && w.bonus_type != GS_MC_BONUS_INVERSE &&
            w.bonus_type != GS_MC_BONUS_LOG)
            return "unknown bonus_type";
        if (w.min_count < 1) return "min_count must be >= 1";
    }
    return nullptr;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_mountaincar_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                                    int32_t *counts_dev, gs_mountaincar_wrappers wrappers, int64_t N, uint64_t seed,
                                    int64_t env_offset, void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev, "gs_mountaincar_reset: bad argument");
    const char *bad = mountaincar_wrappers_error(wrappers, counts_dev);
    GS_REQUIRE(!bad, "gs_mountaincar_reset: %s", bad);
    if (counts_dev && wrappers.position_bins > 0 && wrappers.velocity_bins > 0)
        GS_HIP(hipMemsetAsync(counts_dev, 0,
                              (size_t)N * wrappers.position_bins * wrappers.velocity_bins * sizeof(int32_t),
                              (hipStream_t)stream));
    const MountainCarEnv::Args ev{
        {{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, seed, env_offset}, state_dev},
        counts_dev,
        wrappers};
    return launch_env_reset<MountainCarEnv>(ev, N, stream);
}

extern "C" int gs_mountaincar_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                                   int32_t *counts_dev, gs_mountaincar_wrappers wrappers, const int64_t *actions_dev,
                                   int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                                   float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                                   int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                                   void *stream)
{
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_mountaincar_step: bad argument");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_mountaincar_step: null output row");
    const char *bad = mountaincar_wrappers_error(wrappers, counts_dev);
    GS_REQUIRE(!bad, "gs_mountaincar_step: %s", bad);
    const MountainCarEnv::Args ev{{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                                    max_steps, seed, env_offset},
                                   state_dev},
                                  counts_dev,
                                  wrappers};
    return launch_env_step<MountainCarEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev,
                                           stream);
}
