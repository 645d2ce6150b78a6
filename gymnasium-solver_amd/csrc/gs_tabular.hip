// gs_tabular.hip — a generic tabular device env: any finite MDP whose outcomes per (state, action)
// are K equiprobable alternatives, given as three read-only tables in HBM (next state, reward,
// terminated; [S][A][K]).  Carries gymnasium 1.x FrozenLake-v1 (K = 3 slippery, K = 1 not) and
// Taxi-v3 (K = 1), whose tables gsamd/toytext.py restates; gymnasium is absent offline, so parity
// with its own episodes is UNPINNED (its PCG64 stream is not reproduced: the outcome and reset draws
// come from the counter hash every device env uses).  TimeLimit truncation, NEXT_STEP autoreset,
// the rollout rows and the episode counters are every device env's (gs_env_episode.h).  The env
// type is in gs_tabular_env.h, the kernels in gs_env_kernels.h.  The numpy twin is
// tests/tabular_twin.py.
#include "gs_env_kernels.h"
#include "gs_rollout1.h"
#include "gs_tabular_env.h"

namespace {

using namespace gs;

int check_spec(const gs_tabular_spec &sp, const char *who)
{
    GS_REQUIRE(sp.n_states > 0 && sp.n_actions > 0 && sp.n_outcomes > 0 && sp.n_starts > 0,
               "%s: n_states / n_actions / n_outcomes / n_starts must be positive", who);
    GS_REQUIRE((int64_t)sp.n_states * sp.n_actions * sp.n_outcomes < (int64_t)1 << 31, "%s: tables too large", who);
    int want = 1;
    if (sp.encoding == GS_ENC_BINARY) {
        while (want < 31 && (1 << want) < sp.n_states) ++want;      // max(1, ceil(log2 n_states))
    } else if (sp.encoding == GS_ENC_ONEHOT) {
        want = sp.n_states;
    } else {
        GS_REQUIRE(sp.encoding == GS_ENC_ARRAY, "%s: encoding %d is not GS_ENC_ARRAY / _BINARY / _ONEHOT", who,
                   sp.encoding);
    }
    GS_REQUIRE(want <= kMaxObsDim, "%s: the encoding's %d observation values exceed the policy's limit of %d", who,
               want, kMaxObsDim);
    GS_REQUIRE(sp.obs_dim == want, "%s: obs_dim %d, the encoding of %d states gives %d", who, sp.obs_dim, sp.n_states,
               want);
    return GS_OK;
}

}  // namespace

extern "C" int gs_tabular_reset(int32_t *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                                gs_tabular_spec spec, const int32_t *starts_dev, int64_t N, uint64_t seed,
                                int64_t env_offset, void *stream)
{
    int rc = check_spec(spec, "gs_tabular_reset");
    if (rc) return rc;
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && starts_dev, "gs_tabular_reset: bad argument");
    const TabularEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, nullptr, nullptr, nullptr, 0, seed, env_offset},
                              state_dev, spec, nullptr, nullptr, nullptr, starts_dev};
    return launch_env_reset<TabularEnv>(ev, N, stream);
}

extern "C" int gs_tabular_step(int32_t *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                               gs_tabular_spec spec, const int32_t *next_dev, const float *reward_dev,
                               const uint8_t *term_dev, const int32_t *starts_dev, const int64_t *actions_dev, int64_t N,
                               int32_t max_steps, uint64_t seed, int64_t env_offset, float *rewards_row_dev,
                               uint8_t *dones_row_dev, uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev,
                               float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream)
{
    int rc = check_spec(spec, "gs_tabular_step");
    if (rc) return rc;
    GS_REQUIRE(N > 0 && state_dev && meta_dev && ep_ret_dev && obs_dev && actions_dev && max_steps > 0,
               "gs_tabular_step: bad argument");
    GS_REQUIRE(next_dev && reward_dev && term_dev && starts_dev, "gs_tabular_step: null table");
    GS_REQUIRE(rewards_row_dev && dones_row_dev && timeouts_row_dev, "gs_tabular_step: null output row");
    const TabularEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                               max_steps, seed, env_offset},
                              state_dev, spec, next_dev, reward_dev, term_dev, starts_dev};
    return launch_env_step<TabularEnv>(ev, actions_dev, N, rewards_row_dev, dones_row_dev, timeouts_row_dev, stream);
}

// The whole rollout of a one-hidden-layer policy on the tabular env in one launch (gs_mlp1.hip
// k_rollout1<AMAX, TabularEnv>): gs_tabular_step's spec / table checks, then gs_rollout1.h's.
extern "C" int gs_rollout1_tabular(const float *params, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                                   uint64_t rng_seed, uint64_t rng_counter0, int32_t *state_dev, int32_t *meta_dev,
                                   float *ep_ret_dev, float *obs_dev, gs_tabular_spec spec, const int32_t *next_dev,
                                   const float *reward_dev, const uint8_t *term_dev, const int32_t *starts_dev,
                                   int32_t max_steps, uint64_t seed, int64_t env_offset, int32_t *ep_done_count_dev,
                                   float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows, int64_t *action_rows,
                                   float *logp_rows, float *value_rows, float *reward_rows, uint8_t *done_rows,
                                   uint8_t *timeout_rows, void *stream)
{
    int rc = check_spec(spec, "gs_rollout1_tabular");
    if (rc) return rc;
    const TabularEnv::Args ev{{meta_dev, ep_ret_dev, obs_dev, ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev,
                               max_steps, seed, env_offset},
                              state_dev, spec, next_dev, reward_dev, term_dev, starts_dev};
    const RolloutRows rw{obs_rows, action_rows, logp_rows, value_rows, reward_rows, done_rows, timeout_rows};
    const char *bad = !state_dev ? "null buffer" : (next_dev && reward_dev && term_dev && starts_dev ? nullptr : "null table");
    return rollout1_entry<TabularEnv>("gs_rollout1_tabular", params, dims, N, T, mode, rng_seed, rng_counter0, ev, rw,
                                      spec.obs_dim, spec.n_actions, bad, stream);
}
