// gs_tabular.hip — a generic tabular device env: any finite MDP whose outcomes per (state, action)
// are K equiprobable alternatives, given as three read-only tables in HBM (next state, reward,
// terminated; [S][A][K]).  Carries gymnasium 1.x FrozenLake-v1 (K = 3 slippery, K = 1 not) and
// Taxi-v3 (K = 1), whose tables gsamd/toytext.py restates; gymnasium is absent offline, so parity
// with its own episodes is UNPINNED (its PCG64 stream is not reproduced: the outcome and reset draws
// come from the counter hash every device env uses).  TimeLimit truncation, NEXT_STEP autoreset,
// the rollout rows and the episode counters are gs_cartpole_step's.  The observation is the
// reference's gym_wrappers/discrete_encoder.py applied on the env's own thread, as float32.
// The numpy twin is tests/tabular_twin.py.
#include "gs_common.h"
#include "gs_cartpole_env.h"   // env_mix64, env_reset_unit

namespace {

using namespace gs;

constexpr uint64_t kOutcomeStream = 0x7AB1E;    // distinct from the reset draws' 0xC0 + c

// uniform in [0, 1) of (seed, global env, episode, step in episode): the outcome draw
__device__ __forceinline__ double tabular_outcome_unit(uint64_t seed, uint64_t ge, uint64_t episode, uint64_t step)
{
    const uint64_t h = env_mix64(
        env_mix64(env_mix64(env_mix64(env_mix64(seed) ^ ge) ^ episode) ^ step) ^ kOutcomeStream);
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int tabular_reset_state(const gs_tabular_spec &sp, const int32_t *__restrict__ starts,
                                                   uint64_t seed, uint64_t ge, uint64_t episode)
{
    const double u = env_reset_unit(seed, ge, episode, 0);
    const int j = min(sp.n_starts - 1, (int)(u * (double)sp.n_starts));
    return clampi(starts[j], 0, sp.n_states - 1);
}

// gym_wrappers/discrete_encoder.py observation(), as float32
__device__ __forceinline__ void tabular_write_obs(const gs_tabular_spec &sp, int s, float *__restrict__ o)
{
    if (sp.encoding == GS_ENC_ARRAY) {
        o[0] = (float)s;
    } else if (sp.encoding == GS_ENC_BINARY) {
        for (int i = 0; i < sp.obs_dim; ++i) o[i] = (float)((s >> i) & 1);      // LSB first
    } else {
        for (int i = 0; i < sp.obs_dim; ++i) o[i] = i == s ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_tabular_reset(int32_t *__restrict__ state, int32_t *__restrict__ meta,
                                                       float *__restrict__ ep_ret, float *__restrict__ obs,
                                                       gs_tabular_spec sp, const int32_t *__restrict__ starts,
                                                       int64_t N, uint64_t seed, int64_t env_offset)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const int s = tabular_reset_state(sp, starts, seed, (uint64_t)(env_offset + e), 0);
    state[e] = s;
    meta[3 * e + 0] = 0;   // steps in the current episode
    meta[3 * e + 1] = 0;   // episodes finished (the reset counter)
    meta[3 * e + 2] = 0;   // 1 = the previous step ended an episode (autoreset pending)
    ep_ret[e] = 0.0f;
    tabular_write_obs(sp, s, obs + e * sp.obs_dim);
}

__global__ __launch_bounds__(256) void k_tabular_step(
    int32_t *__restrict__ state, int32_t *__restrict__ meta, float *__restrict__ ep_ret, float *__restrict__ obs,
    gs_tabular_spec sp, const int32_t *__restrict__ next_tab, const float *__restrict__ reward_tab,
    const uint8_t *__restrict__ term_tab, const int32_t *__restrict__ starts, const int64_t *__restrict__ actions,
    int64_t N, int max_steps, uint64_t seed, int64_t env_offset, float *__restrict__ rew_row,
    uint8_t *__restrict__ done_row, uint8_t *__restrict__ to_row, int32_t *__restrict__ ep_cnt,
    float *__restrict__ ep_ret_sum, float *__restrict__ ep_len_sum)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const uint64_t ge = (uint64_t)(env_offset + e);
    int s = clampi(state[e], 0, sp.n_states - 1);
    int steps = meta[3 * e + 0], episodes = meta[3 * e + 1], pending = meta[3 * e + 2];
    float er = ep_ret[e];
    float reward = 0.0f;
    bool done = false, timeout = false;
    if (pending != 0) {        // NEXT_STEP autoreset: this step only resets
        s = tabular_reset_state(sp, starts, seed, ge, (uint64_t)episodes);
        steps = 0;
        pending = 0;
        er = 0.0f;
    } else {
        // every table index is range-checked: a bad action or table entry cannot leave the tables
        const int64_t ar = actions[e];
        const int a = ar < 0 ? 0 : (ar >= sp.n_actions ? sp.n_actions - 1 : (int)ar);
        const double u = tabular_outcome_unit(seed, ge, (uint64_t)episodes, (uint64_t)steps);
        const int k = min(sp.n_outcomes - 1, (int)(u * (double)sp.n_outcomes));
        const int64_t at = ((int64_t)s * sp.n_actions + a) * sp.n_outcomes + k;
        const int ns = next_tab[at];
        const bool bad = ns < 0 || ns >= sp.n_states;      // forced terminal
        const bool terminated = term_tab[at] != 0 || bad;
        reward = reward_tab[at];
        s = bad ? s : ns;
        steps += 1;
        const bool truncated = !terminated && steps >= max_steps;
        er = er + reward;
        done = terminated || truncated;
        timeout = truncated;
        if (done) {
            if (ep_cnt) ep_cnt[e] += 1;
            if (ep_ret_sum) ep_ret_sum[e] += er;
            if (ep_len_sum) ep_len_sum[e] += (float)steps;
            episodes += 1;
            pending = 1;
        }
    }
    rew_row[e] = reward;
    done_row[e] = done ? 1 : 0;
    to_row[e] = timeout ? 1 : 0;
    state[e] = s;
    meta[3 * e + 0] = steps;
    meta[3 * e + 1] = episodes;
    meta[3 * e + 2] = pending;
    ep_ret[e] = er;
    tabular_write_obs(sp, s, obs + e * sp.obs_dim);
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

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
    hipLaunchKernelGGL(k_tabular_reset, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev, meta_dev,
                       ep_ret_dev, obs_dev, spec, starts_dev, N, seed, env_offset);
    GS_LAUNCH_CHECK("k_tabular_reset");
    return GS_OK;
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
    hipLaunchKernelGGL(k_tabular_step, dim3(nblk(N)), dim3(256), 0, (hipStream_t)stream, state_dev, meta_dev,
                       ep_ret_dev, obs_dev, spec, next_dev, reward_dev, term_dev, starts_dev, actions_dev, N,
                       (int)max_steps, seed, env_offset, rewards_row_dev, dones_row_dev, timeouts_row_dev,
                       ep_done_count_dev, ep_ret_sum_dev, ep_len_sum_dev);
    GS_LAUNCH_CHECK("k_tabular_step");
    return GS_OK;
}
