/*
 * gsamd.h — C-ABI of the MI355X-native rollout + GAE + PPO-update path
 * (libgsamd.so, built from gymnasium-solver_amd/csrc/ for gfx950).
 *
 * Conventions (SURVEY.md §8b "What the C-ABI must export"):
 *   - every pointer argument named *_dev is a caller-owned device (HBM) pointer;
 *     *_host pointers are caller-owned host memory;
 *   - kernels are enqueued on the caller's `stream` (a hipStream_t passed as void*;
 *     NULL = legacy default stream) and return without synchronising;
 *   - no hidden device allocation: scratch comes from a caller buffer sized by
 *     gs_ppo_workspace_bytes();
 *   - every function returns GS_OK (0) or a negative GS_E* code; the message of the
 *     last failure on the calling thread is returned by gs_last_error().
 *
 * Data layout in HBM:
 *   rollout buffers are time-major SoA: x[t * n_envs + env]; observations
 *   obs[(t * n_envs + env) * obs_dim + d]; the reference's env-major sample index
 *   i = env * T + t (utils/rollout_buffer.py:11-13) is mapped inside the kernels.
 *   Policy parameters are ONE flat fp32 vector in the reference's state_dict order
 *   (backbone.0.weight[H1][D], backbone.0.bias, backbone.2.weight[H2][H1],
 *   backbone.2.bias, policy_head.weight[A][H2], policy_head.bias,
 *   value_head.weight[1][H2], value_head.bias) — utils/models.py:285-326.
 *   Gradients and Adam moments use the same layout.
 */
#ifndef GSAMD_H
#define GSAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK 0
#define GS_E_INVALID (-1)   /* bad argument / unsupported shape: like the reference's ValueError */
#define GS_E_HIP (-2)       /* HIP runtime error */
#define GS_E_COMM (-3)      /* RCCL error */

/* ---------------------------------------------------------------- misc
 * gs_abi_version() returns GS_ABI_VERSION of the header the library was built with; a binding
 * must refuse a library whose version differs (argument lists change between versions:
 * version 2 added the rollout clock argument of gs_policy_act / gs_cnn_policy_act /
 * gs_env_step / gs_atari_env_step and gs_comm_error_record; version 3 widened the metric record
 * to 24 floats and added gs_ppo_update_global; version 4 added gs_comm_xgmi_set_bwd_exchange, gs_comm_allreduce_sum_f64,
 * gs_ppo_global_adv_stats, gs_ppo_global_records, gs_cnn_ppo_update_global, gs_fc_gemm and
 * gs_episode_window; version 5 added the obs_store argument of gs_cnn_policy_act; version 6 added
 * gs_normalize_advantages(_scratch_bytes), gs_cnn_activation_stats, gs_build_source_hash,
 * gs_comm_xgmi_reset, gs_cnn_workspace_hidden_offset / _act_offset and the parts argument of
 * gs_fc_gemm; version 7 widened the metric record to 40 floats (the GS_M_ACT activation-statistics
 * slots of GS_HP_ACT_STATS updates). */
#define GS_ABI_VERSION 7
int gs_abi_version(void);
const char *gs_last_error(void);
/* sha256 prefix (16 hex digits) of the kernel sources this library was compiled from: path "mlp"
 * (the MLP chain + GAE), "cnn" (the NatureCNN update) or "" (every csrc/ file) — the key under
 * which measured PMC traffic (profiles/) is attributed to a build; NULL for an unknown path. */
const char *gs_build_source_hash(const char *path);

/* ---------------------------------------------------------------- GAE
 * Replaces utils/returns_advantages.py:115-155
 * (compute_batched_gae_advantages_and_returns), called from
 * utils/rollout_collector.py:372-384.  Bit-exact with the reference's float32 numpy
 * loop.  values/rewards/adv/ret are (T, N) f32, dones/timeouts (T, N) u8 (0/1),
 * bootstrap (T, N) f32 or NULL (= bootstrapped_next_values None), last_values (N).
 */
int gs_gae_f32(const float *values_dev, const float *rewards_dev, const uint8_t *dones_dev,
               const uint8_t *timeouts_dev, const float *bootstrap_dev, const float *last_values_dev,
               int64_t T, int64_t N, double gamma, double gae_lambda, float *adv_dev, float *ret_dev,
               void *stream);
/* Rollout-level advantage normalisation, in place over all n elements: replaces
 * utils/returns_advantages.py:61-64 (_normalize_advantages: (a - mean) / (std + eps), std biased),
 * applied by utils/rollout_collector.py:441-442 when normalize_advantages == "rollout".  Bit-exact
 * with numpy on the float32 array: the mean's and std's sums are numpy's float32 pairwise sums over
 * its 8192-element buffer chunks, the statistics and the elementwise pass float32.  scratch_dev:
 * gs_normalize_advantages_scratch_bytes(n) bytes; mean_std_out_dev (2 floats: the mean and std
 * applied) may be NULL.  1 <= n < 2^31. */
size_t gs_normalize_advantages_scratch_bytes(int64_t n);
int gs_normalize_advantages(float *adv_dev, int64_t n, float eps, float *scratch_dev, float *mean_std_out_dev,
                            void *stream);

/* ---------------------------------------------------------------- sampler (host)
 * Replaces utils/samplers.py:25-34 (MultiPassRandomSampler.set_epoch + __iter__):
 * seeds torch's CPU MT19937 with `seed` (= base_seed + epoch), draws
 * rand((num_passes, data_len)) and writes the unstable argsort of each row
 * (torch's introsort tie order) to out_host (num_passes * data_len int32).
 * Host-side by construction (a sequential generator + introsort); n_threads > 1
 * sorts passes in parallel.  The stream is then uploaded once per rollout.
 */
int gs_sampler_stream_i32(int64_t data_len, int64_t num_passes, uint64_t seed, int32_t *out_host,
                          int n_threads);

/* ---------------------------------------------------------------- MLP actor-critic
 * dims: obs_dim D, hidden H1, H2 (two ReLU layers, the reference's mlp_small/medium/
 * large presets; utils/model_registry.py:21-36), n_actions A.
 *
 * hidden2 == 0 means ONE hidden ReLU layer of hidden1 units (the reference's mlp_tiny preset).  The
 * flat parameter vector is then backbone.0.weight[H][D], backbone.0.bias[H], policy_head.weight[A][H],
 * policy_head.bias[A], value_head.weight[1][H], value_head.bias[1] — P = H D + H + A H + A + H + 1.
 * Served by gs_mlp_param_count, gs_policy_scratch_bytes / _act / _value, gs_ppo_workspace_bytes,
 * gs_ppo_update_workspace_bytes, gs_ppo_update, gs_ppo_minibatch_step, gs_ppo_loss and
 * gs_mlp_activation_stats, in fp32 on one GPU; GS_E_INVALID from gs_ppo_stage, gs_ppo_update_global,
 * gs_ppo_exchange_inside_bwd, gs_rollout_synth / _env / _mountaincar, with GS_HP_BF16 and with a
 * communicator; gs_rollout_synth_supported / gs_rollout_env_supported answer 0.  Its one-launch
 * rollouts on the device envs are entries of their own, gs_rollout1_* (below the tabular envs).
 * Its update (gs_ppo_update: every minibatch of the call in ONE launch of one 256-thread workgroup;
 * use_graph is accepted and ignored) keeps the parameters, both Adam moments and the gradient in
 * LDS, so the shape must satisfy, with P4 = P rounded up to 4 and A1 = A + 1:
 *   obs_dim in [1, 64], n_actions in [1, 32], hidden1 a positive multiple of 16, and
 *   10240 + 16 P4 + 4 (round4(32 D) + 64 H + round4(32 A1) + 160 + H) + 8192 <= 163840 bytes
 * (reduction scratch; four parameter-sized vectors; a 32-row tile of observations, hidden
 * activations and their gradients, head outputs and minibatch fields; the dead-neuron counts; the
 * minibatch's row numbers and advantages, up to 1024 rows).
 * 64-64-32 (6 305 parameters) needs 149 056 bytes.  Any other shape is GS_E_INVALID with the byte
 * counts in the message.
 */
typedef struct gs_mlp_dims {
    int32_t obs_dim;
    int32_t hidden1;
    int32_t hidden2;
    int32_t n_actions;
} gs_mlp_dims;

int64_t gs_mlp_param_count(gs_mlp_dims dims);

/* Rollout clock (clock_dev, optional, 2 x uint64 in HBM): {rng counter base, env step base}.
 * When non-NULL the kernels add clock_dev[0] to rng_counter and clock_dev[1] to step_count, so
 * a captured T-step rollout graph replays with the next rollout's counters written into the
 * clock (one 16-byte copy) instead of re-capturing; NULL = the counters as passed. */

/* Policy forward for a rollout step — replaces utils/policy_ops.py:14-34 (policy_act)
 * on MLPActorCritic.forward (utils/models.py:328-346) + Categorical sample / mode /
 * log_prob.  obs_dev (N, D) f32.  mode: 0 = sample (counter-based RNG, key
 * (rng_seed, rng_counter, env)), 1 = deterministic (argmax, first max wins),
 * 2 = replay: actions_dev is an INPUT (recorded actions).  Writes actions (int64),
 * logp, value (N) and, when obs_store_dev != NULL, copies obs into it (the rollout
 * buffer slot of this step).  scratch_dev: gs_policy_scratch_bytes(dims, N) bytes, 16-byte aligned.
 */
size_t gs_policy_scratch_bytes(gs_mlp_dims dims, int64_t N);
int gs_policy_act(const float *params_dev, gs_mlp_dims dims, const float *obs_dev, int64_t N, int mode,
                  uint64_t rng_seed, uint64_t rng_counter, int64_t *actions_dev, float *logp_dev,
                  float *value_dev, float *obs_store_dev, void *scratch_dev, const uint64_t *clock_dev,
                  void *stream);
/* gs_policy_act under an action mask: the policy the reference builds with
 * valid_actions = spec.action_space.valid (utils/models.py:285-346, MaskedCategorical,
 * utils/distributions.py:8-82).  valid_mask: bit a set = action a valid.  The softmax runs over the
 * valid actions only (logp = z[action] - logsumexp over them); mode 1 takes the first maximum among
 * them; mode 0 draws from them with gs_policy_act's uniform under the same key, the inverse CDF in
 * index order, the fallback the last valid action; mode 2 replays (a recorded action outside the
 * valid set is the caller's error: its logp is unspecified, nothing is read out of range).  The
 * envelope, the scratch and the graph capture are gs_policy_act's; valid_mask == 0 means no mask and
 * gives gs_policy_act's bytes; bits at or beyond n_actions are GS_E_INVALID.  The value needs no
 * mask: gs_policy_value serves a masked policy as it is. */
int gs_policy_act_masked(const float *params_dev, gs_mlp_dims dims, const float *obs_dev, int64_t N, int mode,
                         uint64_t rng_seed, uint64_t rng_counter, int64_t *actions_dev, float *logp_dev,
                         float *value_dev, float *obs_store_dev, void *scratch_dev, const uint64_t *clock_dev,
                         void *stream, uint32_t valid_mask);

/* A whole rollout of the synthetic env (gs_env_*) in ONE launch, for MLP policies whose weights
 * fit in LDS (gs_rollout_synth_supported; the C3 shapes do, C2's 256x256 W2 does not): per
 * workgroup 16 envs for all T vector steps, the policy act with gs_policy_act's arithmetic in its
 * order and the env step with gs_env_step's, so every row equals the step-wise rollout bit for
 * bit (actions of mode 2 are read from action_rows).  Rows are time-major (T, N); the env state,
 * running returns and observations are left after the last step, as T gs_env_step calls leave
 * them; the rng counter of step t is rng_counter0 + t, the env step count env_step0 + t + 1.
 * Replaces (with gs_env_step) the loop of utils/rollout_collector.py:459-567. */
int gs_rollout_synth_supported(gs_mlp_dims dims, int *supported_host);
int gs_rollout_synth(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                     uint64_t rng_counter0, int32_t *env_state_dev, float *env_ep_ret_dev, float *env_obs_dev,
                     int32_t episode_len, int32_t truncate_every, float reward, uint64_t env_seed, int64_t env_offset,
                     uint64_t env_step0, int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                     float *obs_rows_dev, int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev,
                     float *reward_rows_dev, uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);

/* The same one-launch rollout on a device env with real dynamics: kind GS_ENV_CARTPOLE
 * (gs_cartpole_*: obs dim 4, 2 actions) or GS_ENV_ACROBOT (gs_acrobot_*: obs dim 6, 3 actions).
 * gs_rollout_env_supported: *supported_host = 1 when dims are that env's and the policy fits in
 * LDS (kind GS_ENV_SYNTHETIC answers as gs_rollout_synth_supported, kind GS_ENV_MOUNTAINCAR for
 * gs_rollout_mountaincar: obs dim 2, 3 actions; gs_rollout_env itself refuses that kind).  gs_rollout_env: env_state_dev
 * / env_meta_dev / env_ep_ret_dev / env_obs_dev and the episode counters are the env's tensors as
 * its gs_*_step takes them; every row, the final env state / meta / observations and the episode
 * counters equal T calls of gs_policy_act + the env's gs_*_step bit for bit, in all three modes
 * and with a ragged last workgroup (N % 16 != 0).  The env's arithmetic is the step kernel's own
 * (csrc/gs_cartpole_env.h, csrc/gs_acrobot_env.h). */
#define GS_ENV_SYNTHETIC 0
#define GS_ENV_CARTPOLE 1
#define GS_ENV_ACROBOT 2
#define GS_ENV_MOUNTAINCAR 3   /* answered by gs_rollout_env_supported; its rollout entry is gs_rollout_mountaincar */
#define GS_ENV_BANDIT 4        /* answered by gs_rollout_env_supported; its rollout entry is gs_rollout_bandit */
int gs_rollout_env_supported(gs_mlp_dims dims, int kind, int *supported_host);
int gs_rollout_env(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                   uint64_t rng_counter0, int kind, double *env_state_dev, int32_t *env_meta_dev,
                   float *env_ep_ret_dev, float *env_obs_dev, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                   int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows_dev,
                   int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev, float *reward_rows_dev,
                   uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);

/* Value-only forward (utils/policy_ops.py:37-42 policy_predict_values), e.g. the
 * bootstrap value of the last observation (utils/rollout_collector.py:373). */
int gs_policy_value(const float *params_dev, gs_mlp_dims dims, const float *obs_dev, int64_t N,
                    float *value_dev, void *scratch_dev, void *stream);

/* ---------------------------------------------------------------- synthetic env
 * Device twin of gsamd/synthetic_env.py.  state_dev: 4 int32 per env
 * (k, episode_idx, ep_len, pad) + ep_ret f32 (N); writes next obs into obs_dev (N, D),
 * reward/done/timeout rows of step t into the (T, N) rollout buffers, and per-env
 * completed-episode stats (ep_done_count, ep_ret_sum, ep_len_sum: N each, accumulated).
 */
int gs_env_reset(int32_t *state_dev, float *ep_ret_dev, float *obs_dev, int64_t N, int32_t obs_dim,
                 int32_t episode_len, uint64_t seed, int64_t env_offset, void *stream);
int gs_env_step(int32_t *state_dev, float *ep_ret_dev, float *obs_dev, int64_t N, int32_t obs_dim,
                int32_t episode_len, int32_t truncate_every, float reward, uint64_t seed,
                int64_t env_offset, uint64_t step_count, float *rewards_row_dev, uint8_t *dones_row_dev,
                uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                float *ep_len_sum_dev, const uint64_t *clock_dev, void *stream);

/* Completed-episode records of a (T, N) rollout, for the collector's episode statistics
 * (utils/rollout_collector.py:210-294 _process_done_infos, :686-760 get_metrics): per env the
 * running return (f32, the rewards summed in step order) and length carry across rollouts in
 * run_ret_dev / run_len_dev (N each, zero after a reset); ep_ret_dev / ep_len_dev (T, N) receive
 * the finished episode's return and length where dones_dev is set, 0 elsewhere. */
int gs_episode_stats(const float *rewards_dev, const uint8_t *dones_dev, int64_t T, int64_t N, float *run_ret_dev,
                     int32_t *run_len_dev, float *ep_ret_dev, int32_t *ep_len_dev, void *stream);
/* The reference's rolling window of the last W finished episodes (rollout_collector.py:242-294,
 * 753-758; track_stats=False keeps it on the device): this rollout's episodes in (step, env) order
 * — dones (T, N) time-major and gs_episode_stats' ep_ret / ep_len rows — appended behind the
 * previous window (2 x W doubles: returns, then lengths; the oldest first), meta[0] += their count,
 * meta[1] = max(meta[1], their best return), *total_out = their count (may be NULL).  One launch,
 * no host round trip. */
int gs_episode_window(const uint8_t *dones_dev, const float *ep_ret_dev, const int32_t *ep_len_dev, int64_t T,
                      int64_t N, int64_t W, double *window_dev, double *meta_dev, int64_t *total_out_dev,
                      void *stream);

/* ---------------------------------------------------------------- PPO update
 * Replaces the minibatch loop: DataLoader(MultiPassRandomSampler) + collate
 * (utils/dataloaders.py:20-77, rollout_collector.py:657-682) + PPOAgent.losses_for_batch
 * (agents/ppo/ppo_agent.py:21-152) + BaseAgent._backpropagate_and_step
 * (agents/base_agent.py:591-621: backward, clip_grad_norm_, Adam.step).
 */
typedef struct gs_ppo_hparams {
    float clip_range;
    float clip_range_vf;
    float vf_coef;
    float ent_coef;
    float max_grad_norm;      /* <= 0: no clipping */
    float lr;
    float adam_beta1;
    float adam_beta2;
    float adam_eps;
    float target_kl;          /* <= 0: None */
    int32_t normalize_adv;    /* 1 = "batch" (utils/torch.py:97-99), 0 = off */
    int32_t flags;            /* GS_HP_* bits; 0 = the fp32 parity path */
} gs_ppo_hparams;
/* bf16 MFMA operands (fp32 accumulation, fp32 parameters / Adam / loss) — a performance mode
 * beside the fp32 one (SURVEY.md Appendix A "Precision modes"): the NatureCNN update's
 * convolutions and GEMMs, and the MLP update's fused chain (gs_ppo_update: the h2 product, the
 * dW2 / dh1 products and the head-weight gradient; compile-time shapes only, GS_E_INVALID
 * elsewhere).  The single-step MLP entries (gs_ppo_minibatch_step, gs_ppo_loss, gs_ppo_stage)
 * stay fp32. */
#define GS_HP_BF16 1
/* Activation statistics per minibatch (the reference's forward hooks, utils/models.py:121-147,
 * recorded by every BaseAgent.training_step, agents/base_agent.py:335-347): the update also writes,
 * into the record of every minibatch whose loss it evaluates, {mean, unbiased std, dead_pct,
 * dead_max} of each hooked layer's pre-activation output z over the minibatch's rows, under the
 * parameters that minibatch's loss used (dead: |z| < 1e-6; dead_pct / dead_max the mean / max over
 * neurons of the fraction of rows) — GS_M_ACT + 4 l + {0, 1, 2, 3} for layer l (MLP: backbone.0,
 * backbone.2; NatureCNN: cnn.0, cnn.2, cnn.4, mlp.0).  gs_ppo_update / gs_ppo_minibatch_step /
 * gs_cnn_ppo_update; not the global-minibatch entries.  Off: those slots stay 0. */
#define GS_HP_ACT_STATS 2
/* The optimizer of the update entries (utils/optimizer_factory.py:6-29: torch's classes at their
 * defaults but lr).  Neither bit: torch.optim.Adam.  GS_HP_OPT_ADAMW: torch.optim.AdamW — per
 * parameter p = p * f32(1 - (double)lr * GS_ADAMW_WEIGHT_DECAY), then Adam's step (decoupled decay: a
 * parameter whose gradient is exactly zero is still decayed, its moments stay 0).  GS_HP_OPT_SGD:
 * torch.optim.SGD (no momentum, no decay) — p = p + f32(-lr) * g; adam_m / adam_v are neither read nor
 * written (the pointers are still required) and adam_step only counts the applied steps.  Both run
 * on the gradient after clip_grad_norm_.  Both bits set: GS_E_INVALID before any launch from every
 * entry that takes an optimizer step; the *_loss entries ignore the bits; gs_ppo_stage (the Adam
 * chain's stages) refuses them.  gs_ppo_update runs AdamW / SGD on the fused chain with the separate
 * clip + step launch (the lagged forward is Adam's). */
#define GS_HP_OPT_ADAMW 4
#define GS_HP_OPT_SGD 8
#define GS_ADAMW_WEIGHT_DECAY 0.01

/* Per-minibatch metric record written by the loss kernel (floats, GS_NUM_METRICS each).
 * KL early stop (agents/base_agent.py:330-366, sticky): the minibatch whose approx_kl exceeds
 * target_kl keeps its loss metrics with KL_STOP = SKIPPED = 1 (no optimizer step); every later
 * one is zeros with SKIPPED = KL_STOP = UNEVALUATED = 1 (its loss was never computed). */
#define GS_NUM_METRICS 40
enum gs_metric_slot {
    GS_M_LOSS = 0, GS_M_POLICY_LOSS, GS_M_VALUE_LOSS, GS_M_ENTROPY, GS_M_CLIP_FRAC,
    GS_M_CLIP_FRAC_VF, GS_M_EXPLAINED_VAR, GS_M_KL, GS_M_APPROX_KL, GS_M_ADV_NORM_MEAN,
    GS_M_ADV_NORM_STD, GS_M_KL_STOP, GS_M_GRAD_NORM, GS_M_SKIPPED, GS_M_UNEVALUATED, GS_M_RES1,
    /* pre-clip gradient norms per component (utils/models.py:196-230 compute_grad_norms, recorded
     * at agents/base_agent.py:607-608): MLP backbone | NatureCNN cnn trunk, policy_head,
     * value_head, and the NatureCNN mlp (fc) trunk (0 for the MLP policy) */
    GS_M_GN_BACKBONE, GS_M_GN_POLICY_HEAD, GS_M_GN_VALUE_HEAD, GS_M_GN_MLP,
    GS_M_RES20, GS_M_RES21, GS_M_RES22, GS_M_RES23,
    /* gs_pg_update / gs_pg_loss (REINFORCE): mean and unbiased std of the policy targets the loss
     * used (after the batch normalisation, when on) — the reserved slots 20 / 21 by another name */
    GS_M_PG_TARGET_MEAN = GS_M_RES20, GS_M_PG_TARGET_STD = GS_M_RES21,
    /* GS_HP_ACT_STATS: 4 layers x {mean, std, dead_pct, dead_max} of the pre-activation outputs */
    GS_M_ACT = 24
};

size_t gs_ppo_workspace_bytes(gs_mlp_dims dims, int64_t batch);

/* Rollout buffers the update reads (time-major (T, N), see header comment). */
typedef struct gs_rollout_view {
    const float *obs;        /* (T, N, D) */
    const int64_t *actions;  /* (T, N) */
    const float *logprobs;   /* (T, N) */
    const float *values;     /* (T, N) */
    const float *advantages; /* (T, N) */
    const float *returns;    /* (T, N) */
    int64_t T;
    int64_t N;
} gs_rollout_view;

/* One fused PPO minibatch step on rows idx_dev[0:batch) (env-major sample indices into
 * the rollout, int32): forward, loss, backward, grad-norm clip and Adam update of
 * params/adam_m/adam_v in place.  adam_step is the 1-based optimizer step count.
 * metrics_dev receives GS_NUM_METRICS floats; stop_flag_dev is the sticky KL early-stop
 * flag (int32, agents/base_agent.py:331-355).  comm may be NULL (single GPU) or a
 * gs_comm handle: gradients are then all-reduced (mean) across ranks before clipping. */
struct gs_comm;
int gs_ppo_minibatch_step(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                          gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout,
                          const int32_t *idx_dev, int64_t batch, int64_t adam_step,
                          float *metrics_dev, int32_t *stop_flag_dev, void *workspace_dev,
                          struct gs_comm *comm, void *stream);

/* Forward + loss only (PPOAgent.losses_for_batch without the optimizer step): writes the
 * GS_NUM_METRICS record (loss, policy/value/entropy terms, clip fractions, KL ...). */
int gs_ppo_loss(const float *params_dev, gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout,
                const int32_t *idx_dev, int64_t batch, float *metrics_dev, void *workspace_dev, void *stream);

/* Activation statistics of the MLP backbone (utils/models.py:120-145: hooks on backbone.0 and
 * backbone.2, i.e. the pre-activation outputs of the two Linear layers; recorded per
 * training_step, base_agent.py:336-347) over rows idx_dev[0..rows) of the rollout (idx_dev null:
 * rows 0..rows).  Writes ceil(rows/16) parts of 2 * (2 + max(hidden1, hidden2)) doubles: per layer
 * {sum z, sum z^2, then per neuron the count of |z| < 1e-6}; the caller adds the parts
 * (mean, unbiased std, dead_pct = mean over neurons of count / rows, dead_max = max). */
int gs_mlp_activation_stats(const float *params_dev, gs_mlp_dims dims, gs_rollout_view rollout,
                            const int32_t *idx_dev, int64_t rows, double *parts_dev, void *stream);

/* Enqueue ONE stage of a minibatch step on the current workspace.  Unfused chain:
 * 0 = k_fwd_hidden, 1 = k_loss, 2 = k_bwd, 3 = k_clip_adam.  Fused chain (the one
 * gs_ppo_update runs for the compile-time shapes): 6 = k_gather_all for a one-minibatch
 * update (run once first), 4 = k_fwd_hidden<fused>, 5 = k_bwd<fused> (loss rows inside),
 * then 3; 7 = k_fwd_hidden<fused> carrying the previous minibatch's clip + Adam step (the
 * lagged chain gs_ppo_update runs on one GPU; writes the update workspace's second parameter set, so the
 * workspace must be gs_ppo_update_workspace_bytes(dims, batch, n >= 1) large).  Used by bench.py
 * to time each kernel with events on the stream it is launched on (roofline measurement). */
int gs_ppo_stage(int stage, float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                 gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev,
                 int64_t batch, int64_t adam_step, float *metrics_dev, void *workspace_dev, void *stream);

/* The whole update phase of one rollout: n_minibatches consecutive steps over
 * idx_dev (n_minibatches * batch indices), metrics_dev gets n_minibatches records.
 * adam_step0 is the optimizer step count BEFORE the first of these steps.
 * use_graph != 0 replays chunks of 512 steps from a captured hipGraph.  stop_flag_dev is the
 * KL early stop of hp.target_kl > 0 (sticky: set when a minibatch's approx_kl exceeds it, every
 * later step skipped); with target_kl unset the update never reads or writes it (the fused
 * chain's kernels then start without that dependent load). */
int gs_ppo_update(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                  gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev,
                  int64_t batch, int64_t n_minibatches, int64_t adam_step0, float *metrics_dev,
                  int32_t *stop_flag_dev, void *workspace_dev, size_t workspace_bytes, struct gs_comm *comm,
                  int use_graph, void *stream);

/* Global-minibatch mode of a data-parallel update (SURVEY.md §8e "exact global" option): the
 * reference's single-GPU math on G ranks.  Every rank runs the SAME n_minibatches global
 * minibatches of batch_global rows, drawn from the reference's permutation of ALL ranks' samples
 * (utils/samplers.py:25-34 over the global env-major index); idx_dev holds, per minibatch, this
 * rank's rows (local env-major indices) padded to `batch` entries with -1 (another rank's row: no
 * loss, no gradient).  The loss and its gradient are means over batch_global rows, so each rank's
 * gradient is its share of the global one and the exchange SUMS them (no 1/G); the advantage
 * normalisation uses the whole minibatch's statistics adv_stats (utils/torch.py:97-99, computed by
 * the caller from all ranks' rows); with target_kl the KL early stop is decided on approx_kl summed
 * over ranks (agents/ppo/ppo_agent.py:126-129), so every rank stops at the same minibatch.  This
 * rank's raw loss sums per minibatch (14 doubles: sum of min-surrogate, clipped value loss,
 * entropy, clip counts, kl, approx_kl, ret - v and its square, ret and its square, normalised adv
 * and its square, one unused slot) go to metric_sums; the caller adds them over ranks and forms the records
 * (gsamd.metrics.records_from_sums). */
typedef struct gs_ppo_global {
    int64_t batch_global;       /* rows of a global minibatch (all ranks) */
    const float *adv_stats;     /* (n_minibatches, 2) f32 {mean, std} of each global minibatch's advantages */
    double *metric_sums;        /* (n_minibatches, 14) out: this rank's raw loss sums */
} gs_ppo_global;
int gs_ppo_update_global(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                         gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev,
                         int64_t batch, int64_t n_minibatches, int64_t adam_step0, float *metrics_dev,
                         int32_t *stop_flag_dev, void *workspace_dev, size_t workspace_bytes, struct gs_comm *comm,
                         int use_graph, const gs_ppo_global *glob, void *stream);

/* Workspace for gs_ppo_update over n_minibatches steps.  When the shape has a compiled
 * fused chain (the BASELINE configs' MLP shapes) this includes the per-update gathered
 * minibatch fields and normalised advantages, so the per-step chain reads x in one load and
 * the loss runs row-parallel with metrics reduced once after the update; a smaller workspace
 * (>= gs_ppo_workspace_bytes) selects the index-chasing chain with bit-identical parameters.
 * The fused chain also needs params/grads/adam_m/adam_v 16-byte aligned (every torch
 * allocation is); unaligned buffers take the index-chasing chain.  The workspace also holds a
 * second params | adam_m | adam_v set for the lagged chain (single GPU: each minibatch's clip +
 * Adam runs inside the next forward kernel; bit-identical results; GS_LAGGED_ADAM=0 in the
 * environment selects a separate clip/Adam launch instead). */
size_t gs_ppo_update_workspace_bytes(gs_mlp_dims dims, int64_t batch, int64_t n_minibatches);

/* The update graphs gs_ppo_update keeps (one per distinct set of buffers and shapes) and the
 * number of captures made so far.  lr never causes a re-capture (the graph reads the step size
 * from a per-call table); a change of another hyper-parameter re-captures in place. */
int gs_ppo_graph_cache_info(int64_t *n_entries_host, int64_t *n_captures_host);
/* Where the fused MLP update (gs_ppo_update without target_kl) exchanges gradients over
 * `comm`: *inside_host = 1 when k_bwd exchanges its own outputs (xGMI transport, the shape
 * within the in-kernel exchange's limits and co-residency, include the one-rank case where the
 * exchange is empty), 0 when a separate exchange launch follows the backward (RCCL, or
 * GS_XGMI_BWD=0).  Host query (reads device attributes, launches nothing). */
int gs_ppo_exchange_inside_bwd(struct gs_comm *comm, gs_mlp_dims dims, int64_t batch, int *inside_host);
/* Global-minibatch mode, the device half around gs_ppo_update_global (no host round trip):
 * gs_ppo_global_adv_stats: Sum adv and Sum adv^2 (double) of this rank's rows (idx >= 0) of every
 * global minibatch, summed over ranks through `comm` (gs_comm_allreduce_sum_f64; comm NULL: one
 * rank), then the whole minibatch's mean and unbiased std into adv_stats[k][2] (f32) for
 * gs_ppo_global.adv_stats — utils/torch.py:97-99 over all G ranks' rows.  sums: 2 x n doubles of
 * workspace (16-B aligned).  gs_ppo_global_records: after the update, the ranks' raw loss sums
 * (gs_ppo_global.metric_sums, 14 doubles per minibatch) summed over ranks in place and every
 * evaluated minibatch's record rewritten from them (loss, policy / value loss, entropy, clip
 * fractions, explained variance, kl, approx_kl, normalised-advantage mean / std) — identical on
 * every rank.  Both are stream-ordered and graph-capturable. */
int gs_ppo_global_adv_stats(const int32_t *idx_dev, int64_t n_minibatches, int64_t batch, int64_t batch_global,
                            const float *advantages_dev, int64_t T, int64_t N, struct gs_comm *comm, double *sums_dev,
                            float *adv_stats_dev, void *stream);
int gs_ppo_global_records(const gs_ppo_hparams *hp, int64_t n_minibatches, int64_t batch_global, struct gs_comm *comm,
                          double *metric_sums_dev, float *metrics_dev, void *stream);

/* ---------------------------------------------------------------- REINFORCE (Monte Carlo returns + policy-gradient update)
 * The reference's second algorithm (agents/reinforce/reinforce_agent.py:11-88 on the targets of
 * utils/rollout_collector.py:385-457).
 *
 * gs_mc_returns_f32 replaces compute_batched_mc_returns (utils/returns_advantages.py:67-91),
 * convert_returns_to_full_episode (:93-113, kind GS_MC_EPISODE) and _build_valid_mask_and_index_map
 * (:33-52) on time-major (T, N) rows.  timeouts_dev NULL: every done cuts the return (the
 * reference's mc_treat_timeouts_as_terminals=True default); non-NULL: a terminal is done && !timeout.
 * returns_dev (T, N): bit-exact with the reference's float32 loop acc = r + f32(gamma) * (acc * nt),
 * three roundings, no FMA.  last_terminal_dev (N): each env's last terminal step, -1 = none; an
 * env's positions 0 .. last terminal are valid.  idx_map_dev (N * T int32, env-major i = env * T + t;
 * may be NULL): every position's nearest earlier-or-equal valid position, positions before the first
 * valid one map to it; with nothing valid the identity (the reference keeps no map then).
 * valid_sums_dev (3 doubles): {count, sum, sum of squares} of the valid returns, summed in double
 * in a fixed order (per env in step order, then over envs).  Two launches, no host round trip.
 * T * N < 2^31. */
#define GS_MC_RTG 0
#define GS_MC_EPISODE 1
int gs_mc_returns_f32(const float *rewards_dev, const uint8_t *dones_dev, const uint8_t *timeouts_dev, int64_t T,
                      int64_t N, double gamma, int kind, float *returns_dev, int32_t *idx_map_dev,
                      int32_t *last_terminal_dev, double *valid_sums_dev, void *stream);

/* REINFORCEAgent.losses_for_batch + BaseAgent._backpropagate_and_step on minibatches of up to 2^20
 * rows (the reference's batch_size is 2048, beyond the PPO entries' 1024): per optimizer step one
 * row-parallel launch (forward, loss, backward; workgroups own 16-row tiles and add their gradient
 * share into their own partial slot) and one step launch (the slots summed in workgroup order, the
 * norms, clip_grad_norm_, Adam).
 *   loss = -mean(logp * t) - ent_coef * mean(entropy),  t = rollout.advantages[row], normalised over
 *   the minibatch as (t - mean) / (std_unbiased + 1e-8) when normalize_targets != 0.
 * rollout.advantages carries the policy targets (returns or advantages, as the caller chose);
 * rollout.values / .returns are not read and may be NULL.  The value head is outside the loss: its
 * gradient is None in the reference, so clip_grad_norm_ and Adam skip it — its slice of params,
 * adam_m and adam_v is not written at all, its slice of grads is zeros.  Every reduction has a
 * fixed order (no float atomics): two runs give the same bytes.
 * Record per minibatch (GS_NUM_METRICS floats): LOSS, POLICY_LOSS, ENTROPY, KL, APPROX_KL,
 * ADV_NORM_MEAN / _STD (the normalised targets' mean / unbiased std when normalising, else 0),
 * GRAD_NORM, GN_BACKBONE, GN_POLICY_HEAD, GS_M_PG_TARGET_MEAN / _STD; every other slot 0.
 * Shapes: obs_dim in [1, 64], hidden1 / hidden2 in [1, 512], n_actions in [1, 32]; batch in
 * [2, 2^20]; idx_dev: n_minibatches * batch env-major sample indices.  GS_E_INVALID for hidden2 == 0
 * (one hidden layer), GS_HP_BF16 in flags and a non-NULL communicator.  workspace_dev: 16-byte
 * aligned, gs_pg_update_workspace_bytes(dims, batch) bytes — it grows with min(row tiles, 256), not
 * with batch (one parameter-sized slot per row workgroup: at 4096 rows or more 18 MB for 4-128-128-2,
 * 69 MB for 4-256-256-2).  gs_pg_loss: the same forward, loss and gradient (into grads_dev) and the record,
 * no optimizer step. */
typedef struct gs_pg_hparams {
    float ent_coef;
    float max_grad_norm;        /* <= 0: no clipping */
    float lr;
    float adam_beta1;
    float adam_beta2;
    float adam_eps;
    int32_t normalize_targets;  /* 1 = "batch" (utils/torch.py:97-99), 0 = off */
    int32_t flags;              /* GS_HP_BF16 is refused; GS_HP_OPT_* as above; other bits ignored */
} gs_pg_hparams;
size_t gs_pg_update_workspace_bytes(gs_mlp_dims dims, int64_t batch);
int gs_pg_update(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev, gs_mlp_dims dims,
                 gs_pg_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev, int64_t batch,
                 int64_t n_minibatches, int64_t adam_step0, float *metrics_dev, void *workspace_dev,
                 size_t workspace_bytes, struct gs_comm *comm, void *stream);
int gs_pg_loss(const float *params_dev, float *grads_dev, gs_mlp_dims dims, gs_pg_hparams hp, gs_rollout_view rollout,
               const int32_t *idx_dev, int64_t batch, float *metrics_dev, void *workspace_dev, size_t workspace_bytes,
               void *stream);

/* ---------------------------------------------------------------- PPO update, row-parallel (minibatches beyond 1024 rows)
 * gs_ppo_update's semantics (PPOAgent.losses_for_batch + BaseAgent._backpropagate_and_step over
 * n_minibatches * batch env-major indices, the same GS_NUM_METRICS record per minibatch, the same Adam
 * state) for the one- and two-hidden-layer actor-critics on minibatches of up to 2^20 rows, where
 * gs_ppo_update / gs_ppo_minibatch_step / gs_ppo_loss stop at 1024 (whole-minibatch tiles in LDS).  All
 * parameters train: the value head is inside the loss.  Per optimizer step: the advantage sums (with
 * normalize_adv), one row-parallel launch (workgroups own 16-row tiles and loop over them: forward, loss
 * row, backward, their gradient share into their own partial slot; the H1 x H2 products of a two-layer
 * net on v_mfma_f32_16x16x4_f32, exact f32), the slots summed in workgroup order, and the norms, clip,
 * Adam and the record.  Every reduction has a fixed order (no float atomics): two runs give the same
 * bytes, and one call of n minibatches equals n calls of one.
 *   gs_ppo_rows_update: grads_dev is left holding the last applied step's clipped gradient.
 *   gs_ppo_rows_loss:   forward, loss, record and the unclipped gradient (into grads_dev) of one
 *                       minibatch; no optimizer step, no stop flag.
 * Record: write_metrics' slots as gs_ppo_update, GS_M_GRAD_NORM and GS_M_GN_BACKBONE / _POLICY_HEAD /
 * _VALUE_HEAD (pre-clip; 0 in the record of the minibatch that trips the KL stop, whose gradient is
 * never summed), GS_M_GN_MLP 0.  hp.normalize_adv: (adv - mean) / (std_unbiased + 1e-8) over the
 * minibatch's rows, the statistics in double in a fixed order.  hp.target_kl > 0: the sticky early stop
 * described beside GS_NUM_METRICS; parameters, moments and gradient are then byte-identical to a run
 * of that many steps fewer without a target; with the target unset stop_flag_dev is neither read nor
 * written (and may be NULL).  GS_HP_ACT_STATS: GS_M_ACT + 4 l + {0..3} for l = 0 (backbone.0) and, with
 * two hidden layers, l = 1 (backbone.2), over the minibatch's rows only (a ragged tile's padding rows
 * count for nothing).
 * Envelope: obs_dim in [1, 64]; hidden1 a multiple of 16 in [16, 512]; hidden2 0 (one hidden layer) or
 * a multiple of 16 in [16, 512]; n_actions in [1, 32]; batch in [2, 2^20] (1024 and below included);
 * T * N < 2^31.  Indices outside the rollout and actions outside [0, n_actions) are clamped.
 * GS_E_INVALID before any launch, the reason in gs_last_error, for: a shape or batch outside the
 * envelope, a non-NULL communicator, GS_HP_BF16, a workspace smaller than
 * gs_ppo_rows_workspace_bytes(dims, batch) or not 16-byte aligned, parameters not 16-byte aligned, a
 * NULL buffer, target_kl without a stop flag, and a row kernel whose static + dynamic LDS would pass
 * 160 KB (none inside the envelope today: the widest net, 64-512-512-32, takes 155 392 bytes, all dynamic).
 * Workspace (gs_ppo_rows_workspace_bytes; 0 = shape or batch not served), 256-byte aligned pieces:
 * 64 x 2 doubles of advantage parts, 256 x 3 doubles of norm parts, then per row workgroup 14 doubles
 * of metric sums, 4 doubles of activation sums, hidden1 + hidden2 u32 dead counts and one
 * parameter-sized gradient slot (round4(P) floats).  Row workgroups = min(ceil(batch / 16), 256), so it
 * grows with the batch up to 4096 rows and not beyond (4-256-256-2: 70 MB; 12-128-128-18: 21 MB;
 * 64-512-512-32, the widest: 321 MB). */
size_t gs_ppo_rows_workspace_bytes(gs_mlp_dims dims, int64_t batch);
int gs_ppo_rows_update(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                       gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev,
                       int64_t batch, int64_t n_minibatches, int64_t adam_step0, float *metrics_dev,
                       int32_t *stop_flag_dev, void *workspace_dev, size_t workspace_bytes,
                       struct gs_comm *comm, void *stream);
int gs_ppo_rows_loss(const float *params_dev, float *grads_dev, gs_mlp_dims dims, gs_ppo_hparams hp,
                     gs_rollout_view rollout, const int32_t *idx_dev, int64_t batch, float *metrics_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream);
/* The two entries above under an action mask (valid_mask: bit a set = action a valid), for a policy
 * that acts through gs_policy_act_masked: the envelope, workspace, record, KL stop, GS_HP_ACT_STATS
 * and determinism contract are unchanged.  Per row the normalisation runs over the valid actions,
 * the entropy is MaskedCategorical's -sum_valid p logf(p + 1e-8f), and dLoss/dlogit of an invalid
 * action is an exact 0: the invalid rows of policy_head.weight / .bias get a zero gradient, their
 * Adam moments stay 0 and their parameters keep their bytes.  The row kernel forms every head column
 * and zeroes the invalid ones' gradient (no column compaction).  valid_mask == 0 means no mask and
 * gives the unmasked entries' bytes; bits at or beyond n_actions are GS_E_INVALID; a recorded action
 * outside the valid set is the caller's error (values unspecified, no out-of-range access). */
int gs_ppo_rows_update_masked(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                              gs_mlp_dims dims, gs_ppo_hparams hp, gs_rollout_view rollout, const int32_t *idx_dev,
                              int64_t batch, int64_t n_minibatches, int64_t adam_step0, float *metrics_dev,
                              int32_t *stop_flag_dev, void *workspace_dev, size_t workspace_bytes,
                              struct gs_comm *comm, void *stream, uint32_t valid_mask);
int gs_ppo_rows_loss_masked(const float *params_dev, float *grads_dev, gs_mlp_dims dims, gs_ppo_hparams hp,
                            gs_rollout_view rollout, const int32_t *idx_dev, int64_t batch, float *metrics_dev,
                            void *workspace_dev, size_t workspace_bytes, void *stream, uint32_t valid_mask);

/* ---------------------------------------------------------------- NatureCNN actor-critic (C4/C5)
 * Replaces CNNActorCritic (utils/models.py:347-455; conv 8x8s4 -> 4x4s2 -> 3x3s1 with 32/64/64
 * channels, ReLU, Linear F->hidden ReLU, policy/value heads), action masking
 * (utils/policy_ops.py:44-75 + MaskedCategorical utils/distributions.py:8-82) and the same PPO
 * minibatch step as gs_ppo_update for image observations.  Observations are the u8 frame
 * stacks (T, N, in_c, in_h, in_w) exactly as the reference stores them; the model divides by
 * 255.  Flat parameter layout: the reference's tensor order (cnn.0, cnn.2, cnn.4, mlp.0,
 * policy_head, value_head; weight then bias) with conv2/conv3 weights stored (out, ky, kx, in)
 * and the fc weight (hidden, y, x, c) — gsamd.cnn converts state_dicts both ways. */
typedef struct gs_cnn_dims {
    int32_t in_c, in_h, in_w;  /* frame stack (4, 84, 84) */
    int32_t n_actions;         /* full action space (18 for ALE) */
    int32_t hidden;            /* fc width (512) */
    uint32_t valid_mask;       /* bit a set = action a valid; 0 = unmasked Categorical */
} gs_cnn_dims;

typedef struct gs_rollout_view_u8 {
    const uint8_t *obs;      /* (T, N, in_c, in_h, in_w) */
    const int64_t *actions;  /* (T, N) */
    const float *logprobs;   /* (T, N) */
    const float *values;     /* (T, N) */
    const float *advantages; /* (T, N) */
    const float *returns;    /* (T, N) */
    int64_t T;
    int64_t N;
} gs_rollout_view_u8;

int64_t gs_cnn_param_count(gs_cnn_dims dims);
/* scratch for `rows` rows (the minibatch B for updates, N envs for gs_cnn_policy_act); the workspace
 * base must be 16-byte aligned (every torch allocation is): the update places its internal buffers,
 * the bf16 parameter copy included, relative to it and refuses (GS_E_INVALID) an unaligned base */
size_t gs_cnn_workspace_bytes(gs_cnn_dims dims, int64_t rows);
/* Byte offset, inside a workspace of that many rows, of the fc layer's output h [rows][HID] fp32
 * (after relu): after gs_cnn_ppo_update / _global it holds the last minibatch step's values (the
 * device's fc ReLU decisions, which a teacher-forced comparison takes over); -1 on a bad shape. */
int64_t gs_cnn_workspace_hidden_offset(gs_cnn_dims dims, int64_t rows);
/* The same for the convolution activations: layer 1, 2, 3 -> a1, a2, a3 (NHWC, fp32 in the fp32
 * update: the device's conv ReLU decisions of the last minibatch step), 4 -> the fc output as
 * above; -1 on a bad shape or layer. */
int64_t gs_cnn_workspace_act_offset(gs_cnn_dims dims, int64_t rows, int layer);
/* policy_act on N frame stacks obs_dev (N, in_c, in_h, in_w): mode 0 sample / 1 argmax /
 * 2 replay (as gs_policy_act); masked actions are never drawn.  obs_store_dev (may be NULL): the
 * rollout buffer's obs row, receives a copy of obs_dev (written by the first convolution from the
 * frames it loads, no separate copy launch). */
int gs_cnn_policy_act(const float *params_dev, gs_cnn_dims dims, const uint8_t *obs_dev, int64_t N, int mode,
                      uint64_t rng_seed, uint64_t rng_counter, int64_t *actions_dev, float *logp_dev,
                      float *value_dev, uint8_t *obs_store_dev, void *workspace_dev, const uint64_t *clock_dev,
                      void *stream);
/* losses_for_batch on one minibatch: metrics record + (optional) dLoss/dlogits (B, A+1). */
int gs_cnn_ppo_loss(const float *params_dev, gs_cnn_dims dims, gs_ppo_hparams hp, gs_rollout_view_u8 rollout,
                    const int32_t *idx_dev, int64_t batch, float *metrics_dev, float *dlogits_dev,
                    void *workspace_dev, void *stream);
/* Activation statistics of the NatureCNN on one minibatch (the reference's forward hooks,
 * utils/models.py:121-147, registered on cnn.0 / cnn.2 / cnn.4 / mlp.0 at :419-422 and recorded
 * per training step at agents/base_agent.py:335-347): stats_out_dev receives 16 doubles, per
 * layer in that order {mean, std (unbiased), dead_pct, dead_max} of the layer's pre-activation
 * output over the batch rows (dead: |z| < 1e-6, per-neuron fraction of rows; dead_pct its mean
 * over neurons, dead_max its max).  fp32 (the reference's precision) whatever the update's mode;
 * uses the update's workspace (gs_cnn_workspace_bytes(dims, batch)). */
int gs_cnn_activation_stats(const float *params_dev, gs_cnn_dims dims, gs_rollout_view_u8 rollout,
                            const int32_t *idx_dev, int64_t batch, double *stats_out_dev, void *workspace_dev,
                            void *stream);
/* n_minibatches fused steps (forward, loss, backward, optional all-reduce, clip, Adam).
 * params / grads / adam_m / adam_v: 16-byte aligned (the clip + Adam kernel moves float4s). */
int gs_cnn_ppo_update(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev, gs_cnn_dims dims,
                      gs_ppo_hparams hp, gs_rollout_view_u8 rollout, const int32_t *idx_dev, int64_t batch,
                      int64_t n_minibatches, int64_t adam_step0, float *metrics_dev, int32_t *stop_flag_dev,
                      void *workspace_dev, struct gs_comm *comm, void *stream);
/* Global-minibatch mode of the NatureCNN update (dp_mode "global", the MLP's gs_ppo_update_global
 * for NatureCNN): idx = this rank's rows of every global minibatch (-1 = another rank's row),
 * frame_idx = the same with -1 replaced by a valid sample (those rows are read but dead: zero
 * dLoss/dz, so every gradient gets exact zeros from them); advantage statistics from
 * glob->adv_stats (gs_ppo_global_adv_stats), the loss averaged over glob->batch_global rows, the
 * exchange summing the ranks' shares (no 1/world), and this rank's raw loss sums in
 * glob->metric_sums (14 per minibatch, slot 13 zero) for gs_ppo_global_records.  No KL early
 * stop (target_kl must be unset).  Replaces agents/base_agent.py:591-621 over the reference's
 * single-process minibatches (utils/samplers.py:25-34, utils/torch.py:97-99). */
int gs_cnn_ppo_update_global(float *params_dev, float *grads_dev, float *adam_m_dev, float *adam_v_dev,
                             gs_cnn_dims dims, gs_ppo_hparams hp, gs_rollout_view_u8 rollout, const int32_t *idx_dev,
                             const int32_t *frame_idx_dev, int64_t batch, int64_t n_minibatches, int64_t adam_step0,
                             float *metrics_dev, int32_t *stop_flag_dev, void *workspace_dev, struct gs_comm *comm,
                             const gs_ppo_global *glob, void *stream);

/* ---------------------------------------------------------------- CartPole-v1 dynamics (f1)
 * gymnasium 1.x CartPoleEnv.step restated on device (double-precision state, Euler, tau 0.02,
 * TimeLimit max_steps, NEXT_STEP autoreset), for training on real CartPole dynamics without a
 * host round trip.  state_dev: 4 doubles per env; meta_dev: 3 int32 per env; actions_dev: the
 * (N) int64 actions of this step (ignored on autoreset steps).  Rows/counters as gs_env_step.
 * Reset draws come from a counter hash (gymnasium's PCG64 stream is not reproduced). */
int gs_cartpole_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int64_t N,
                      uint64_t seed, int64_t env_offset, void *stream);
int gs_cartpole_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                     const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                     float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                     int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream);

/* CartPole-v1 under the reference's CartPoleV1_RewardShaper (gym_wrappers/CartPoleV1/
 * reward_shaper.py:23-77), the env of CartPole-v1:ppo_rewardshaped.  Dynamics, termination,
 * truncation, counters and reset hash are gs_cartpole_step's; only the reward and what the
 * episode-return accumulator adds change.  In double, on the float32 observation {x, theta}:
 *   pos = 1 - |x| / max(2.4, 1e-6), ang = 1 - |theta| / max(12 * 2 pi / 360, 1e-6), both clipped
 *   to [0, 1] with clip_potential; phi = angle_reward_scale * ang + position_reward_scale * pos;
 *   reward = (float)(1.0 + (phi - prev_phi)); prev_phi = phi.
 * prev_phi_dev: (N) f64, the potential of the observation the wrapper last saw; the reset entry
 * and a NEXT_STEP autoreset row (reward 0) set it to phi(reset observation).  shaper == 0: no
 * shaping (reward 1).  state_dev stays (N, 4) f64. */
typedef struct gs_cartpole_wrappers {
    int32_t shaper;                 /* 1: CartPoleV1_RewardShaper */
    int32_t clip_potential;
    double angle_reward_scale, position_reward_scale;
} gs_cartpole_wrappers;
int gs_cartpole_shaped_reset(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                             float *obs_dev, gs_cartpole_wrappers wrappers, int64_t N, uint64_t seed,
                             int64_t env_offset, void *stream);
int gs_cartpole_shaped_step(double *state_dev, double *prev_phi_dev, int32_t *meta_dev, float *ep_ret_dev,
                            float *obs_dev, gs_cartpole_wrappers wrappers, const int64_t *actions_dev, int64_t N,
                            int32_t max_steps, uint64_t seed, int64_t env_offset, float *rewards_row_dev,
                            uint8_t *dones_row_dev, uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev,
                            float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream);
/* gs_rollout_env for the shaped CartPole (gs_rollout_env_supported's kind GS_ENV_CARTPOLE answers
 * for it: obs dim 4, 2 actions): bit for bit T calls of gs_policy_act + gs_cartpole_shaped_step,
 * prev_phi included. */
int gs_rollout_cartpole_shaped(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                               uint64_t rng_seed, uint64_t rng_counter0, double *env_state_dev,
                               double *env_prev_phi_dev, int32_t *env_meta_dev, float *env_ep_ret_dev,
                               float *env_obs_dev, gs_cartpole_wrappers wrappers, int32_t max_steps,
                               uint64_t env_seed, int64_t env_offset, int32_t *ep_done_count_dev,
                               float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows_dev,
                               int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev,
                               float *reward_rows_dev, uint8_t *done_rows_dev, uint8_t *timeout_rows_dev,
                               void *stream);

/* ---------------------------------------------------------------- Bandit-v0 (f1)
 * The reference's gym_envs/mab_env.py MultiArmedBanditEnv on device: a stateless Gaussian
 * multi-armed bandit.  obs_dev (N, n_arms) f32 is all zeros, on reset and after every step;
 * actions in [0, n_arms) (an action outside is clamped into the range); reward =
 * (float)((double)means[a] + (double)stds[a] * z); terminated when the steps in the episode reach
 * episode_length; TimeLimit max_steps (truncated = !terminated && steps >= max_steps); NEXT_STEP
 * autoreset; meta_dev (N, 3) i32 {steps, episodes, pending}, rows and counters as
 * gs_cartpole_step.  There is no state tensor.
 * z is a standard normal by Box-Muller, z = sqrt(-2 log(1 - u1)) cos(2 pi u2), with u1, u2 the
 * 53-bit uniforms of the counter hash of (seed, env_offset + env, episode, step in episode,
 * component) on tags of its own: it depends on those counters only, so the step loop, a captured
 * graph and the one-launch rollout draw the same bits.  numpy's PCG64 ziggurat stream is not
 * reproduced: parity with the reference's own reward stream is unpinned, as for every device env. */
#define GS_BANDIT_MAX_ARMS 32
typedef struct gs_bandit_spec {
    int32_t n_arms, episode_length;            /* 2 .. GS_BANDIT_MAX_ARMS, >= 1 */
    float means[GS_BANDIT_MAX_ARMS], stds[GS_BANDIT_MAX_ARMS];   /* stds >= 0 */
} gs_bandit_spec;
int gs_bandit_reset(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec, int64_t N,
                    void *stream);
int gs_bandit_step(int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_bandit_spec spec,
                   const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                   float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                   int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream);
/* gs_rollout_env for the bandit (gs_rollout_env_supported's kind GS_ENV_BANDIT: obs dim ==
 * n_actions in [2, GS_BANDIT_ROLLOUT_MAX_ARMS] and a policy that fits in LDS; more arms take the
 * step loop): bit for bit T calls of gs_policy_act + gs_bandit_step.  The bound is the
 * reference config's 10 arms: the kernel is instantiated for that action count alone. */
#define GS_BANDIT_ROLLOUT_MAX_ARMS 10
int gs_rollout_bandit(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                      uint64_t rng_counter0, int32_t *env_meta_dev, float *env_ep_ret_dev, float *env_obs_dev,
                      gs_bandit_spec spec, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                      int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows_dev,
                      int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev, float *reward_rows_dev,
                      uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);

/* ---------------------------------------------------------------- Acrobot-v1 dynamics (f1)
 * gymnasium 1.x AcrobotEnv.step ("book" variant, no torque noise) restated on device: state
 * {theta1, theta2, omega1, omega2} in double precision, one classical RK4 step of dt 0.2 under
 * torque action - 1, angles wrapped into [-pi, pi] (at most 16 turns each way, so a non-finite
 * state cannot spin), velocities clamped to 4 pi / 9 pi, terminated when
 * -cos(theta1) - cos(theta1 + theta2) > 1, reward -1 (0 on the terminating step), TimeLimit
 * max_steps, NEXT_STEP autoreset.  obs_dev: (N, 6) f32 {cos t1, sin t1, cos t2, sin t2, w1, w2}.
 * state_dev / meta_dev / actions_dev / rows / counters as gs_cartpole_step.  Reset draws are
 * uniform in [-0.1, 0.1) from the counter hash, rounded to float32 (gymnasium's PCG64 stream is
 * not reproduced: parity with gymnasium's own episodes is unpinned, as for CartPole). */
int gs_acrobot_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int64_t N,
                     uint64_t seed, int64_t env_offset, void *stream);
int gs_acrobot_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev,
                    const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed, int64_t env_offset,
                    float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                    int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream);

/* ---------------------------------------------------------------- MountainCar-v0 dynamics (f1)
 * gymnasium 1.x MountainCarEnv.step restated on device, with the reference's two MountainCar
 * reward wrappers (gym_wrappers/MountainCarV0/reward_shaper.py, state_count_bonus.py) applied on
 * the env's own thread.  state_dev: (N, 4) f64 {position, velocity, prev_position, prev_velocity}
 * (prev_*: the float32 observation the shaper last saw).  Double precision: v += (a - 1) 0.001 +
 * cos(3 p) (-0.0025), v clipped to +-0.07, p += v, p clipped to [-1.2, 0.6], v = 0 at the left
 * wall; terminated when p >= 0.5 and v >= 0; reward -1 on every step; TimeLimit max_steps;
 * NEXT_STEP autoreset (the reset step adds no wrapper term).  obs_dev: (N, 2) f32.  Reset: p
 * uniform in [-0.6, -0.4) from the counter hash (kept in double), v = 0; gymnasium's PCG64 stream
 * is not reproduced (parity with gymnasium's own episodes is unpinned).
 * Wrappers (gs_mountaincar_wrappers, by value): order[] lists up to two of GS_MC_WRAP_SHAPER /
 * GS_MC_WRAP_BONUS, innermost first, each at most once, GS_MC_WRAP_NONE in the unused slots; they
 * work in double on the float32 observation and the step's reward is (float)(-1 + addends in
 * that order).  The count bonus reads and increments counts_dev: (N, position_bins *
 * velocity_bins) i32, env e's row only by env e's thread (no atomics); gs_mountaincar_reset
 * zeroes it, an episode boundary does not.  counts_dev may be null without a count bonus.
 * meta_dev / actions_dev / rows / counters as gs_cartpole_step. */
#define GS_MC_WRAP_NONE 0
#define GS_MC_WRAP_SHAPER 1
#define GS_MC_WRAP_BONUS 2
#define GS_MC_BONUS_COUNT 0     /* scale / sqrt(max(count, min_count)) */
#define GS_MC_BONUS_INVERSE 1   /* scale / max(count, min_count) */
#define GS_MC_BONUS_LOG 2       /* scale / log(max(count, min_count) + 1) */
typedef struct gs_mountaincar_wrappers {
    int32_t order[2];
    double position_reward_scale, velocity_reward_scale, height_reward_scale;
    int32_t position_bins, velocity_bins;      /* > 0, product <= 16384 */
    int32_t bonus_type, min_count;             /* GS_MC_BONUS_*, >= 1 */
    double bonus_scale;
} gs_mountaincar_wrappers;
int gs_mountaincar_reset(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int32_t *counts_dev,
                         gs_mountaincar_wrappers wrappers, int64_t N, uint64_t seed, int64_t env_offset, void *stream);
int gs_mountaincar_step(double *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, int32_t *counts_dev,
                        gs_mountaincar_wrappers wrappers, const int64_t *actions_dev, int64_t N, int32_t max_steps,
                        uint64_t seed, int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev,
                        uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                        float *ep_len_sum_dev, void *stream);
/* gs_rollout_env for MountainCar (kind GS_ENV_MOUNTAINCAR: obs dim 2, 3 actions): the same
 * one-launch rollout with the env's count tables and wrappers; the tables stay in HBM (L2), the
 * kernel's LDS budget is gs_rollout_env's.  Bit for bit T calls of gs_policy_act +
 * gs_mountaincar_step, counts included. */
int gs_rollout_mountaincar(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                           uint64_t rng_seed, uint64_t rng_counter0, double *env_state_dev, int32_t *env_meta_dev,
                           float *env_ep_ret_dev, float *env_obs_dev, int32_t *env_counts_dev,
                           gs_mountaincar_wrappers wrappers, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                           int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                           float *obs_rows_dev, int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev,
                           float *reward_rows_dev, uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);

/* ---------------------------------------------------------------- tabular envs (FrozenLake-v1, Taxi-v3)
 * Any finite MDP whose outcomes per (state, action) are n_outcomes equiprobable alternatives, as
 * three read-only tables in HBM: next_dev i32 [S][A][K], reward_dev f32 [S][A][K], term_dev u8
 * [S][A][K] (terminated).  gsamd/toytext.py restates gymnasium 1.x FrozenLake-v1 (4x4 / 8x8;
 * slippery K = 3, else K = 1) and Taxi-v3 (K = 1) in this form; gymnasium's PCG64 stream is not
 * reproduced, so parity with its own episodes is unpinned, as for the other device envs.
 * state_dev: (N) i32; meta_dev (N, 3) i32 {steps, episodes, pending}; NEXT_STEP autoreset (a reset
 * step only resets: reward 0, not done), TimeLimit max_steps, rows and episode counters as
 * gs_cartpole_step.  Outcome of a step: k = min(K - 1, (int)(u K)), u in [0, 1) from the counter
 * hash of (seed, env_offset + env, episode, step in episode) on a stream of its own; reset:
 * starts_dev[min(n_starts - 1, (int)(u n_starts))] with u the reset hash of (seed, env_offset + env,
 * episode), so trajectories do not depend on the launch geometry or on how env_offset partitions
 * the envs.  Every table index is range-checked on device: an action outside [0, A) is clamped, a
 * next state outside [0, S) ends the episode in place.
 * obs_dev (N, obs_dim) f32 is the reference's gym_wrappers/discrete_encoder.py of the state:
 * GS_ENC_ARRAY [(float)s] (the reference keeps int64 there; the MLP's input is its float32 value),
 * GS_ENC_BINARY the max(1, ceil(log2 S)) bits LSB first, GS_ENC_ONEHOT the unit vector (S <= 64, the
 * policy's obs_dim limit; GS_E_INVALID beyond).  spec.obs_dim must be the encoding's. */
#define GS_ENC_ARRAY 0
#define GS_ENC_BINARY 1
#define GS_ENC_ONEHOT 2
typedef struct gs_tabular_spec {
    int32_t n_states, n_actions, n_outcomes;   /* K >= 1 */
    int32_t n_starts;                          /* reset: uniform over starts_dev[0..n_starts) */
    int32_t encoding;                          /* GS_ENC_ARRAY / GS_ENC_BINARY / GS_ENC_ONEHOT */
    int32_t obs_dim;                           /* 1 / max(1, ceil(log2 n_states)) / n_states */
} gs_tabular_spec;
int gs_tabular_reset(int32_t *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_tabular_spec spec,
                     const int32_t *starts_dev, int64_t N, uint64_t seed, int64_t env_offset, void *stream);
int gs_tabular_step(int32_t *state_dev, int32_t *meta_dev, float *ep_ret_dev, float *obs_dev, gs_tabular_spec spec,
                    const int32_t *next_dev, const float *reward_dev, const uint8_t *term_dev,
                    const int32_t *starts_dev, const int64_t *actions_dev, int64_t N, int32_t max_steps, uint64_t seed,
                    int64_t env_offset, float *rewards_row_dev, uint8_t *dones_row_dev, uint8_t *timeouts_row_dev,
                    int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, void *stream);

/* ---------------------------------------------------------------- one-launch rollouts, one hidden layer
 * A whole rollout of a device env in ONE launch for the one-hidden-layer policy (hidden2 == 0;
 * csrc/gs_mlp1.hip k_rollout1): one thread owns one env for all T vector steps, the parameters in
 * LDS, the env's state in registers, its observation in the thread's own LDS row; a workgroup is
 * one wave of 64 envs and the result does not depend on that split.  The forward is
 * gs_policy_act's one-hidden-layer arithmetic in its order, the env step the env's gs_*_step, so
 * every row, the final env tensors and the episode counters equal T calls of gs_policy_act + the
 * env's step bit for bit, in all three modes (mode 2 reads action_rows_dev) and for any N; the rng
 * counter of step t is rng_counter0 + t and the row id the env's index.  These entries take
 * hidden2 == 0 only (GS_E_INVALID otherwise; the gs_rollout_* entries above keep refusing it and
 * gs_rollout_env_supported keeps answering 0), check what their two-hidden-layer siblings check,
 * need dims to be the env's (obs dim and actions) and do nothing for T == 0.
 * gs_rollout1_supported: *supported_host = 1 when dims lie in the one-hidden-layer envelope (beside
 * gs_mlp_dims) and 4 (round4(P) + 64 (obs_dim | 1)) bytes fit in 160 KiB of LDS, 0 with GS_OK for
 * a valid shape that does not fit, GS_E_INVALID for hidden2 != 0 or dims outside the envelope.
 * gs_rollout1_env (kind GS_ENV_CARTPOLE / GS_ENV_ACROBOT), gs_rollout1_cartpole_shaped,
 * gs_rollout1_mountaincar and gs_rollout1_bandit take the argument lists of gs_rollout_env,
 * gs_rollout_cartpole_shaped, gs_rollout_mountaincar and gs_rollout_bandit unchanged (the bandit
 * up to GS_BANDIT_MAX_ARMS arms).  gs_rollout1_tabular takes the tabular env's tensors, spec and
 * tables as gs_tabular_step does (the same spec / table checks; dims.obs_dim == spec.obs_dim,
 * dims.n_actions == spec.n_actions) between the policy arguments and the episode counters. */
int gs_rollout1_supported(gs_mlp_dims dims, int *supported_host);
int gs_rollout1_env(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                    uint64_t rng_counter0, int kind, double *env_state_dev, int32_t *env_meta_dev,
                    float *env_ep_ret_dev, float *env_obs_dev, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                    int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows_dev,
                    int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev, float *reward_rows_dev,
                    uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);
int gs_rollout1_cartpole_shaped(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                                uint64_t rng_seed, uint64_t rng_counter0, double *env_state_dev,
                                double *env_prev_phi_dev, int32_t *env_meta_dev, float *env_ep_ret_dev,
                                float *env_obs_dev, gs_cartpole_wrappers wrappers, int32_t max_steps, uint64_t env_seed,
                                int64_t env_offset, int32_t *ep_done_count_dev, float *ep_ret_sum_dev,
                                float *ep_len_sum_dev, float *obs_rows_dev, int64_t *action_rows_dev,
                                float *logp_rows_dev, float *value_rows_dev, float *reward_rows_dev,
                                uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);
int gs_rollout1_mountaincar(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode,
                            uint64_t rng_seed, uint64_t rng_counter0, double *env_state_dev, int32_t *env_meta_dev,
                            float *env_ep_ret_dev, float *env_obs_dev, int32_t *env_counts_dev,
                            gs_mountaincar_wrappers wrappers, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                            int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                            float *obs_rows_dev, int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev,
                            float *reward_rows_dev, uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);
int gs_rollout1_bandit(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                       uint64_t rng_counter0, int32_t *env_meta_dev, float *env_ep_ret_dev, float *env_obs_dev,
                       gs_bandit_spec spec, int32_t max_steps, uint64_t env_seed, int64_t env_offset,
                       int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev, float *obs_rows_dev,
                       int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev, float *reward_rows_dev,
                       uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);
int gs_rollout1_tabular(const float *params_dev, gs_mlp_dims dims, int64_t N, int64_t T, int mode, uint64_t rng_seed,
                        uint64_t rng_counter0, int32_t *state_dev, int32_t *meta_dev, float *ep_ret_dev,
                        float *obs_dev, gs_tabular_spec spec, const int32_t *next_dev, const float *reward_dev,
                        const uint8_t *term_dev, const int32_t *starts_dev, int32_t max_steps, uint64_t seed,
                        int64_t env_offset, int32_t *ep_done_count_dev, float *ep_ret_sum_dev, float *ep_len_sum_dev,
                        float *obs_rows_dev, int64_t *action_rows_dev, float *logp_rows_dev, float *value_rows_dev,
                        float *reward_rows_dev, uint8_t *done_rows_dev, uint8_t *timeout_rows_dev, void *stream);

/* The fp32 MFMA GEMM under the CNN path (convolutions as GEMMs, fc, heads), exported for its
 * tests: row-major C[M][N] = op(A) op(B) + beta C (+ bias[n]) (ReLU if relu), op(X) = X^T
 * when t* != 0 (A stored K x M, B stored N x K). */
int gs_gemm_f32(int ta, int tb, int64_t M, int64_t N, int64_t K, const float *A_dev, int64_t lda,
                const float *B_dev, int64_t ldb, float *C_dev, int64_t ldc, float beta, const float *bias_dev,
                int relu, void *stream);
/* The NatureCNN fc layer's three GEMMs (utils/models.py:56-110: h = relu(a3 Wf^T + bf) and its
 * backward) on the hand-written MFMA kernels the update runs (csrc/gs_fc.hip), exposed for
 * parity tests: op 0 C[M][N] = relu(A[M][K] B[N][K]^T + aux[N]); op 1 C = A^T B with A [K][M],
 * B [K][N]; op 2 C = (A B) .* (aux > 0) with A [M][K], B [K][N], aux [M][ldc].  bf16 != 0: bf16
 * operands (round to nearest even), fp32 accumulation.  GS_E_INVALID for shapes outside
 * K % 64 == 0, 16-B aligned rows (and M, N % 4 == 0 for K-strided operands).  parts_dev (may be NULL;
 * 2 M N floats): with it the fp32 forward runs the update's split-K form (two K halves summed in
 * order, then the bias + ReLU epilogue), without it the single-pass form (ABI 6 added it). */
int gs_fc_gemm(int op, int bf16, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda, const float *B,
               int64_t ldb, float *C, int64_t ldc, const float *aux, float *parts_dev, void *stream);

/* ---------------------------------------------------------------- Atari pixel path (a13)
 * The observation pipeline of ale-py's AtariVectorEnv / gymnasium AtariPreprocessing +
 * FrameStackObservation (utils/environment.py:240-303, :362-385), on device: two raw
 * 210x160x3 u8 frames per env step -> OpenCV-RGB2GRAY grayscale -> max of the two -> area
 * resize to out_h x out_w -> stack of stack_n frames, newest last, zero padding after reset.
 * The frame source is synthetic (hash of seed, env, frame, byte): ALE itself is not
 * available offline.  frames_dev: (N, 2, 210, 160, 3) u8 scratch; stack_dev: (N, stack_n,
 * out_h, out_w) u8 = the observation; state_dev: 4 int32 per env; counters and rows as
 * gs_env_step. */
int gs_atari_preprocess(const uint8_t *frames_dev, int64_t N, int32_t out_h, int32_t out_w, uint8_t *out_dev,
                        void *stream);
int gs_atari_render(uint8_t *frames_dev, int64_t N, uint64_t seed, int64_t env_offset, uint64_t step_count,
                    void *stream);
int gs_atari_env_reset(int32_t *state_dev, float *ep_ret_dev, uint8_t *stack_dev, uint8_t *frames_dev, int64_t N,
                       int32_t stack_n, int32_t out_h, int32_t out_w, int32_t episode_len, uint64_t seed,
                       int64_t env_offset, void *stream);
int gs_atari_env_step(int32_t *state_dev, float *ep_ret_dev, uint8_t *stack_dev, uint8_t *frames_dev, int64_t N,
                      int32_t stack_n, int32_t out_h, int32_t out_w, int32_t episode_len, int32_t truncate_every,
                      uint64_t seed, int64_t env_offset, uint64_t step_count, float *rewards_row_dev,
                      uint8_t *dones_row_dev, uint8_t *timeouts_row_dev, int32_t *ep_done_count_dev,
                      float *ep_ret_sum_dev, float *ep_len_sum_dev, const uint64_t *clock_dev, void *stream);

/* ---------------------------------------------------------------- multi-GPU (xGMI / RCCL)
 * One process per GPU; replaces the reference's single-process gradient step
 * (agents/base_agent.py:331-355 manual_backward + optimizer.step) with a data-parallel
 * mean over ranks.  Two transports behind the same handle:
 *   RCCL: rank 0 creates the 128-byte unique id, the launcher broadcasts it
 *         (torch.distributed), every rank calls gs_comm_init.
 *   xGMI one-shot (default for the update): every rank calls gs_comm_xgmi_create (allocates
 *         and IPC-exports its exchange region, max_count = largest exchange in floats),
 *         the launcher all-gathers the 64-byte handles in rank order, every rank calls
 *         gs_comm_xgmi_connect; after a barrier the communicator is ready.  A wait that
 *         exceeds GS_XGMI_TIMEOUT_S (default 120 s) sets a sticky error that
 *         gs_comm_status reports (GS_E_COMM); later exchanges then fail fast. */
int gs_comm_unique_id(uint8_t out_id[128]);
int gs_comm_init(const uint8_t id[128], int nranks, int rank, struct gs_comm **out);
int gs_comm_xgmi_create(int nranks, int rank, int64_t max_count, uint8_t out_handle[64], struct gs_comm **out);
int gs_comm_xgmi_connect(struct gs_comm *comm, const uint8_t *handles);
int gs_comm_status(struct gs_comm *comm);
/* The first timeout's record (host-only read of the region, synchronous): *timed_out = 1 when a
 * wait gave up; then *workgroup = the exchange workgroup that waited, *peer = the rank it waited
 * for, *site = where (1 exchange launch, 2 / 3 reduce-scatter / all-gather flags of the rsag
 * launch, 4 / 5 push / result flags of the exchange inside k_bwd); -1 / 0 when none.  Any out
 * pointer may be NULL.  gs_comm_status's message carries the same record. */
int gs_comm_error_record(struct gs_comm *comm, int *timed_out, int *workgroup, int *peer, int *site);
/* The MLP update's exchange runs inside the backward kernel (every workgroup waits for the
 * same workgroup of its peers), which needs the peers' workgroups to be resident together.
 * That always holds with one rank per GPU (a node); with c ranks sharing a GPU it needs
 * (c - 1) backward grids to leave a free workgroup slot, and even then the ranks are separate
 * processes, which the GPU time-slices rather than co-schedules.  The launcher reports the
 * largest number of ranks sharing one GPU here; until it does (more than one rank) the
 * colocation counts as unknown and the update exchanges with a separate launch after the
 * backward, as it does from 2 ranks per GPU (GS_XGMI_BWD=1 forces the in-backward form where the
 * grids fit: correct, but paced by the time-slicing).  Host-only, no GPU call. */
int gs_comm_xgmi_set_colocation(struct gs_comm *comm, int ranks_per_device);
/* Where the MLP update exchanges on this communicator: mode 0 = always a separate exchange
 * launch after the backward, 1 = inside the backward where one rank runs per GPU (the default),
 * 2 = inside the backward also for ranks sharing a GPU (GS_XGMI_BWD=1).  The launcher's
 * connect-time self-test (gsamd.distributed.init_xgmi_comm) runs the in-backward form on the
 * job's shapes and sets mode 0 on every rank when it fails.  Every rank must set the same mode
 * before its next update; captured update graphs are keyed by it.  Host-only, no GPU call. */
int gs_comm_xgmi_set_bwd_exchange(struct gs_comm *comm, int mode);
/* Back to the connect-time protocol state after a failed or timed-out exchange: this rank's flag
 * banks, sticky error word and sequence counters are zeroed (synchronous).  Collective in the
 * caller's protocol: every rank drains its device work, meets the others at a host barrier, calls
 * this, and meets them again before the next exchange (gsamd.distributed.xgmi_reset). */
int gs_comm_xgmi_reset(struct gs_comm *comm);
int gs_comm_allreduce_mean_f32(struct gs_comm *comm, float *buf_dev, int64_t count, void *stream);
/* Sum of `count` doubles over ranks, in place (16-B aligned buffer), the same result bits on every
 * rank: xGMI sums the sources in rank order in double (pieces of the communicator's capacity),
 * RCCL runs ncclAllReduce(ncclFloat64, ncclSum).  Stream-ordered. */
int gs_comm_allreduce_sum_f64(struct gs_comm *comm, double *buf_dev, int64_t count, void *stream);
/* What a communicator is: its rank count, this process's rank and the transport
 * (GS_COMM_RCCL / GS_COMM_XGMI).  Any out pointer may be NULL.  Host-only, no GPU call. */
#define GS_COMM_RCCL 0
#define GS_COMM_XGMI 1
int gs_comm_info(struct gs_comm *comm, int *nranks, int *rank, int *transport);
int gs_comm_destroy(struct gs_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* GSAMD_H */
