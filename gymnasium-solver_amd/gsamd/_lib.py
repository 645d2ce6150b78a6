"""ctypes binding of libgsamd.so (the C-ABI declared in include/gsamd.h).

The library is built in-tree by ``__graft_entry__.build()`` and linked against the same
HIP runtime soname torch loads (libamdhip64.so.7), so importing torch first makes both
share one runtime.  There is no fallback: if the library is missing, importing any
device module raises, loudly.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before the library)

# GSAMD_LIB selects a diagnostic build of the same library (tools/ phase-timer variant)
LIB_PATH = os.environ.get("GSAMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgsamd.so")

GS_OK, GS_E_INVALID, GS_E_HIP, GS_E_COMM = 0, -1, -2, -3
GS_ABI_VERSION = 7          # include/gsamd.h: the argument lists this binding declares
GS_NUM_METRICS = 40
GS_ENV_SYNTHETIC, GS_ENV_CARTPOLE, GS_ENV_ACROBOT = 0, 1, 2     # include/gsamd.h: gs_rollout_env kinds
GS_ENV_MOUNTAINCAR = 3      # answered by gs_rollout_env_supported; rolled out by gs_rollout_mountaincar
GS_ENV_BANDIT = 4           # answered by gs_rollout_env_supported; rolled out by gs_rollout_bandit
GS_MC_WRAP_NONE, GS_MC_WRAP_SHAPER, GS_MC_WRAP_BONUS = 0, 1, 2
GS_MC_BONUS_TYPES = {"count": 0, "inverse": 1, "log": 2}       # GS_MC_BONUS_*
METRIC_SLOTS = (
    "loss", "policy_loss", "value_loss", "entropy", "clip_fraction", "clip_fraction_vf",
    "explained_var", "kl", "approx_kl", "adv_norm_mean", "adv_norm_std", "kl_stop", "grad_norm",
    "skipped", "unevaluated", "res1",
    # pre-clip per-component gradient norms (utils/models.py:196-230)
    # slots 20 / 21: GS_M_PG_TARGET_MEAN / _STD in gs_pg_update's records (M["pg_target_mean"], M["pg_target_std"])
    "gn_backbone", "gn_policy_head", "gn_value_head", "gn_mlp", "res20", "res21", "res22", "res23",
    # GS_HP_ACT_STATS: per hooked layer {mean, std, dead_pct, dead_max} (utils/models.py:121-147)
    *(f"act{l}_{k}" for l in range(4) for k in ("mean", "std", "dead_pct", "dead_max")),
)
ACT_SLOT = 24                # GS_M_ACT
M = {name: i for i, name in enumerate(METRIC_SLOTS)}
M["pg_target_mean"], M["pg_target_std"] = M["res20"], M["res21"]


class MlpDims(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("hidden1", ctypes.c_int32), ("hidden2", ctypes.c_int32),
                ("n_actions", ctypes.c_int32)]


class MountainCarWrappers(ctypes.Structure):
    """gs_mountaincar_wrappers (include/gsamd.h): up to two wrappers, innermost first."""
    _fields_ = [("order", ctypes.c_int32 * 2), ("position_reward_scale", ctypes.c_double),
                ("velocity_reward_scale", ctypes.c_double), ("height_reward_scale", ctypes.c_double),
                ("position_bins", ctypes.c_int32), ("velocity_bins", ctypes.c_int32),
                ("bonus_type", ctypes.c_int32), ("min_count", ctypes.c_int32), ("bonus_scale", ctypes.c_double)]


class CartPoleWrappers(ctypes.Structure):
    """gs_cartpole_wrappers (include/gsamd.h): the CartPoleV1_RewardShaper's parameters."""
    _fields_ = [("shaper", ctypes.c_int32), ("clip_potential", ctypes.c_int32),
                ("angle_reward_scale", ctypes.c_double), ("position_reward_scale", ctypes.c_double)]


GS_BANDIT_MAX_ARMS = 32             # include/gsamd.h
GS_BANDIT_ROLLOUT_MAX_ARMS = 10     # the one-launch rollout's bound; more arms take the step loop


class BanditSpec(ctypes.Structure):
    """gs_bandit_spec (include/gsamd.h): the arms' float32 means and stds, by value."""
    _fields_ = [("n_arms", ctypes.c_int32), ("episode_length", ctypes.c_int32),
                ("means", ctypes.c_float * GS_BANDIT_MAX_ARMS), ("stds", ctypes.c_float * GS_BANDIT_MAX_ARMS)]


GS_ENCODINGS = {"array": 0, "binary": 1, "onehot": 2}          # GS_ENC_*


class TabularSpec(ctypes.Structure):
    """gs_tabular_spec (include/gsamd.h): the shape of a tabular env and its observation encoding."""
    _fields_ = [("n_states", ctypes.c_int32), ("n_actions", ctypes.c_int32), ("n_outcomes", ctypes.c_int32),
                ("n_starts", ctypes.c_int32), ("encoding", ctypes.c_int32), ("obs_dim", ctypes.c_int32)]


class PPOHparams(ctypes.Structure):
    _fields_ = [("clip_range", ctypes.c_float), ("clip_range_vf", ctypes.c_float), ("vf_coef", ctypes.c_float),
                ("ent_coef", ctypes.c_float), ("max_grad_norm", ctypes.c_float), ("lr", ctypes.c_float),
                ("adam_beta1", ctypes.c_float), ("adam_beta2", ctypes.c_float), ("adam_eps", ctypes.c_float),
                ("target_kl", ctypes.c_float), ("normalize_adv", ctypes.c_int32), ("flags", ctypes.c_int32)]


class PGHparams(ctypes.Structure):
    """gs_pg_hparams (include/gsamd.h): the REINFORCE update's hyper-parameters."""
    _fields_ = [("ent_coef", ctypes.c_float), ("max_grad_norm", ctypes.c_float), ("lr", ctypes.c_float),
                ("adam_beta1", ctypes.c_float), ("adam_beta2", ctypes.c_float), ("adam_eps", ctypes.c_float),
                ("normalize_targets", ctypes.c_int32), ("flags", ctypes.c_int32)]


GS_MC_RTG, GS_MC_EPISODE = 0, 1     # include/gsamd.h: gs_mc_returns_f32 kinds
GS_HP_BF16 = 1      # include/gsamd.h: bf16 MFMA operands in the NatureCNN update
GS_HP_ACT_STATS = 2  # include/gsamd.h: per-minibatch activation statistics into the records (GS_M_ACT)
GS_HP_OPT_ADAMW = 4  # include/gsamd.h: torch.optim.AdamW's step (decoupled decay GS_ADAMW_WEIGHT_DECAY); neither bit: Adam
GS_HP_OPT_SGD = 8    # include/gsamd.h: torch.optim.SGD's step (no momentum, no decay)
GS_ADAMW_WEIGHT_DECAY = 0.01
OPT_FLAGS = {"adam": 0, "adamw": GS_HP_OPT_ADAMW, "sgd": GS_HP_OPT_SGD}   # config.optimizer -> the flags bit


class RolloutView(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("logprobs", ctypes.c_void_p),
                ("values", ctypes.c_void_p), ("advantages", ctypes.c_void_p), ("returns", ctypes.c_void_p),
                ("T", ctypes.c_int64), ("N", ctypes.c_int64)]


class PPOGlobal(ctypes.Structure):
    """gs_ppo_global (include/gsamd.h): the global-minibatch mode's extra arguments."""
    _fields_ = [("batch_global", ctypes.c_int64), ("adv_stats", ctypes.c_void_p), ("metric_sums", ctypes.c_void_p)]


class CnnDims(ctypes.Structure):
    _fields_ = [("in_c", ctypes.c_int32), ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32),
                ("n_actions", ctypes.c_int32), ("hidden", ctypes.c_int32), ("valid_mask", ctypes.c_uint32)]


class RolloutViewU8(ctypes.Structure):
    _fields_ = RolloutView._fields_


class GsError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is not built: the device path has no CPU fallback. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repo root.")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp, i32, i64, u64, f32, f64, sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
                                       ctypes.c_float, ctypes.c_double, ctypes.c_size_t)
    # The env and rollout entries' lists, from the groups gsamd.rollout.DeviceVecEnv forms its calls of:
    # an env's own group (its tensors and parameters), then per entry
    #   reset:   group, N, seed, env_offset, stream
    #   step:    group, actions, N, max_steps, seed, env_offset, 3 rows, 3 episode counters, stream
    #   rollout: head, [env_kind,] group, max_steps, seed, env_offset, 3 episode counters, 7 rows, stream
    plain = [vp, vp, vp, vp]                                   # state, meta, ep_ret, obs
    groups = {"cartpole": plain, "acrobot": plain,
              "cartpole_shaped": [vp, vp, vp, vp, vp, CartPoleWrappers],       # state, prev_phi, meta, ..., wrappers
              "mountaincar": [vp, vp, vp, vp, vp, MountainCarWrappers],        # ..., obs, counts, wrappers
              "bandit": [vp, vp, vp, BanditSpec],                              # meta, ep_ret, obs, spec: no state
              "tabular": [vp, vp, vp, vp, TabularSpec, vp, vp, vp, vp]}        # ..., obs, spec, 3 tables, starts
    reset_tail = [i64, u64, i64, vp]
    step_tail = [vp, i64, i32, u64, i64] + [vp] * 7
    head = [vp, MlpDims, i64, i64, ctypes.c_int, u64, u64]     # params, dims, N, T, mode, rng_seed, counter0
    run = [i32, u64, i64, vp, vp, vp]                          # max_steps, seed, env_offset, the counters
    rows = [vp] * 8                                            # the buffer's seven rows, the stream
    rollouts = {"env": head + [ctypes.c_int] + plain + run + rows,
                **{x: head + groups[x] + run + rows for x in ("cartpole_shaped", "mountaincar", "bandit", "tabular")}}
    sig = {
        "gs_abi_version": (ctypes.c_int, []),
        "gs_last_error": (ctypes.c_char_p, []),
        "gs_build_source_hash": (ctypes.c_char_p, [ctypes.c_char_p]),
        "gs_normalize_advantages_scratch_bytes": (sz, [i64]),
        "gs_normalize_advantages": (ctypes.c_int, [vp, i64, f32, vp, vp, vp]),
        "gs_cnn_activation_stats": (ctypes.c_int, [vp, CnnDims, RolloutViewU8, vp, i64, vp, vp, vp]),
        "gs_gae_f32": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, f64, f64, vp, vp, vp]),
        "gs_sampler_stream_i32": (ctypes.c_int, [i64, i64, u64, vp, ctypes.c_int]),
        "gs_mc_returns_f32": (ctypes.c_int, [vp, vp, vp, i64, i64, f64, ctypes.c_int, vp, vp, vp, vp, vp]),
        "gs_pg_update_workspace_bytes": (sz, [MlpDims, i64]),
        "gs_pg_update": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PGHparams, RolloutView, vp, i64, i64, i64, vp, vp, sz,
                                        vp, vp]),
        "gs_pg_loss": (ctypes.c_int, [vp, vp, MlpDims, PGHparams, RolloutView, vp, i64, vp, vp, sz, vp]),
        "gs_ppo_rows_workspace_bytes": (sz, [MlpDims, i64]),
        "gs_ppo_rows_update": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, i64, i64, vp,
                                              vp, vp, sz, vp, vp]),
        "gs_ppo_rows_loss": (ctypes.c_int, [vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, vp, vp, sz, vp]),
        # the masked head's entries: their unmasked sibling's list + valid_mask (bit a set = action a valid)
        "gs_ppo_rows_update_masked": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, i64, i64,
                                                     vp, vp, vp, sz, vp, vp, ctypes.c_uint32]),
        "gs_ppo_rows_loss_masked": (ctypes.c_int, [vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, vp, vp, sz, vp,
                                                   ctypes.c_uint32]),
        "gs_policy_act_masked": (ctypes.c_int, [vp, MlpDims, vp, i64, ctypes.c_int, u64, u64, vp, vp, vp, vp, vp, vp, vp,
                                                ctypes.c_uint32]),
        "gs_mlp_param_count": (i64, [MlpDims]),
        "gs_policy_scratch_bytes": (sz, [MlpDims, i64]),
        "gs_policy_act": (ctypes.c_int, [vp, MlpDims, vp, i64, ctypes.c_int, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "gs_policy_value": (ctypes.c_int, [vp, MlpDims, vp, i64, vp, vp, vp]),
        "gs_rollout_synth_supported": (ctypes.c_int, [MlpDims, vp]),
        # state, ep_ret, obs, episode_len, truncate_every, reward, seed, env_offset, step count, the counters
        "gs_rollout_synth": (ctypes.c_int, head + [vp, vp, vp, i32, i32, f32, u64, i64, u64, vp, vp, vp] + rows),
        "gs_rollout_env_supported": (ctypes.c_int, [MlpDims, ctypes.c_int, vp]),
        "gs_env_reset": (ctypes.c_int, [vp, vp, vp, i64, i32, i32, u64, i64, vp]),
        "gs_env_step": (ctypes.c_int, [vp, vp, vp, i64, i32, i32, i32, f32, u64, i64, u64, vp, vp, vp, vp, vp,
                                       vp, vp, vp]),
        "gs_episode_stats": (ctypes.c_int, [vp, vp, i64, i64, vp, vp, vp, vp, vp]),
        "gs_episode_window": (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp]),
        "gs_ppo_workspace_bytes": (sz, [MlpDims, i64]),
        "gs_ppo_minibatch_step": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, i64,
                                                 vp, vp, vp, vp, vp]),
        "gs_ppo_loss": (ctypes.c_int, [vp, MlpDims, PPOHparams, RolloutView, vp, i64, vp, vp, vp]),
        "gs_mlp_activation_stats": (ctypes.c_int, [vp, MlpDims, RolloutView, vp, i64, vp, vp]),
        "gs_ppo_stage": (ctypes.c_int, [ctypes.c_int, vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64,
                                        i64, vp, vp, vp]),
        "gs_ppo_update": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, i64, i64, vp,
                                         vp, vp, sz, vp, ctypes.c_int, vp]),
        "gs_ppo_update_global": (ctypes.c_int, [vp, vp, vp, vp, MlpDims, PPOHparams, RolloutView, vp, i64, i64, i64,
                                                vp, vp, vp, sz, vp, ctypes.c_int, ctypes.POINTER(PPOGlobal), vp]),
        "gs_ppo_update_workspace_bytes": (sz, [MlpDims, i64, i64]),
        "gs_ppo_graph_cache_info": (ctypes.c_int, [vp, vp]),
        "gs_ppo_exchange_inside_bwd": (ctypes.c_int, [vp, MlpDims, ctypes.c_int64, vp]),
        "gs_cnn_param_count": (i64, [CnnDims]),
        "gs_cnn_workspace_bytes": (sz, [CnnDims, i64]),
        "gs_cnn_workspace_hidden_offset": (i64, [CnnDims, i64]),
        "gs_cnn_workspace_act_offset": (i64, [CnnDims, i64, ctypes.c_int]),
        "gs_cnn_policy_act": (ctypes.c_int, [vp, CnnDims, vp, i64, ctypes.c_int, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "gs_cnn_ppo_loss": (ctypes.c_int, [vp, CnnDims, PPOHparams, RolloutViewU8, vp, i64, vp, vp, vp, vp]),
        "gs_cnn_ppo_update": (ctypes.c_int, [vp, vp, vp, vp, CnnDims, PPOHparams, RolloutViewU8, vp, i64, i64, i64,
                                             vp, vp, vp, vp, vp]),
        "gs_cnn_ppo_update_global": (ctypes.c_int, [vp, vp, vp, vp, CnnDims, PPOHparams, RolloutViewU8, vp, vp, i64, i64,
                                                    i64, vp, vp, vp, vp, ctypes.POINTER(PPOGlobal), vp]),
        "gs_gemm_f32": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, i64, i64, i64, vp, i64, vp, i64, vp, i64,
                                       f32, vp, ctypes.c_int, vp]),
        "gs_fc_gemm": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, i64, i64, i64, vp, i64, vp, i64, vp, i64, vp, vp,
                                      vp]),
        **{f"gs_{x}_reset": (ctypes.c_int, g + reset_tail) for x, g in groups.items() if x not in ("bandit", "tabular")},
        "gs_bandit_reset": (ctypes.c_int, groups["bandit"] + [i64, vp]),               # no reset draw: no seed, no offset
        "gs_tabular_reset": (ctypes.c_int, plain + [TabularSpec, vp] + reset_tail),    # spec, starts: none of the tables
        **{f"gs_{x}_step": (ctypes.c_int, g + step_tail) for x, g in groups.items()},
        # the one-launch rollouts; a one-hidden-layer policy's entry takes its two-hidden-layer sibling's
        # list (the same object), and the tabular env has only that one
        **{f"gs_rollout_{x}": (ctypes.c_int, a) for x, a in rollouts.items() if x != "tabular"},
        **{f"gs_rollout1_{x}": (ctypes.c_int, a) for x, a in rollouts.items()},
        "gs_rollout1_supported": (ctypes.c_int, [MlpDims, vp]),
        "gs_atari_preprocess": (ctypes.c_int, [vp, i64, i32, i32, vp, vp]),
        "gs_atari_render": (ctypes.c_int, [vp, i64, u64, i64, u64, vp]),
        "gs_atari_env_reset": (ctypes.c_int, [vp, vp, vp, vp, i64, i32, i32, i32, i32, u64, i64, vp]),
        "gs_atari_env_step": (ctypes.c_int, [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, u64, i64, u64, vp, vp, vp,
                                             vp, vp, vp, vp, vp]),
        "gs_comm_unique_id": (ctypes.c_int, [vp]),
        "gs_comm_init": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]),
        "gs_comm_xgmi_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, i64, vp, ctypes.POINTER(vp)]),
        "gs_comm_xgmi_connect": (ctypes.c_int, [vp, vp]),
        "gs_comm_status": (ctypes.c_int, [vp]),
        "gs_comm_error_record": (ctypes.c_int, [vp, vp, vp, vp, vp]),
        "gs_comm_xgmi_set_colocation": (ctypes.c_int, [vp, ctypes.c_int]),
        "gs_comm_xgmi_set_bwd_exchange": (ctypes.c_int, [vp, ctypes.c_int]),
        "gs_comm_xgmi_reset": (ctypes.c_int, [vp]),
        "gs_comm_allreduce_mean_f32": (ctypes.c_int, [vp, vp, i64, vp]),
        "gs_comm_allreduce_sum_f64": (ctypes.c_int, [vp, vp, i64, vp]),
        "gs_ppo_global_adv_stats": (ctypes.c_int, [vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp]),
        "gs_ppo_global_records": (ctypes.c_int, [ctypes.POINTER(PPOHparams), i64, i64, vp, vp, vp, vp]),
        "gs_comm_info": (ctypes.c_int, [vp, vp, vp, vp]),
        "gs_comm_destroy": (ctypes.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.gs_abi_version() != GS_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} implements C-ABI version {L.gs_abi_version()}, this binding version "
                          f"{GS_ABI_VERSION}: rebuild the library (__graft_entry__.build())")
    return L, tuple(sig)


lib, EXPORTED = _load()          # the library and the names of every entry declared above


def check(rc: int, what: str = "") -> None:
    """Raise on a non-zero status: ValueError for bad arguments (the reference's error
    type for shape/config problems), GsError for runtime/RCCL failures."""
    if rc == GS_OK:
        return
    msg = (lib.gs_last_error() or b"").decode(errors="replace")
    if rc == GS_E_INVALID:
        raise ValueError(f"{what}: {msg}")
    raise GsError(f"{what} failed ({rc}): {msg}")


def ptr(t) -> int | None:
    """Device/host address of a torch tensor (None passes NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_handle(stream=None) -> int | None:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream
