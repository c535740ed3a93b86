"""ctypes binding of the C ABI in include/susnet.h (libsusnet_hip.so).

The library is the product: there is NO fallback.  If it is missing or does not export every symbol the
header declares, importing this module's `lib()` raises -- loudly.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libsusnet_hip.so"
LIB_PATH = os.environ.get("SUSNET_LIB_PATH", os.path.join(PKG_DIR, LIB_NAME))  # override: A/B experiments only

ABI_VERSION = 8
MAX_AGENTS, MAX_JOBS, MAX_GRID, N_METRICS, N_LIFETIME = 16, 16, 16, 13, 12
DQN_MAX_LEARNERS = 16  # SUSNET_DQN_MAX_LEARNERS
SPATIAL_SWEEP_MAX_LEARNERS = 16  # SUSNET_SPATIAL_SWEEP_MAX_LEARNERS: learners of one susnet_spatial_train_sweep call
MLP_SWEEP_MAX_LEARNERS = 16  # SUSNET_MLP_SWEEP_MAX_LEARNERS: learners of one susnet_mlp_train_sweep call
MLP_MAX_F, MLP_ROW_TILE, MLP_MAX_GRID = 1024, 64, 512  # SUSNET_MLP_*: susnet_mlp_forward's input width cap, rows per tile, grid cap
MLP_MAX_HIDDEN, MLP_MAX_OUT = 256, 32
WINDOW_MAX_T = 8  # susnet_window_push: states per window
# SUSNET_SPATIAL_*: susnet_spatial_forward's bounds (window steps, image size, input channels, convolutions, RNN input width, RNN layers),
# the convolution kernel's images per group and grid cap
SPATIAL_MAX_T, SPATIAL_MAX_N, SPATIAL_MAX_C, SPATIAL_MAX_CONV, SPATIAL_MAX_R, SPATIAL_MAX_RNN_LAYERS = 8, 16, 32, 4, 4096, 4
SPATIAL_CONV_GROUP, SPATIAL_CONV_MAX_GRID = 16, 1024
SPATIAL_TRAIN_MAX_GRID = 256  # SUSNET_SPATIAL_TRAIN_MAX_GRID: workgroups of susnet_spatial_train_step's gradient kernels
SPATIAL_LDS_BYTES = 160 * 1024  # a workgroup's LDS: (rnn_layers + 1) x 64 rows x max(rnn_hidden, head widths) floats must fit

VARIANT_BASE, VARIANT_ITG, VARIANT_TAGGING = 0, 1, 2
RNG_TAPE, RNG_PHILOX = 1, 2
U8, I32, I64, F32, F64 = 0, 1, 2, 3, 4
LAYOUT_AB, LAYOUT_BA = 0, 1
OBS_NONE, OBS_RAW, OBS_FLAT, OBS_PLANES, OBS_PERSP = 0, 1, 2, 3, 4
OBS_PERSP_ROOM, OBS_PERSP_ROOM_MASK = 5, 6  # the Perspective views under the observer's room mask: susnet_featurize only
E_INVALID, E_HIP, E_STATE, E_ACTION_ASSERT, E_ACTION_INDEX, E_TAPE, E_ROW = -1, -2, -3, -4, -5, -6, -7

RECORD_DEFAULT, RECORD_COMPACT = 0, 1
EPISODE_DONE, EPISODE_TRUNCATED = 1, 2  # susnet_episode_record.ended_by bits
OUTCOME_CREW_WON, OUTCOME_IMPOSTER_WON = 1, 2  # susnet_episode_info.outcome bits
FLAT_COMPONENTS = {"onehot_pos": 0, "coord_pos": 1, "alive_crew": 2, "l1_crew": 3, "closest_crew": 4,
                   "walls3x3": 5, "dist_to_imp": 6, "room_loc": 7}
LIFETIME_NAMES = ["episodes", "crew_won", "imposter_won", "truncated", "imp_killed_crew", "completed_jobs",
                  "sabotaged_jobs", "imp_voted_out", "crew_voted_out", "episode_steps", "env_steps", "reserved"]

# every symbol include/susnet.h declares
EXPORTS = [
    "susnet_abi_version", "susnet_last_error", "susnet_create", "susnet_destroy", "susnet_get_layout",
    "susnet_bind_state", "susnet_bind_tape", "susnet_seed", "susnet_tick", "susnet_reset", "susnet_sample_actions", "susnet_policy_actions", "susnet_agent_policy_actions", "susnet_qnet_packed_floats", "susnet_qnet_pack", "susnet_qnet_forward", "susnet_mlp_forward", "susnet_spatial_forward", "susnet_spatial_forward_dropout", "susnet_spatial_act_dropout_mask", "susnet_window_push", "susnet_state_window_push", "susnet_step", "susnet_policy_step", "susnet_qnet_policy_step", "susnet_qnet_policy_rollout",
    "susnet_rollout", "susnet_record_layout", "susnet_record_layout_of", "susnet_set_launch_limit", "susnet_observe", "susnet_obs_size", "susnet_featurize", "susnet_export_state", "susnet_import_state",
    "susnet_reduce_lifetime", "susnet_device_tick", "susnet_poll_errors", "susnet_ring_append", "susnet_scent",
    "susnet_dqn_workspace_bytes", "susnet_dqn_train_step", "susnet_dqn_train_sweep", "susnet_mlp_train_workspace_bytes", "susnet_mlp_train_step", "susnet_mlp_train_sweep", "susnet_spatial_train_workspace_bytes", "susnet_spatial_train_step", "susnet_spatial_train_dropout_workspace_bytes", "susnet_spatial_train_step_dropout", "susnet_rnn_dropout_mask", "susnet_spatial_train_sweep_table_bytes", "susnet_spatial_train_sweep", "susnet_episode_stats_bytes", "susnet_episode_stats",
]


class Config(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("abi_version", C.c_uint32), ("variant", C.c_int32), ("batch", C.c_int32),
        ("n_imposters", C.c_int32), ("n_crew", C.c_int32), ("n_jobs", C.c_int32), ("grid_n", C.c_int32),
        ("grid_rows", C.c_uint16 * MAX_GRID),
        ("kill_reward", C.c_double), ("complete_job_reward", C.c_double), ("sabotage_reward", C.c_double),
        ("time_step_reward", C.c_double), ("game_end_reward", C.c_double), ("dead_penalty", C.c_double),
        ("vote_reward", C.c_double),
        ("max_time_steps", C.c_int32), ("is_action_order_random", C.c_int32), ("shuffle_imposter_index", C.c_int32),
        ("tag_reset_interval", C.c_int32), ("auto_reset", C.c_int32), ("rng_mode", C.c_int32),
        ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class Layout(C.Structure):
    _fields_ = [
        ("state_bytes", C.c_uint64), ("state_align", C.c_uint64), ("batch_padded", C.c_int32), ("n_agents", C.c_int32),
        ("n_actions_imposter", C.c_int32), ("n_actions_crew", C.c_int32), ("action_space_n", C.c_int32),
        ("obs_raw_size", C.c_int32), ("envs_per_wave", C.c_int32), ("test_overrides", C.c_uint32),
    ]


class ObsSpec(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("dtype", C.c_int32), ("n_components", C.c_int32), ("components", C.c_int32 * 16),
        ("out", C.c_void_p), ("out2", C.c_void_p),
    ]


class StepIO(C.Structure):
    _fields_ = [
        ("actions", C.c_void_p), ("actions_dtype", C.c_int32), ("actions_layout", C.c_int32),
        ("rewards", C.c_void_p), ("rewards_dtype", C.c_int32), ("rewards_layout", C.c_int32),
        ("done", C.c_void_p), ("truncated", C.c_void_p), ("obs", C.POINTER(ObsSpec)), ("term_obs", C.c_void_p), ("roles", C.c_void_p),
        ("ep_info", C.c_void_p),
    ]


class RolloutIO(C.Structure):
    _fields_ = [
        ("n_ticks", C.c_int32), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("done", C.c_void_p),
        ("truncated", C.c_void_p), ("obs", C.POINTER(ObsSpec)), ("record", C.c_void_p),
        ("term_obs", C.c_void_p), ("roles", C.c_void_p), ("record_format", C.c_int32),
    ]


class RingIO(C.Structure):
    _fields_ = [
        ("n_ticks", C.c_int32), ("trajectory_size", C.c_int32), ("actions", C.c_void_p), ("rewards", C.c_void_p),
        ("done", C.c_void_p), ("truncated", C.c_void_p), ("obs", C.c_void_p), ("term_obs", C.c_void_p), ("roles", C.c_void_p),
        ("window", C.c_void_p), ("max_size", C.c_int64), ("idx", C.c_int64), ("states", C.c_void_p), ("next_states", C.c_void_p),
        ("ring_actions", C.c_void_p), ("ring_rewards", C.c_void_p), ("ring_dones", C.c_void_p), ("ring_imposters", C.c_void_p),
        ("record", C.c_void_p), ("record_format", C.c_int32),
    ]


class FeedIO(C.Structure):
    _fields_ = [("actions", C.c_void_p), ("rewards", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p), ("obs", C.c_void_p),
                ("term_obs", C.c_void_p), ("roles", C.c_void_p), ("q", C.c_void_p), ("ep_info", C.c_void_p)]


class PolicyOpts(C.Structure):
    _fields_ = [("epsilon", C.c_float), ("mask_dead", C.c_int32), ("crew_packed", C.c_void_p), ("crew_dims", C.POINTER(C.c_int32)),
                ("crew_n_dims", C.c_int32), ("pad_", C.c_int32), ("crew_q_out", C.c_void_p)]


class MlpIO(C.Structure):
    _fields_ = [("n_dims", C.c_int32), ("dims", C.c_int32 * 8), ("weight", C.c_void_p * 7), ("bias", C.c_void_p * 7), ("slope", C.c_void_p * 6),
                ("rows", C.c_void_p), ("n", C.c_int64), ("q_out", C.c_void_p)]


class SpatialIO(C.Structure):
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("n_conv", C.c_int32), ("k", C.c_int32),
                ("conv_out", C.c_int32 * 4), ("conv_stride", C.c_int32 * 4), ("conv_padding", C.c_int32 * 4), ("conv_dilation", C.c_int32 * 4),
                ("conv_weight", C.c_void_p * 4), ("conv_bias", C.c_void_p * 4), ("Fn", C.c_int32), ("rnn_layers", C.c_int32), ("rnn_hidden", C.c_int32),
                ("w_ih", C.c_void_p * 4), ("w_hh", C.c_void_p * 4), ("b_ih", C.c_void_p * 4), ("b_hh", C.c_void_p * 4),
                ("n_dims", C.c_int32), ("dims", C.c_int32 * 8), ("weight", C.c_void_p * 7), ("bias", C.c_void_p * 7), ("slope", C.c_void_p * 6),
                ("spatial", C.c_void_p), ("spatial_stride", C.c_int64 * 3), ("non_spatial", C.c_void_p), ("non_spatial_stride", C.c_int64 * 3),
                ("agents", C.c_int32), ("n", C.c_int64), ("rnn_in", C.c_void_p), ("q_out", C.c_void_p)]


class WindowIO(C.Structure):
    _fields_ = [("fresh", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p), ("src", C.c_void_p), ("dst", C.c_void_p),
                ("T", C.c_int32), ("F", C.c_int32), ("n", C.c_int64)]


class DqnTeam(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("n_dims", C.c_int32), ("dims", C.c_int32 * 8), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("params", C.c_void_p), ("target_params", C.c_void_p), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("packed", C.c_void_p)]


class DqnIO(C.Structure):
    _fields_ = [("n_components", C.c_int32), ("components", C.c_int32 * 16), ("trajectory_size", C.c_int32), ("states", C.c_void_p),
                ("next_states", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p), ("imposters", C.c_void_p),
                ("max_size", C.c_int64), ("indices", C.c_void_p), ("n", C.c_int64), ("gamma", C.c_double), ("team", DqnTeam * 2),
                ("losses_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class MlpTrainIO(C.Structure):
    _fields_ = [("feat", C.c_void_p), ("next_feat", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
                ("imposters", C.c_void_p), ("max_size", C.c_int64), ("indices", C.c_void_p), ("n", C.c_int64), ("gamma", C.c_double),
                ("team", DqnTeam * 2), ("losses_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class SpatialNet(C.Structure):
    _fields_ = [("T", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("Fn", C.c_int32), ("n_conv", C.c_int32), ("k", C.c_int32),
                ("conv_out", C.c_int32 * 4), ("conv_stride", C.c_int32 * 4), ("conv_padding", C.c_int32 * 4), ("conv_dilation", C.c_int32 * 4),
                ("rnn_layers", C.c_int32), ("rnn_hidden", C.c_int32)]


class SpatialTrainIO(C.Structure):
    _fields_ = [("net", SpatialNet * 2), ("team", DqnTeam * 2), ("spatial", C.c_void_p), ("next_spatial", C.c_void_p),
                ("spatial_stride", C.c_int64 * 3), ("non_spatial", C.c_void_p), ("next_non_spatial", C.c_void_p),
                ("non_spatial_stride", C.c_int64 * 3), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
                ("imposters", C.c_void_p), ("max_size", C.c_int64), ("indices", C.c_void_p), ("n", C.c_int64), ("gamma", C.c_double),
                ("losses_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64)]


class RnnDropout(C.Structure):  # susnet_rnn_dropout: p[0] the online network, p[1] the target network
    _fields_ = [("p", C.c_float * 2), ("seed", C.c_uint64), ("offset", C.c_uint64), ("row_base", C.c_int64)]


class EpisodeRecord(C.Structure):
    _fields_ = [("imposter_return", C.c_double), ("crew_return", C.c_double), ("tick", C.c_int64), ("env", C.c_int32), ("length", C.c_int32),
                ("ended_by", C.c_int32), ("reserved", C.c_int32)]


class EpisodeIO(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("reserved", C.c_int32), ("rewards", C.c_void_p), ("done", C.c_void_p), ("truncated", C.c_void_p),
                ("roles", C.c_void_p), ("gamma", C.c_double), ("tick_base", C.c_int64), ("carry", C.c_void_p), ("carry_bytes", C.c_uint64),
                ("log", C.c_void_p), ("capacity", C.c_int64), ("count", C.c_void_p), ("dropped", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_uint64), ("info", C.c_void_p), ("info_log", C.c_void_p)]


class EpisodeInfo(C.Structure):
    _fields_ = [("time_steps", C.c_uint32), ("completed_jobs", C.c_uint32), ("sabotaged_jobs", C.c_uint32), ("imp_killed_crew", C.c_uint8),
                ("imp_voted_out", C.c_uint8), ("crew_voted_out", C.c_uint8), ("outcome", C.c_uint8)]


class RecordLayout(C.Structure):
    _fields_ = [("record_bytes", C.c_int32), ("off_rewards", C.c_int32), ("off_actions", C.c_int32), ("off_done", C.c_int32),
                ("off_truncated", C.c_int32), ("off_obs", C.c_int32), ("planar", C.c_int32), ("n_obs_segments", C.c_int32),
                ("obs_segments", (C.c_int32 * 2) * 4), ("flags_packed", C.c_int32)]


class StateView(C.Structure):
    _fields_ = [
        ("agent_positions", C.c_void_p), ("alive_agents", C.c_void_p), ("imposter_mask", C.c_void_p),
        ("job_positions", C.c_void_p), ("completed_jobs", C.c_void_p), ("used_tag_actions", C.c_void_p),
        ("tag_counts", C.c_void_p), ("tag_reset_timer", C.c_void_p), ("t", C.c_void_p), ("metrics", C.c_void_p),
        ("rng_cursor", C.c_void_p), ("lifetime", C.c_void_p), ("episode_index", C.c_void_p),
    ]


class SusnetError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsusnet_hip: {msg} (code {code})")
        self.code = code


_lib = None


def _assert_single_hip_runtime():
    """torch ships its own libamdhip64; ours must resolve to the SAME loaded runtime or stream handles and
    device pointers would belong to different runtimes."""
    seen = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    seen.add(line.split()[-1])
    except OSError:
        return
    if len(seen) > 1:
        raise ImportError(f"two HIP runtimes mapped in one process: {sorted(seen)}; import torch before sus-net_amd")


def lib():
    """Load libsusnet_hip.so (built by `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is the product and there is no CPU fallback. "
            "Build it with `python -m build_hip` or `__graft_entry__.build()` (needs hipcc, gfx950).")
    import torch  # noqa: F401  (loads torch's libamdhip64 first so ours binds to the same runtime)

    L = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS if not hasattr(L, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} does not export {missing}")
    _assert_single_hip_runtime()
    P = C.POINTER
    L.susnet_abi_version.restype = C.c_int
    L.susnet_last_error.restype = C.c_char_p
    L.susnet_create.argtypes = [P(Config), P(C.c_void_p)]
    L.susnet_destroy.argtypes = [C.c_void_p]
    L.susnet_destroy.restype = None
    L.susnet_get_layout.argtypes = [C.c_void_p, P(Layout)]
    L.susnet_bind_state.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.susnet_bind_tape.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.susnet_seed.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.susnet_tick.argtypes = [C.c_void_p, P(C.c_uint64), P(C.c_uint64), C.c_void_p]
    L.susnet_reset.argtypes = [C.c_void_p, C.c_void_p, P(ObsSpec), C.c_void_p]
    L.susnet_sample_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.susnet_step.argtypes = [C.c_void_p, P(StepIO), C.c_void_p]
    L.susnet_rollout.argtypes = [C.c_void_p, P(RolloutIO), C.c_void_p]
    L.susnet_policy_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(PolicyOpts), P(StepIO), C.c_void_p]
    L.susnet_qnet_policy_step.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, P(PolicyOpts), P(StepIO),
                                          C.c_void_p]
    L.susnet_qnet_policy_rollout.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32, C.c_void_p, P(PolicyOpts), P(FeedIO), C.c_int32,
                                             C.c_void_p]
    L.susnet_record_layout_of.argtypes = [C.c_void_p, C.c_int32, P(RecordLayout)]
    L.susnet_policy_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(PolicyOpts), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.susnet_agent_policy_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(PolicyOpts), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.susnet_qnet_packed_floats.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32]
    L.susnet_qnet_pack.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32, P(C.c_void_p), P(C.c_void_p), C.c_void_p, C.c_void_p]
    L.susnet_qnet_forward.argtypes = [C.c_void_p, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.susnet_mlp_forward.argtypes = [C.c_void_p, P(MlpIO), C.c_void_p]
    L.susnet_spatial_forward.argtypes = [C.c_void_p, P(SpatialIO), C.c_void_p]
    L.susnet_window_push.argtypes = [C.c_void_p, P(WindowIO), C.c_void_p]
    L.susnet_state_window_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.susnet_record_layout.argtypes = [C.c_void_p, P(RecordLayout)]
    L.susnet_set_launch_limit.argtypes = [C.c_void_p, C.c_uint64]
    L.susnet_observe.argtypes = [C.c_void_p, P(ObsSpec), C.c_void_p]
    L.susnet_obs_size.argtypes = [C.c_void_p, P(ObsSpec), P(C.c_int32), P(C.c_int32)]
    L.susnet_featurize.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, P(ObsSpec), C.c_void_p]
    L.susnet_export_state.argtypes = [C.c_void_p, P(StateView), C.c_void_p]
    L.susnet_import_state.argtypes = [C.c_void_p, P(StateView), C.c_void_p]
    L.susnet_reduce_lifetime.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.susnet_device_tick.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.susnet_poll_errors.argtypes = [C.c_void_p, P(C.c_uint32), C.c_void_p]
    L.susnet_ring_append.argtypes = [C.c_void_p, P(RingIO), C.c_void_p]
    L.susnet_scent.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    L.susnet_dqn_workspace_bytes.argtypes = [C.c_void_p, P(DqnIO), P(C.c_uint64)]
    L.susnet_dqn_train_step.argtypes = [C.c_void_p, P(DqnIO), C.c_void_p]
    L.susnet_dqn_train_sweep.argtypes = [P(C.c_void_p), P(DqnIO), C.c_int32, C.c_void_p]
    L.susnet_mlp_train_workspace_bytes.argtypes = [C.c_void_p, P(MlpTrainIO), P(C.c_uint64)]
    L.susnet_mlp_train_step.argtypes = [C.c_void_p, P(MlpTrainIO), C.c_void_p]
    L.susnet_mlp_train_sweep.argtypes = [P(C.c_void_p), P(MlpTrainIO), C.c_int32, C.c_void_p]
    L.susnet_spatial_train_workspace_bytes.argtypes = [C.c_void_p, P(SpatialTrainIO), P(C.c_uint64)]
    L.susnet_spatial_train_step.argtypes = [C.c_void_p, P(SpatialTrainIO), C.c_void_p]
    L.susnet_spatial_train_dropout_workspace_bytes.argtypes = [C.c_void_p, P(SpatialTrainIO), P(C.c_uint64)]
    L.susnet_spatial_train_step_dropout.argtypes = [C.c_void_p, P(SpatialTrainIO), P(RnnDropout), C.c_void_p]
    L.susnet_rnn_dropout_mask.argtypes = [C.c_void_p, P(RnnDropout), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p]
    L.susnet_spatial_forward_dropout.argtypes = [C.c_void_p, P(SpatialIO), P(RnnDropout), C.c_int32, C.c_void_p]
    L.susnet_spatial_act_dropout_mask.argtypes = [C.c_void_p, P(RnnDropout), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p]
    L.susnet_spatial_train_sweep_table_bytes.argtypes = [C.c_int32, P(C.c_uint64)]
    L.susnet_spatial_train_sweep.argtypes = [P(C.c_void_p), P(SpatialTrainIO), P(RnnDropout), C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.susnet_episode_stats_bytes.argtypes = [C.c_void_p, C.c_int32, P(C.c_uint64), P(C.c_uint64)]
    L.susnet_episode_stats.argtypes = [C.c_void_p, P(EpisodeIO), C.c_void_p]
    for name in EXPORTS:
        if name not in ("susnet_last_error", "susnet_destroy"):
            getattr(L, name).restype = C.c_int
    L.susnet_qnet_packed_floats.restype = C.c_int64
    if L.susnet_abi_version() != ABI_VERSION:
        raise ImportError(f"ABI mismatch: library {L.susnet_abi_version()} vs binding {ABI_VERSION}")
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise SusnetError(rc, lib().susnet_last_error().decode())
