"""ctypes mirror of ``include/wedm_hip.h`` (ABI version = ``ABI_VERSION`` below, cross-checked against the library by the loader).

Pure declarations — no library is loaded here, so this module imports on a
GPU-less box.  Field order and types must match the header exactly; the loader
(`sparc_amd._lib`) cross-checks ``sizeof(wedm_params)`` against the library.
"""
from __future__ import annotations

import ctypes as C
import enum

ABI_VERSION = 4
MAX_MODE = 19


def t_quads(n_seg_max: int) -> int:
    """``WEDM_T_QUADS``: 16-byte words (rows of the quad-interleaved T block) a wire of n_seg_max segments occupies."""
    return (int(n_seg_max) + 3) >> 2


# status codes -----------------------------------------------------------------
OK = 0
ERR_BAD_ARG = -1
ERR_NOT_BOUND = -2
ERR_HIP = -3
ERR_NO_DEVICE = -4
ERR_BAD_MODE = -5
ERR_UNSUPPORTED = -6

STATUS_NAMES = {
    OK: "WEDM_OK",
    ERR_BAD_ARG: "WEDM_ERR_BAD_ARG",
    ERR_NOT_BOUND: "WEDM_ERR_NOT_BOUND",
    ERR_HIP: "WEDM_ERR_HIP",
    ERR_NO_DEVICE: "WEDM_ERR_NO_DEVICE",
    ERR_BAD_MODE: "WEDM_ERR_BAD_MODE",
    ERR_UNSUPPORTED: "WEDM_ERR_UNSUPPORTED",
}


class F64(enum.IntEnum):
    """Rows of the float64 state block (``enum wedm_f64_field``)."""

    WORKPIECE_POS = 0
    WIRE_POS = 1
    WIRE_VEL = 2
    PREV_ACCEL = 3
    DEBRIS_VOLUME = 4
    DEBRIS_DENSITY = 5
    FLOW = 6
    LAST_GAP = 7
    LAST_DENSITY = 8
    WIRE_LAST_FLOW = 9
    VOLTAGE = 10
    CURRENT = 11
    SPARK_Y = 12
    LAST_CRATER = 13
    CAVITY = 14
    TARGET_DELTA = 15
    TARGET_VOLTAGE = 16
    ON_TIME = 17
    OFF_TIME = 18
    TARGET_POS = 19
    UNWIND_VEL = 20
    H_BASE = 21
    H_ZONE = 22
    TMAX = 23
    VOLT_ACC = 24
    VOLT_SUM = 25


F64_COUNT = 26


class I32(enum.IntEnum):
    """Rows of the int32 state block (``enum wedm_i32_field``)."""

    TIME = 0
    SINCE_SERVO = 1
    SINCE_OPEN_V = 2
    SINCE_IGNITION = 3
    SINCE_SPARK_END = 4
    SPARK_DUR = 5
    RANDOM_SHORT_REM = 6
    DEBRIS_SHORT_REM = 7
    TIME_CRITICAL = 8
    CURRENT_MODE = 9
    EPISODE = 10
    KEY_LO = 11
    KEY_HI = 12
    SPARK_COUNT = 13
    TIME_HI = 14


I32_COUNT = 15


class I8(enum.IntEnum):
    """Rows of the int8 state block (``enum wedm_i8_field``)."""

    SPARK_STATE = 0
    IS_SHORT = 1
    WIRE_BROKEN = 2
    TARGET_REACHED = 3
    DONE = 4
    CTRL_STEP = 5
    ERROR = 6
    MODE_CACHED = 7


I8_COUNT = 8


class STAT(enum.IntEnum):
    """Rows of the optional statistics block (``enum wedm_stat_field``)."""

    CRATER_SUM = 0
    CRATER_SUMSQ = 1
    CRATER_MIN = 2
    CRATER_MAX = 3


STAT_COUNT = 4


class PULSE(enum.IntEnum):
    """Rows of the optional pulse-statistics block (``enum wedm_pulse_field``, int32)."""

    SPARK_ACC = 0
    SHORT_ACC = 1
    SHORT_STEPS_ACC = 2
    SPARK_LAST = 3
    SHORT_LAST = 4
    SHORT_STEPS_LAST = 5


PULSE_COUNT = 6
# obs columns 8-10 of an environment built with pulse_stats=True (the published rows, float32)
PULSE_OBS_NAMES = ("spark_pulses", "short_pulses", "short_steps")


class SIG(enum.IntEnum):
    """Rows of the optional signal-statistics block (``enum wedm_sig_field``, float64)."""

    SAMPLES_ACC = 0
    CURRENT_ACC = 1
    ENERGY_ACC = 2
    GAP_ACC = 3
    GAP_MIN_ACC = 4
    TMAX_PEAK_ACC = 5
    SAMPLES_LAST = 6
    CURRENT_LAST = 7
    ENERGY_LAST = 8
    GAP_LAST = 9
    GAP_MIN_LAST = 10
    TMAX_PEAK_LAST = 11


SIG_COUNT = 12
# obs columns of an environment built with signal_stats=True: five published rows as float32 (raw sums over the interval,
# not means), at columns 8-12, or 11-15 behind the pulse columns
SIGNAL_OBS_NAMES = ("current_sum", "energy_sum", "gap_sum", "gap_min", "tmax_peak")


class ENVP(enum.IntEnum):
    """Rows of the optional per-environment physics block (``enum wedm_envp_field``, float64)."""

    BASE_CRITICAL_DENSITY = 0
    GAP_COEFFICIENT = 1
    MAX_CRITICAL_DENSITY = 2
    HARD_SHORT_GAP = 3
    SIGMOID_STEEPNESS = 4
    SPARK_VOLTAGE_FACTOR = 5
    DEBRIS_REMOVAL_PER_US = 6
    DIELECTRIC_TEMPERATURE = 7
    PLASMA_EFFICIENCY = 8
    BASE_CONVECTION = 9
    DAMPING_COEFF = 10
    STIFFNESS_COEFF = 11
    OMEGA_N = 12
    MAX_ACCELERATION = 13
    MAX_JERK_DT = 14
    MAX_SPEED = 15


ENVP_COUNT = 16


class WMAT(enum.IntEnum):
    """Rows of the optional per-environment wire-material block (``enum wedm_wmat_field``, float64)."""

    RHO_ELEC = 0
    ALPHA_RHO = 1
    RHO_C = 2
    CRITICAL_TEMPERATURE = 3
    BREAKING_TEMPERATURE = 4


WMAT_COUNT = 5


class GF64(enum.IntEnum):
    """Rows of the per-environment geometry float64 block."""

    HEIGHT = 0
    KERF_BASE = 1
    CAVITY_COEFF = 2
    K_COND = 3
    TUF = 4
    A_SURF = 5
    S_AREA = 6
    JOULE_GEOM = 7


GEOM_F64_COUNT = 8


class GI32(enum.IntEnum):
    """Rows of the per-environment geometry int32 block."""

    N_SEG = 0
    ZONE_START = 1
    AZ_START = 2
    AZ_END = 3
    CONTACT_BOTTOM = 4
    CONTACT_TOP = 5


GEOM_I32_COUNT = 6

REPLAY_SLOTS = 5  # enum wedm_replay_slot: debris roll, random-short roll, ignition roll, spark y [mm], crater volume [um^3]


class KERNEL(enum.IntEnum):
    """The kernel numbers of wedm_set_kernel (`enum Kernel` of sparc_amd/csrc/wedm_kernels.hip)."""
    AUTO = 0
    GLOBAL = 1
    LANES_PK = 2
    FUSED = 3
    PACKED = 4
    SPLIT = 5
    STREAM = 6
    REGS = 7
    WIDE = 8
    SERVED = 9
    LANES = 10
    LANES_SERVED = 11
    REGS_SERVED = 12


class FORM(enum.IntFlag):
    """The form bits of a step kernel's instantiation (the `F_*` enum of sparc_amd/csrc/wedm_device.h), as
    wedm_debug_registry and wedm_debug_last_form report them."""
    TRACE = 1 << 0
    F64 = 1 << 1
    REPLAY = 1 << 2
    PULSE = 1 << 3
    ENVP = 1 << 4
    MAT = 1 << 5
    FROZEN_OK = 1 << 6
    N1 = 1 << 7
    EXTRA = 1 << 8
    CUT = 1 << 9
    ONE = 1 << 10
    CMAX104 = 1 << 11
    MINB2 = 1 << 12
    SIG = 1 << 13


OBS_DIM = 8
OBS_NAMES = ("gap", "wire_velocity", "voltage", "current", "spark_state", "debris_density", "flow_rate", "tmax")

_d = C.c_double
_i = C.c_int32
_tab = _d * (MAX_MODE + 1)
_itab = _i * (MAX_MODE + 1)


class Params(C.Structure):
    """``struct wedm_params``."""

    _fields_ = [
        ("servo_interval", _i), ("dt_us", _i), ("control_mode", _i), ("per_env_geometry", _i),
        ("initial_gap", _d), ("target_cutting_distance", _d),
        ("n_seg", _i), ("zone_start", _i), ("az_start", _i), ("az_end", _i),
        ("contact_bottom", _i), ("contact_top", _i),
        ("workpiece_height", _d), ("kerf_base", _d), ("cavity_coeff", _d),
        ("k_cond", _d), ("tuf", _d), ("a_surf", _d), ("s_area", _d), ("joule_geom", _d),
        ("segment_len", _d),
        ("spool_T", _d), ("temp_ref", _d), ("rho_elec", _d), ("alpha_rho", _d), ("rho_c", _d),
        ("plasma_efficiency", _d), ("base_convection", _d),
        ("convection_velocity_factor", _d), ("convection_flow_enhancement", _d),
        ("critical_temperature", _d), ("breaking_temperature", _d), ("dielectric_temperature", _d),
        ("base_critical_density", _d), ("gap_coefficient", _d), ("max_critical_density", _d),
        ("hard_short_gap", _d), ("sigmoid_steepness", _d),
        ("debris_short_duration", _i), ("random_short_duration", _i),
        ("random_short_min_gap", _d), ("random_short_max_gap", _d), ("random_short_max_probability", _d),
        ("ignition_a", _d), ("ignition_b", _d), ("ignition_c", _d), ("ln2", _d),
        ("default_target_voltage", _d), ("default_on_time", _d), ("default_off_time", _d),
        ("default_current", _d), ("spark_voltage_factor", _d),
        ("reference_gap", _d), ("debris_obstruction_coeff", _d), ("debris_removal_per_us", _d),
        ("dt_s", _d), ("damping_coeff", _d), ("stiffness_coeff", _d), ("omega_n", _d),
        ("max_acceleration", _d), ("max_jerk_dt", _d), ("max_speed", _d),
        ("mode_current", _tab), ("crater_mean", _tab), ("crater_std", _tab), ("crater_depth", _tab),
        ("crater_valid", _itab),
        ("env_id_offset", C.c_uint32), ("obs_dim", _i),
        ("disable_ignition", _i), ("autoreset", _i), ("reward_mode", _i), ("stencil_mode", _i),
        ("reset_semantics", _i), ("keep_stepping_terminated", _i),
        ("reward_break_penalty", _d),
    ]


class StatePtrs(C.Structure):
    """``struct wedm_state_ptrs``."""

    _fields_ = [
        ("f64", C.c_void_p), ("i32", C.c_void_p), ("i8", C.c_void_p), ("T", C.c_void_p),
        ("obs", C.c_void_p), ("stride", C.c_int64), ("stats", C.c_void_p), ("reward", C.c_void_p),
        ("crater_log", C.c_void_p), ("crater_log_capacity", C.c_int64),
    ]


class GeomPtrs(C.Structure):
    """``struct wedm_geom_ptrs``."""

    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


class ActionPtrs(C.Structure):
    """``struct wedm_action_ptrs``."""

    _fields_ = [
        ("servo", C.c_void_p), ("target_voltage", C.c_void_p), ("on_time", C.c_void_p),
        ("off_time", C.c_void_p), ("current_mode", C.c_void_p),
    ]


class TraceDesc(C.Structure):
    """``struct wedm_trace_desc``."""

    _fields_ = [
        ("f64", C.c_void_p), ("i32", C.c_void_p), ("i8", C.c_void_p), ("T", C.c_void_p),
        ("f64_mask", C.c_uint32), ("i32_mask", C.c_uint32), ("i8_mask", C.c_uint32),
        ("env_lo", C.c_int32), ("env_count", C.c_int32), ("every", C.c_int32), ("capacity", C.c_int32),
        ("reserved0", C.c_int32),
    ]


COPY_MAX_PLANES = 16  # WEDM_COPY_MAX_PLANES


class CopyPlane(C.Structure):
    """``struct wedm_copy_plane``: one block on both sides of `wedm_copy_columns` (strides in elements)."""

    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("elem_bytes", C.c_int32),
        ("src_stride", C.c_int64), ("dst_stride", C.c_int64), ("src_cols", C.c_int32), ("dst_cols", C.c_int32),
    ]


PROFILE_MAX_BINS = 64  # WEDM_PROFILE_MAX_BINS


class PR(enum.IntEnum):
    """``enum wedm_profile_field``: the fixed rows of a wire profile; ``bins`` rows BIN_MAX and ``bins`` rows BIN_MEAN follow."""

    ZONE_MEAN = 0
    WIRE_MEAN = 1
    WIRE_MAX = 2
    HOT_CELL = 3


PR_FIXED = 4


def profile_rows(bins: int) -> int:
    """``WEDM_PROFILE_ROWS``."""
    return PR_FIXED + 2 * int(bins)


class ProfileDesc(C.Structure):
    """``struct wedm_profile_desc``: what `wedm_wire_profile` reads and where it writes (strides in elements)."""

    _fields_ = [
        ("T", C.c_void_p), ("stride", C.c_int64), ("num_envs", C.c_int32), ("n_seg_max", C.c_int32),
        ("n_seg", C.c_int32), ("az_start", C.c_int32), ("az_end", C.c_int32),
        ("geom_i32", C.c_void_p), ("bins", C.c_int32), ("out", C.c_void_p), ("out_stride", C.c_int64),
        ("out_cols", C.c_int32),
    ]


# `wedm_normalize` (sparc_amd.normalize): C = D + 1 columns at most, tiles of the partials workspace at most, environments
# per tile; enum wedm_norm_flag; the rows of a moments block (enum wedm_norm_moment)
NORM_MAX_COLUMNS = 160  # WEDM_NORM_MAX_COLUMNS
NORM_MAX_TILES = 4096   # WEDM_NORM_MAX_TILES
NORM_TILE = 256         # WEDM_NORM_TILE
NORM_UPDATE, NORM_STEP, NORM_REDUCE, NORM_APPLY = 1, 2, 4, 8
NM_COUNT, NM_MEAN, NM_M2, NORM_MOMENTS = 0, 1, 2, 3


class NormPlane(C.Structure):
    """``struct wedm_norm_plane``: one struct-of-arrays source block of `wedm_normalize` (stride in elements)."""

    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_int32), ("reserved", C.c_int32), ("stride", C.c_int64)]


class NormDesc(C.Structure):
    """``struct wedm_norm_desc``: what `wedm_normalize` reads and where it writes."""

    _fields_ = [
        ("plane", NormPlane * 2),
        ("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("mask", C.c_void_p), ("skip", C.c_void_p),
        ("obs_out", C.c_void_p), ("reward_out", C.c_void_p),
        ("ret", C.c_void_p), ("ep_return", C.c_void_p), ("last_return", C.c_void_p), ("ep_length", C.c_void_p),
        ("last_length", C.c_void_p), ("ep_count", C.c_void_p), ("finished", C.c_void_p),
        ("stats_in", C.c_void_p), ("stats_out", C.c_void_p), ("partials", C.c_void_p),
        ("tile_offset", C.c_int32), ("n_tiles_total", C.c_int32),
        ("gamma", C.c_double), ("eps", C.c_double), ("clip_obs", C.c_double), ("clip_reward", C.c_double),
        ("flags", C.c_int32), ("num_envs", C.c_int32),
    ]


GAE_SKIP_AFTER_DONE, GAE_NORMALIZE, GAE_SCAN, GAE_APPLY = 1, 2, 4, 8  # enum wedm_gae_flag
GAE_MAX_STEPS = 65536  # WEDM_GAE_MAX_STEPS


class GaeDesc(C.Structure):
    """``struct wedm_gae_desc``: what `wedm_gae` reads and where it writes (strides in elements; ``lam``: lambda)."""

    _fields_ = [
        ("reward", C.c_void_p), ("value", C.c_void_p), ("last_value", C.c_void_p), ("terminated", C.c_void_p),
        ("truncated", C.c_void_p), ("prev_done_in", C.c_void_p),
        ("advantage", C.c_void_p), ("returns", C.c_void_p), ("advantage_norm", C.c_void_p), ("valid", C.c_void_p),
        ("prev_done_out", C.c_void_p), ("partials", C.c_void_p), ("moments", C.c_void_p),
        ("in_stride", C.c_int64), ("out_stride", C.c_int64),
        ("gamma", C.c_double), ("lam", C.c_double), ("eps", C.c_double),
        ("T", C.c_int32), ("num_envs", C.c_int32), ("tile_offset", C.c_int32), ("n_tiles_total", C.c_int32),
        ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


HEAD_SAMPLE, HEAD_EVALUATE, HEAD_BACKWARD = 0, 1, 2  # enum wedm_head_op
HEAD_DETERMINISTIC = 1  # enum wedm_head_flag
HEAD_MAX_MODES = 19  # WEDM_HEAD_MAX_MODES
HEAD_STREAM0 = 0xC0000000  # WEDM_HEAD_STREAM0


class HeadDesc(C.Structure):
    """``struct wedm_head_desc``: what `wedm_policy_head` reads and where it writes (strides in elements; ``action``: the
    four float64 leaves servo, target_voltage, ON_time, OFF_time)."""

    _fields_ = [
        ("params", C.c_void_p), ("u", C.c_void_p), ("mode_index", C.c_void_p), ("action", C.c_void_p * 4),
        ("current_mode", C.c_void_p), ("log_prob", C.c_void_p), ("entropy", C.c_void_p), ("g_log_prob", C.c_void_p),
        ("g_entropy", C.c_void_p), ("grad_params", C.c_void_p),
        ("param_stride", C.c_int64), ("grad_stride", C.c_int64), ("seed", C.c_uint64), ("t", C.c_uint64),
        ("lo", C.c_double * 4), ("hi", C.c_double * 4), ("log_span", C.c_double * 4),
        ("modes", C.c_int32 * HEAD_MAX_MODES), ("n_modes", C.c_int32), ("rows", C.c_int32),
        ("env_id_offset", C.c_uint32), ("op", C.c_int32), ("flags", C.c_int32),
    ]


PPO_CLIP_VALUE, PPO_COUNT, PPO_MAIN, PPO_FOLD = 1, 2, 4, 8  # enum wedm_ppo_flag
PPO_SUMS, PPO_STATS, PPO_COUNT_WORDS = 7, 8, 2  # WEDM_PPO_SUMS, WEDM_PPO_STATS, WEDM_PPO_COUNT_WORDS
# enum wedm_ppo_stat: the entries of ``stats``
PPO_STAT_NAMES = ("n", "n_bad", "loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")


class PpoDesc(C.Structure):
    """``struct wedm_ppo_desc``: what `wedm_ppo_loss` reads and where it writes (strides in elements; ``n_src``: the length
    of the stored blocks that ``index`` points into)."""

    _fields_ = [
        ("params", C.c_void_p), ("value", C.c_void_p), ("index", C.c_void_p), ("u", C.c_void_p), ("mode_index", C.c_void_p),
        ("old_log_prob", C.c_void_p), ("advantage", C.c_void_p), ("returns", C.c_void_p), ("old_value", C.c_void_p),
        ("valid", C.c_void_p), ("grad_params", C.c_void_p), ("grad_value", C.c_void_p), ("partials", C.c_void_p),
        ("stats", C.c_void_p), ("count", C.c_void_p),
        ("param_stride", C.c_int64), ("grad_stride", C.c_int64), ("n_src", C.c_int64),
        ("clip", C.c_double), ("vf_coef", C.c_double), ("ent_coef", C.c_double), ("clip_value", C.c_double),
        ("lo", C.c_double * 4), ("hi", C.c_double * 4), ("log_span", C.c_double * 4),
        ("n_modes", C.c_int32), ("rows", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


NET_FORWARD, NET_BACKWARD, NET_FOLD, NET_ACCUMULATE = 1, 2, 4, 8  # enum wedm_net_flag
NET_RELU, NET_TANH = 0, 1  # enum wedm_net_activation
NET_MAX_HIDDEN = 128  # WEDM_NET_MAX_HIDDEN
NET_ACTIVATIONS = ("relu", "tanh")  # by enum value


class NetDesc(C.Structure):
    """``struct wedm_net_desc``: what `wedm_policy_net` reads and where it writes (strides in elements; ``n_src``: the rows
    of ``obs`` that ``index`` points into)."""

    _fields_ = [
        ("theta", C.c_void_p), ("obs", C.c_void_p), ("index", C.c_void_p), ("params", C.c_void_p), ("value", C.c_void_p),
        ("grad_params", C.c_void_p), ("grad_value", C.c_void_p), ("partials", C.c_void_p), ("grad_theta", C.c_void_p),
        ("obs_stride", C.c_int64), ("param_stride", C.c_int64), ("grad_stride", C.c_int64), ("n_src", C.c_int64),
        ("obs_dim", C.c_int32), ("hidden1", C.c_int32), ("hidden2", C.c_int32), ("n_modes", C.c_int32),
        ("activation", C.c_int32), ("rows", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


OPT_CLIP, OPT_KL_GATE, OPT_NEW_UPDATE, OPT_NORM, OPT_DECIDE, OPT_APPLY = 1, 2, 4, 8, 16, 32  # enum wedm_opt_flag
OPT_STATE, OPT_INFO = 8, 8  # WEDM_OPT_STATE, WEDM_OPT_INFO
OPT_ONE_BLOCK_MAX = 4096  # WEDM_OPT_ONE_BLOCK_MAX: the largest n that one block takes when no phase bit is set
# enum wedm_opt_state and enum wedm_opt_info: the entries of ``state`` (the last two are zero) and of ``info``
OPT_STATE_NAMES = ("b1pow", "b2pow", "t", "skipped_nonfinite", "skipped_kl", "latch")
OPT_INFO_NAMES = ("sumsq", "norm", "scale", "lr", "applied", "kl", "bc1", "bc2")


class OptDesc(C.Structure):
    """``struct wedm_opt_desc``: what `wedm_adam` reads and where it writes."""

    _fields_ = [
        ("theta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p), ("partials", C.c_void_p),
        ("state", C.c_void_p), ("info", C.c_void_p), ("kl", C.c_void_p),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
        ("max_norm", C.c_double), ("kl_limit", C.c_double),
        ("n", C.c_int32), ("flags", C.c_int32),
    ]


MB_COUNT, MB_OFFSETS, MB_SCATTER = 1, 2, 4  # enum wedm_mb_flag
MB_STREAM0 = 0xE0000000  # WEDM_MB_STREAM0: the Philox stream of key block c is MB_STREAM0 + c
MB_TILE, MB_MAX_ROWS, MB_MAX_PARTS = 1024, 1 << 26, 4096  # WEDM_MB_TILE, WEDM_MB_MAX_ROWS, WEDM_MB_MAX_PARTS


class MbDesc(C.Structure):
    """``struct wedm_mb_desc``: what `wedm_minibatch_index` reads and where it writes."""

    _fields_ = [
        ("valid", C.c_void_p), ("index", C.c_void_p), ("count", C.c_void_p), ("tile_counts", C.c_void_p), ("tile_base", C.c_void_p),
        ("seed", C.c_uint64), ("draw", C.c_uint64),
        ("rows", C.c_int32), ("n_parts", C.c_int32), ("flags", C.c_int32),
    ]


ELOG_MAX_PLANES, ELOG_MAX_ROWS = 32, 96  # WEDM_ELOG_MAX_PLANES, WEDM_ELOG_MAX_ROWS
ELOG_LAST, ELOG_SUM_F32, ELOG_SUM_F64, ELOG_SUM_I32 = 0, 1, 2, 3  # enum wedm_elog_kind
ELOG_COUNT, ELOG_SCATTER, ELOG_COMMIT = 1, 2, 4  # enum wedm_elog_flag


class ElogPlane(C.Structure):
    """``struct wedm_elog_plane``: one source block of `wedm_episode_log`, its rows of the ring and (a sum) its accumulators."""

    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("acc", C.c_void_p), ("src_stride", C.c_int64),
                ("n_rows", C.c_int32), ("elem_bytes", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32)]


class ElogDesc(C.Structure):
    """``struct wedm_elog_desc``: what `wedm_episode_log` reads and where it writes (strides in elements)."""

    _fields_ = [
        ("plane", ElogPlane * ELOG_MAX_PLANES),
        ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("mask", C.c_void_p),
        ("env_out", C.c_void_p), ("stamp_out", C.c_void_p), ("head", C.c_void_p), ("tile_counts", C.c_void_p),
        ("capacity", C.c_int64), ("env_id_offset", C.c_int64), ("stamp", C.c_int64),
        ("n_planes", C.c_int32), ("num_envs", C.c_int32), ("tile_offset", C.c_int32), ("n_tiles_total", C.c_int32),
        ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


class RW(enum.IntEnum):
    """``enum wedm_reward_term``: the ten terms of `wedm_reward`, in the order of their addition."""

    PROGRESS = 0
    STEP = 1
    WIRE_BREAK = 2
    TARGET = 3
    SPARKS = 4
    SHORTS = 5
    SHORT_STEPS = 6
    ENERGY = 7
    GAP_BELOW = 8
    TMAX_ABOVE = 9


RW_COUNT = 10  # WEDM_RW_COUNT


class RewardDesc(C.Structure):
    """``struct wedm_reward_desc``: what `wedm_reward` reads and where it writes (strides in elements)."""

    _fields_ = [
        ("f64", C.c_void_p), ("i8", C.c_void_p), ("pulse", C.c_void_p), ("sig", C.c_void_p), ("pos_before", C.c_void_p),
        ("restart", C.c_void_p), ("mask", C.c_void_p), ("reward_out", C.c_void_p), ("terms_out", C.c_void_p),
        ("stride", C.c_int64), ("terms_stride", C.c_int64),
        ("weight", C.c_double * RW_COUNT), ("pos_restart", C.c_double), ("gap_floor", C.c_double), ("tmax_ceiling", C.c_double),
        ("num_envs", C.c_int32), ("reserved", C.c_int32),
    ]


class SN(enum.IntEnum):
    """``enum wedm_sensor_field``: the rows of `wedm_sensor`'s float64 channel table."""

    SIGMA = 0
    GAIN_SPREAD = 1
    OFFSET_SPREAD = 2
    LSB = 3
    LO = 4
    HI = 5


SENSOR_FIELDS = 6               # WEDM_SENSOR_FIELDS
SN_SOURCE, SN_MAX_DELAY = 0, 1  # enum wedm_sensor_route
SENSOR_ROUTES = 2               # WEDM_SENSOR_ROUTES
SENSOR_MAX_DELAY = 7            # WEDM_SENSOR_MAX_DELAY
SENSOR_STREAM0 = 0xA0000000     # WEDM_SENSOR_STREAM0


class SensorDesc(C.Structure):
    """``struct wedm_sensor_desc``: what `wedm_sensor` reads, its state and where it writes (strides in elements)."""

    _fields_ = [
        ("plane", NormPlane * 2), ("chan", C.c_void_p), ("route", C.c_void_p), ("first", C.c_void_p), ("mask", C.c_void_p),
        ("episode", C.c_void_p), ("out", C.c_void_p), ("ring", C.c_void_p), ("pos", C.c_void_p), ("age", C.c_void_p),
        ("out_stride", C.c_int64), ("ring_stride", C.c_int64), ("seed", C.c_uint64), ("t", C.c_uint64),
        ("env_id_offset", C.c_uint32), ("num_envs", C.c_int32), ("n_out", C.c_int32), ("ring_len", C.c_int32),
        ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


class GEOMC(enum.IntEnum):
    """``enum wedm_geomc_field``: one row of the (material, diameter) combination table `wedm_derive_geometry` reads -- what
    `derive_geometry` derives from the diameter and the material alone, and ``PI_R = math.pi * (diameter / 2)``."""

    K_COND = 0
    TUF = 1
    A_SURF = 2
    S_AREA = 3
    JOULE_GEOM = 4
    KERF_BASE = 5
    PI_R = 6


GEOMC_COUNT = 7
# status bits of `wedm_derive_geometry`: a height that is NaN, infinite or <= 0; a height over the capacity; an index
# outside the combination table
GEOM_STATUS_HEIGHT, GEOM_STATUS_CAPACITY, GEOM_STATUS_INDEX = 1, 2, 4


class GeomDeriveDesc(C.Structure):
    """``struct wedm_geom_derive_desc``: what `wedm_derive_geometry` reads and where it writes (stride in elements)."""

    _fields_ = [
        ("segment_len", _d), ("buffer_len_bottom", _d), ("buffer_len_top", _d), ("contact_offset_top", _d),
        ("zone_start0", _i), ("contact_bottom0", _i), ("num_envs", _i), ("n_seg_max", _i),
        ("stride", C.c_int64), ("combo", C.c_void_p), ("n_diameters", _i), ("n_materials", _i),
        ("geom_f64", C.c_void_p), ("geom_i32", C.c_void_p),
    ]


# `wedm_draw_episode`: slot s < DRAW_ENVP_SLOTS is name s of `core.env_params.NAMES` (enum wedm_draw_slot_id), then the wire
# material, the workpiece height and the wire-diameter index; the Philox stream of call q is DRAW_STREAM0 + q
DRAW_ENVP_SLOTS = 15
DRAW_SLOT_MATERIAL, DRAW_SLOT_HEIGHT, DRAW_SLOT_DIAMETER = 15, 16, 17
DRAW_SLOTS = 18
DRAW_STREAM0 = 0x80000000
DRAW_NONE, DRAW_UNIFORM, DRAW_CHOICE = 0, 1, 2  # enum wedm_draw_kind


class DrawSlot(C.Structure):
    """``struct wedm_draw_slot``."""

    _fields_ = [("kind", _i), ("k", _i), ("lo", _d), ("hi", _d), ("span", _d)]


class DrawDesc(C.Structure):
    """``struct wedm_draw_desc``: what `wedm_draw_episode` draws and where it writes (stride in elements)."""

    _fields_ = [
        ("seed", C.c_uint64), ("env_id_offset", C.c_uint32), ("num_envs", _i), ("stride", C.c_int64),
        ("slot", DrawSlot * DRAW_SLOTS), ("base_flow_rate", _d), ("dt_s", _d),
        ("envp_src", C.c_void_p), ("envp_rows", C.c_void_p), ("material_index", C.c_void_p), ("wmat_table", C.c_void_p),
        ("wmat_rows", C.c_void_p), ("wmat_geom_table", C.c_void_p), ("geom_f64", C.c_void_p), ("height", C.c_void_p),
        ("diameter_index", C.c_void_p), ("geom_status", C.c_void_p), ("dynamic", _i), ("reserved", _i),
        ("geom", GeomDeriveDesc),
    ]
