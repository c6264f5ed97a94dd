/*
 * wedm_hip.h — C-ABI of the MI355X batched Wire-EDM step.
 *
 * This is the drop-in boundary for ONE hot path of geduardo/SPARC (`wedm` 0.2.0):
 * the per-microsecond physics step of `WireEDMEnv.step()`
 * (reference src/wedm/envs/wire_edm.py:116-157 and the five module `update()`s it
 * calls: modules/ignition.py:175-195, material.py:79-96, dielectric.py:82-163,
 * wire.py:259-347 (+ the stencil wire.py:58-123), mechanics.py:79-114).
 *
 * The reference is pure Python and has no FFI; the binding a maintainer would add
 * is a `ctypes.CDLL` load of `libwedm_hip.so`.  Every entry
 * point below therefore cites the Python method it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are DEVICE pointers unless noted;
 *   - the caller owns every byte of state (torch tensors on the host side); the
 *     library owns only the opaque handle and one small constant table;
 *   - every call returns an int32 status (WEDM_OK or a negative wedm_status);
 *     nothing throws across the boundary; wedm_last_error() gives the text;
 *   - launches are asynchronous on the `hipStream_t` passed as `void* stream`
 *     (NULL = the null stream); the library creates no streams and no threads;
 *   - a handle is not thread-safe: one handle per device per process.
 *
 * State layout: struct-of-arrays, field-major, environment-minor.  Field `f` of
 * environment `e` lives at  block[f * stride + e]  so that the 64 lanes of a
 * wavefront (64 consecutive environments) read 64 consecutive elements.
 * The wire temperature (float32) is QUAD-INTERLEAVED (ABI v4): four consecutive
 * segments of one environment form one 16-byte word, words are environment-minor,
 *     T[((seg >> 2) * stride + e) * 4 + (seg & 3)]          (WEDM_T_INDEX below),
 * i.e. T[ceil(n_seg_max / 4)][stride][4].  A lane that owns a run of consecutive
 * segments of one environment loads / stores it 16 bytes at a time
 * (global_load_dwordx4), and the 64 lanes of a wavefront still touch contiguous
 * 1-KB runs.  The cells of the last word past n_seg_max are padding: written at
 * reset (spool temperature), never read into a result, never rewritten by a step.
 * (ABI v3 had T[seg][env]: one dword per lane and instruction, which is what bound
 * the one-launch-per-microsecond kernels: DESIGN.md section 4.2.)
 *
 * What a launch writes (tests/test_memory_contract.py holds every kernel to it).  Every block is [rows][stride]; only
 * the first num_envs columns of a row are the library's, the columns [num_envs, stride) are the caller's padding, and
 * what lies before a block's first row and behind its last one is somebody else's memory.
 *   1. wedm_step and wedm_reset write only: columns [0, num_envs) of the rows of the bound state blocks (f64, i32, i8,
 *      T, obs, stats, reward, crater_log); the same columns of the pulse and signal-statistics blocks, where bound; in a bound trace ring, the
 *      slots and the environment window its descriptor names.
 *   2. Columns [num_envs, stride) of every one of those rows are never written, and no launch writes a byte before a
 *      block's first row or after its last row, the action leaves, the reset mask, the geometry, env-param and
 *      wire-material rows, the replay table, or the device copy of the params.
 *   3. 2 holds at every stride >= num_envs that wedm_bind_state accepts, not only at multiples of 64, and the results in
 *      the owned columns are the same at every such stride.
 */
#ifndef WEDM_HIP_H
#define WEDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WEDM_ABI_VERSION 4

/* element index of wire segment `seg` of environment `e` in the T block */
#define WEDM_T_INDEX(seg, stride, e) ((((int64_t)((seg) >> 2) * (int64_t)(stride) + (int64_t)(e)) << 2) + ((seg) & 3))
/* 16-byte words (rows of the T block) a wire of n_seg_max segments occupies */
#define WEDM_T_QUADS(n_seg_max) (((n_seg_max) + 3) >> 2)

/* ------------------------------------------------------------------ status */
typedef enum wedm_status {
    WEDM_OK = 0,
    WEDM_ERR_BAD_ARG = -1,     /* NULL pointer, non-positive size, bad enum      */
    WEDM_ERR_NOT_BOUND = -2,   /* wedm_step/reset before wedm_bind_state         */
    WEDM_ERR_HIP = -3,         /* a HIP runtime call failed (text in last_error) */
    WEDM_ERR_NO_DEVICE = -4,   /* no gfx950 device visible                       */
    WEDM_ERR_BAD_MODE = -5,    /* current_mode without crater data (material.py:108-113) */
    WEDM_ERR_UNSUPPORTED = -6  /* n_seg exceeds what the fused kernel can stage  */
} wedm_status;

/* ------------------------------------------------------- float64 state rows
 * One row per mutable Python-float attribute of EDMState (core/state.py:25-91)
 * plus the module-private floats the reference keeps outside the state
 * (dielectric.py:69-80, mechanics.py:60, wire.py:224,205).                   */
enum wedm_f64_field {
    WEDM_F_WORKPIECE_POS = 0,  /* state.workpiece_position        [um]   */
    WEDM_F_WIRE_POS,           /* state.wire_position             [um]   */
    WEDM_F_WIRE_VEL,           /* state.wire_velocity             [um/s] */
    WEDM_F_PREV_ACCEL,         /* MechanicsModule.prev_accel (mechanics.py:60) */
    WEDM_F_DEBRIS_VOLUME,      /* DielectricModule.debris_volume / state.debris_volume [mm^3] */
    WEDM_F_DEBRIS_DENSITY,     /* state.debris_density                   */
    WEDM_F_FLOW,               /* state.flow_rate == DielectricModule._last_flow_condition */
    WEDM_F_LAST_GAP,           /* DielectricModule._last_gap_um (init -1)       */
    WEDM_F_LAST_DENSITY,       /* DielectricModule._last_debris_density (init -1) */
    WEDM_F_WIRE_LAST_FLOW,     /* WireModule._last_flow_condition (init 0)      */
    WEDM_F_VOLTAGE,            /* state.voltage (None -> 0)              */
    WEDM_F_CURRENT,            /* state.current (None -> 0)              */
    WEDM_F_SPARK_Y,            /* state.spark_status[1]; NaN encodes None */
    WEDM_F_LAST_CRATER,        /* state.last_crater_volume        [mm^3] */
    WEDM_F_CAVITY,             /* state.cavity_volume             [mm^3] */
    WEDM_F_TARGET_DELTA,       /* state.target_delta   (latched action)  */
    WEDM_F_TARGET_VOLTAGE,     /* state.target_voltage (latched; 0 encodes None) */
    WEDM_F_ON_TIME,            /* state.ON_time        (latched; 0 encodes None) */
    WEDM_F_OFF_TIME,           /* state.OFF_time       (latched; 0 encodes None) */
    WEDM_F_TARGET_POS,         /* state.target_position                  */
    WEDM_F_UNWIND_VEL,         /* state.wire_unwinding_velocity          */
    WEDM_F_H_BASE,             /* WireModule.h_eff_zone outside the zone (float32 value) */
    WEDM_F_H_ZONE,             /* WireModule.h_eff_zone inside the zone  (float32 value) */
    WEDM_F_TMAX,               /* max(T) after the last step (float32 value)    */
    /* The driver's 1 ms voltage history (experiments/run_simulation.py:258-281) as a running sum:
     * VOLT_ACC = sum of state.voltage after every step since (and including) the last control
     * step, in step order; at a control step the kernels publish VOLT_SUM = VOLT_ACC (this step
     * included) and restart VOLT_ACC from this step's voltage.  With servo_interval = 1000 us
     * VOLT_SUM is exactly the sum of the <= 1001 samples `create_voltage_controller` averages
     * (run_simulation.py:262-270): this interval's microseconds plus the previous control step's. */
    WEDM_F_VOLT_ACC,
    WEDM_F_VOLT_SUM,
    WEDM_F64_COUNT
};

/* --------------------------------------------------------- int32 state rows */
enum wedm_i32_field {
    WEDM_I_TIME = 0,           /* state.time [us], LOW 32 bits (unsigned, wraps); the high word is WEDM_I_TIME_HI:
                                  the reference counts in unbounded Python ints (wire_edm.py:135).  Also Philox
                                  counter word 0 (an episode's variates repeat after 2^32 us = 71.6 simulated minutes) */
    WEDM_I_SINCE_SERVO,        /* state.time_since_servo                */
    WEDM_I_SINCE_OPEN_V,       /* state.time_since_open_voltage         */
    WEDM_I_SINCE_IGNITION,     /* state.time_since_spark_ignition       */
    WEDM_I_SINCE_SPARK_END,    /* state.time_since_spark_end            */
    WEDM_I_SPARK_DUR,          /* state.spark_status[2]                 */
    WEDM_I_RANDOM_SHORT_REM,   /* IgnitionModule.random_short_remaining */
    WEDM_I_DEBRIS_SHORT_REM,   /* IgnitionModule.debris_short_remaining */
    WEDM_I_TIME_CRITICAL,      /* state.time_in_critical_temp           */
    WEDM_I_CURRENT_MODE,       /* state.current_mode: n for "I<n>", 0 encodes None; -1 = None while the ignition module's
                                  current cache still names a mode of an earlier episode (reset_semantics 1 only) */
    WEDM_I_EPISODE,            /* resets seen by this environment (RNG counter word) */
    WEDM_I_KEY_LO,             /* Philox key, low  32 bits of the reset seed */
    WEDM_I_KEY_HI,             /* Philox key, high 32 bits of the reset seed */
    WEDM_I_SPARK_COUNT,        /* fresh sparks since reset (len(crater_volumes_um3), material.py:133) */
    WEDM_I_TIME_HI,            /* state.time >> 32: bumped by wedm_step when the low word wraps inside a launch (a launch
                                  advances an environment by less than 2^31 us: wedm_step refuses n_substeps * dt_us >= 2^31) */
    WEDM_I32_COUNT
};

/* ---------------------------------------------------------- int8 state rows */
enum wedm_i8_field {
    WEDM_B_SPARK_STATE = 0,    /* state.spark_status[0]: 0 idle, 1 spark, -1 short, -2 rest */
    WEDM_B_IS_SHORT,           /* state.is_short_circuit                */
    WEDM_B_WIRE_BROKEN,        /* state.is_wire_broken                  */
    WEDM_B_TARGET_REACHED,     /* state.is_target_distance_reached      */
    WEDM_B_DONE,               /* terminated: the environment is frozen until reset */
    WEDM_B_CTRL_STEP,          /* info["control_step"] of the LAST substep run */
    WEDM_B_ERROR,              /* sticky: 1 = fresh spark with a mode that has no crater data */
    WEDM_B_MODE_CACHED,        /* IgnitionModule._cached_current_mode is not None (ignition.py:79-81,98-113): a peak current
                                  has been looked up for a latched mode.  Survives a reset with reset_semantics 1; while
                                  state.current_mode is None, a set flag makes the lookup answer `default_current`
                                  instead of the fresh module's 60 A */
    WEDM_I8_COUNT
};

/* ------------------------------------------------ running statistics (optional)
 * Accumulated inside the kernels at every fresh spark with fire-and-forget float64 atomics
 * (one lane per environment, so the order of the additions is the order of the sparks); what
 * the reference computes from its `crater_volumes_um3` list in
 * `MaterialRemovalModule.get_crater_statistics` (material.py:207-227).  Count =
 * WEDM_I_SPARK_COUNT; mean = sum / n; std = sqrt(sumsq / n - mean^2).                        */
enum wedm_stat_field {
    WEDM_S_CRATER_SUM = 0,     /* sum of the sampled crater volumes            [um^3]   */
    WEDM_S_CRATER_SUMSQ,       /* sum of their squares                         [um^6]   */
    WEDM_S_CRATER_MIN,         /* smallest crater volume so far (+inf while n == 0)     */
    WEDM_S_CRATER_MAX,         /* largest crater volume so far  (-inf while n == 0)     */
    WEDM_STAT_COUNT
};

/* ------------------------------------------------ pulse statistics (optional)
 * The reference driver's "Sparks" / "Short pulses" (experiments/run_simulation.py:597-636) per control interval,
 * counted inside the kernels.  A SAMPLE is the state after one physics step an environment ran (a frozen environment
 * has none; the state right after a reset counts as a sample with current 0 and no short).  With I = state.current and
 * threshold 0.1 A:  spark pulse = a sample where (I > 0.1) && !is_short_circuit holds and did not hold at the previous
 * sample; short pulse = the same with is_short_circuit; short step = a sample with is_short_circuit.  The *_ACC rows
 * accumulate sample by sample; at every control step (this step's sample included) the kernels publish them into the
 * *_LAST rows and restart them from zero.  A reset (wedm_reset, the in-launch autoreset, either reset_semantics) clears
 * all six rows.  Counts are per physics step: with dt_us = 2 short_steps counts steps, not microseconds.            */
enum wedm_pulse_field {
    WEDM_P_SPARK_ACC = 0,      /* spark pulses since the last control step          */
    WEDM_P_SHORT_ACC,          /* short pulses since the last control step          */
    WEDM_P_SHORT_STEPS_ACC,    /* short-circuit samples since the last control step */
    WEDM_P_SPARK_LAST,         /* spark pulses of the last completed interval       */
    WEDM_P_SHORT_LAST,         /* short pulses of the last completed interval       */
    WEDM_P_SHORT_STEPS_LAST,   /* short-circuit samples of the last completed interval */
    WEDM_PULSE_COUNT
};

/* ------------------------------------------------ signal statistics (optional)
 * What a controller works from over one control interval besides the voltage sum (WEDM_F_VOLT_SUM) and the pulse counts:
 * the current and the energy that went into the gap, how close the wire came to the workpiece and how hot it got at its
 * worst.  A SAMPLE is what it is for the pulse block: the state after one physics step an environment ran (a frozen
 * environment has none; with keep_stepping_terminated every step it keeps running is one).  With V = state.voltage,
 * I = state.current, gap = workpiece_position - wire_position (the float64 expression observation column 0 rounds) and
 * tmax = row WEDM_F_TMAX after the step, the *_ACC rows are updated sample by sample, in step order, in float64:
 * SAMPLES += 1, CURRENT += I, ENERGY += V * I (the product rounded to float64, then the addition: never fused), GAP += gap,
 * GAP_MIN = min(GAP_MIN, gap), TMAX_PEAK = max(TMAX_PEAK, (double)tmax).  At every control step (this step's sample
 * included) the kernels publish the six accumulators into the *_LAST rows and restart them from their identities
 * 0, 0, 0, 0, +inf, -inf: a publication has SAMPLES >= 1 and never holds an infinity.  A reset (wedm_reset, the in-launch
 * autoreset, either reset_semantics) sets the *_ACC rows to their identities and the *_LAST rows to 0.  The accumulators
 * survive launches: single microseconds and one fused launch give the same rows.
 * Observation: a control step also writes five float32 columns, (float) of CURRENT_LAST, ENERGY_LAST, GAP_LAST,
 * GAP_MIN_LAST, TMAX_PEAK_LAST (raw sums, not means), at columns base .. base + 4, where base = 11 while a pulse block is
 * bound (wedm_bind_pulse_stats) and 8 otherwise; only where wedm_params.obs_dim >= base + 5.                          */
enum wedm_sig_field {
    WEDM_SG_SAMPLES_ACC = 0,   /* samples since the last control step                          */
    WEDM_SG_CURRENT_ACC,       /* sum of state.current over them                     [A]       */
    WEDM_SG_ENERGY_ACC,        /* sum of state.voltage * state.current               [V A]     */
    WEDM_SG_GAP_ACC,           /* sum of workpiece_position - wire_position          [um]      */
    WEDM_SG_GAP_MIN_ACC,       /* smallest such gap (+inf while there is no sample)  [um]      */
    WEDM_SG_TMAX_PEAK_ACC,     /* largest WEDM_F_TMAX (-inf while there is no sample)          */
    WEDM_SG_SAMPLES_LAST,      /* the same six of the last completed interval                  */
    WEDM_SG_CURRENT_LAST,
    WEDM_SG_ENERGY_LAST,
    WEDM_SG_GAP_LAST,
    WEDM_SG_GAP_MIN_LAST,
    WEDM_SG_TMAX_PEAK_LAST,
    WEDM_SIG_COUNT
};

/* ------------------------------------ per-environment physics parameters (optional)
 * Domain randomisation: one value per environment of each row below, float64, overriding the uniform value of the same
 * name in wedm_params (derived rows hold what the host derives, exactly as for wedm_params: damping_coeff =
 * -2 zeta omega_n, stiffness_coeff = -(omega_n ** 2), max_jerk_dt = max_jerk * dt_s, debris_removal_per_us =
 * efficiency * base_flow_rate * 1e-6).  Not in the set, on purpose: the random-short parameters (has_random_short is a
 * wave-uniform switch), the crater and current tables, material properties and tcrit / tbreak (the served kernels'
 * no-break proof relies on them) and geometry (wedm_geom_*_field).  Nothing of the reset reads any of these rows.   */
enum wedm_envp_field {
    WEDM_EP_BASE_CRITICAL_DENSITY = 0,
    WEDM_EP_GAP_COEFFICIENT,
    WEDM_EP_MAX_CRITICAL_DENSITY,
    WEDM_EP_HARD_SHORT_GAP,
    WEDM_EP_SIGMOID_STEEPNESS,
    WEDM_EP_SPARK_VOLTAGE_FACTOR,
    WEDM_EP_DEBRIS_REMOVAL_PER_US,     /* dielectric.py:64-66, 150-158                       */
    WEDM_EP_DIELECTRIC_TEMPERATURE,    /* the float32 stencil rounds it to float32           */
    WEDM_EP_PLASMA_EFFICIENCY,         /* wire.py:298                                       */
    WEDM_EP_BASE_CONVECTION,           /* wire.py:349-374                                   */
    WEDM_EP_DAMPING_COEFF,             /* mechanics.py:52                                   */
    WEDM_EP_STIFFNESS_COEFF,           /* mechanics.py:53                                   */
    WEDM_EP_OMEGA_N,                   /* velocity control                                  */
    WEDM_EP_MAX_ACCELERATION,
    WEDM_EP_MAX_JERK_DT,               /* mechanics.py:57                                   */
    WEDM_EP_MAX_SPEED,
    WEDM_ENVP_COUNT
};

/* ------------------------------------------------ per-environment wire material (optional)
 * One wire material per environment: float64, one value per environment of each row below, overriding the uniform value
 * of the same quantity in wedm_params, bit for bit as the host derives it for wedm_params (rho_c = density *
 * specific_heat, critical temperature = melting_point * critical_temp_threshold).  The material's conductivity and heat
 * capacity also enter WEDM_G_K_COND and WEDM_G_TUF of the geometry rows, so the block needs per-environment geometry.
 * Nothing of the reset reads any of these rows.                                                                      */
enum wedm_wmat_field {
    WEDM_WM_RHO_ELEC = 0,          /* electrical_resistivity                     (wire.py:186)            */
    WEDM_WM_ALPHA_RHO,             /* temperature_coefficient                    (wire.py:187)            */
    WEDM_WM_RHO_C,                 /* density * specific_heat                    (wire.py:305-310 prefix) */
    WEDM_WM_CRITICAL_TEMPERATURE,  /* melting_point * critical_temp_threshold    (wire.py:216-218)        */
    WEDM_WM_BREAKING_TEMPERATURE,  /* breaking_temperature                       (wire.py:220)            */
    WEDM_WMAT_COUNT
};

/* -------------------------------------- per-environment geometry (optional)
 * BASELINE config 5: workpiece_height / wire_diameter differ per environment.
 * When bound, these rows override the uniform values in wedm_params.       */
enum wedm_geom_f64_field {
    WEDM_G_HEIGHT = 0,         /* config.workpiece_height [mm]                       */
    WEDM_G_KERF_BASE,          /* base_overcut + wire_diameter (material.py:158-160) */
    WEDM_G_CAVITY_COEFF,       /* pi * r * h              (dielectric.py:62)         */
    WEDM_G_K_COND,             /* k * S / dy              (wire.py:174-176)          */
    WEDM_G_TUF,                /* dt / (rho c S dy)       (wire.py:195)              */
    WEDM_G_A_SURF,             /* 2 pi r dy               (wire.py:171)              */
    WEDM_G_S_AREA,             /* pi r^2                  (wire.py:170)              */
    WEDM_G_JOULE_GEOM,         /* dy / S                  (wire.py:183)              */
    WEDM_GEOM_F64_COUNT
};
enum wedm_geom_i32_field {
    WEDM_GI_N_SEG = 0,         /* wire.py:149      */
    WEDM_GI_ZONE_START,        /* wire.py:151,156  (plasma index base)  */
    WEDM_GI_AZ_START,          /* wire.py:207      (h_eff zone start)   */
    WEDM_GI_AZ_END,            /* wire.py:208      (h_eff zone end)     */
    WEDM_GI_CONTACT_BOTTOM,    /* wire.py:239-248  */
    WEDM_GI_CONTACT_TOP,       /* wire.py:242-251  */
    WEDM_GEOM_I32_COUNT
};

/* ----------------------------------------------------------------- params
 * Everything that is constant during a run.  Derived constants are computed by
 * the HOST in the reference's own float arithmetic (Python floats) and passed in
 * verbatim: the device never re-derives them (SURVEY.md §7 "floor-division
 * geometry quirks").                                                        */
#define WEDM_MAX_MODE 19

typedef struct wedm_params {
    /* EnvironmentConfig (core/env_config.py:17-35) */
    int32_t servo_interval;       /* [us] */
    int32_t dt_us;                /* [us] */
    int32_t control_mode;         /* 0 = position, 1 = velocity (mechanics.py:62-67) */
    int32_t per_env_geometry;     /* 0 = uniform values below, 1 = geometry rows bound */
    double initial_gap;
    double target_cutting_distance;

    /* uniform geometry (WireModule.__init__, wire.py:143-257) */
    int32_t n_seg, zone_start, az_start, az_end, contact_bottom, contact_top;
    double workpiece_height, kerf_base, cavity_coeff;
    double k_cond, tuf, a_surf, s_area, joule_geom;
    double segment_len;           /* [mm] for plasma_idx = zone_start + int(y // segment_len) */

    /* wire material + WireModuleParameters */
    double spool_T, temp_ref, rho_elec, alpha_rho, rho_c;   /* rho_c = density * specific_heat */
    double plasma_efficiency, base_convection, convection_velocity_factor, convection_flow_enhancement;
    double critical_temperature, breaking_temperature;
    double dielectric_temperature;

    /* IgnitionModuleParameters (ignition.py:17-57) */
    double base_critical_density, gap_coefficient, max_critical_density, hard_short_gap;
    double sigmoid_steepness;
    int32_t debris_short_duration, random_short_duration;
    double random_short_min_gap, random_short_max_gap, random_short_max_probability;
    double ignition_a, ignition_b, ignition_c, ln2;
    double default_target_voltage, default_on_time, default_off_time, default_current;
    double spark_voltage_factor;

    /* DielectricModuleParameters (dielectric.py:15-31) */
    double reference_gap, debris_obstruction_coeff, debris_removal_per_us;

    /* MechanicsModuleParameters (mechanics.py:12-23), pre-multiplied as in mechanics.py:48-57 */
    double dt_s, damping_coeff, stiffness_coeff, omega_n;
    double max_acceleration, max_jerk_dt, max_speed;

    /* tables: index n = mode "I<n>", n in 1..19; index 0 unused.
     * mode_current: currents.json.  crater_*: area_corrected.json
     * (ellipsoid_volume_half, ellipsoid_volume_std, depth); crater_valid[n] = 0
     * where the reference raises ValueError (material.py:108-113).           */
    double mode_current[WEDM_MAX_MODE + 1];
    double crater_mean[WEDM_MAX_MODE + 1];
    double crater_std[WEDM_MAX_MODE + 1];
    double crater_depth[WEDM_MAX_MODE + 1];
    int32_t crater_valid[WEDM_MAX_MODE + 1];

    /* sharding: global id of local environment 0 (Philox counter word 2) */
    uint32_t env_id_offset;
    int32_t obs_dim;              /* columns of the obs matrix written at control steps (0 = none) */
    int32_t disable_ignition;     /* 1: skip IgnitionModule.update — the monkeypatch of
                                     experiments/single_spark_animation.py:218-223 (spark forced by the caller) */
    /* Next-step autoreset inside the launch (the termination of wire_edm.py:172-179 handled without the
     * host): 1 = an environment that is DONE when a wedm_step begins is re-initialised by that launch
     * exactly as wedm_reset(mask = its DONE flag, reseed = 0) would (episode + 1, module state cleared,
     * wire at the spool temperature, statistics and observation zeroed) and then steps on.  Its DONE /
     * terminal flags therefore stay readable between two launches.                                   */
    int32_t autoreset;
    /* 0 = the reward row is never written (the reference's `_calculate_reward` is a TODO returning 0.0,
     * wire_edm.py:185-187); 1 = every wedm_step writes, for the environments it stepped, the float32
     * reward of that launch: (workpiece_position after - workpiece_position at the start of the launch
     * [after an autoreset]) - reward_break_penalty * is_wire_broken.                                  */
    int32_t reward_mode;
    /* typing of the wire stencil (wire.py:58-123): 0 = float32 op for op (what the reference computes when
     * NumPy-2 scalar promotion evaluates it, i.e. without Numba); 1 = float64 expressions rounded at each
     * float32 store (how Numba types the same lines; without fastmath re-association).                 */
    int32_t stencil_mode;
    /* what wedm_reset (and the in-launch autoreset) re-initialises: 0 = everything, module-private state included (a
     * fresh environment: the default, documented deviation); 1 = what the reference's reset() does (wire_edm.py:106-114):
     * a new EDMState only -- the module objects live on, so the ignition short timers and current cache
     * (ignition.py:75-81), the debris volume and the flow / density caches (dielectric.py:69-80), `prev_accel`
     * (mechanics.py:60), the convection cache and coefficients (wire.py:205,224) and the crater list / statistics
     * (material.py:133) carry over into the next episode.                                                        */
    int32_t reset_semantics;
    /* 0 = a terminated environment is frozen until it is reset (the default, documented deviation); 1 = it keeps being
     * stepped as the reference does when step() is called after `terminated` (wire_edm.py:116-157 has no guard): after a
     * wire break the wire module returns at once (wire.py:260-261) and the step returns before mechanics and clocks
     * (wire_edm.py:129-130); after the cutting target everything goes on.  WEDM_B_DONE then holds `terminated` of the
     * last step (is_wire_broken or is_target_distance_reached) and freezes nothing.                              */
    int32_t keep_stepping_terminated;
    double reward_break_penalty;  /* reward_mode 1 */
} wedm_params;

typedef struct wedm_state_ptrs {
    double* f64;        /* [WEDM_F64_COUNT][stride] */
    int32_t* i32;       /* [WEDM_I32_COUNT][stride] */
    int8_t* i8;         /* [WEDM_I8_COUNT ][stride] */
    float* T;           /* [WEDM_T_QUADS(n_seg_max)][stride][4], see WEDM_T_INDEX */
    float* obs;         /* [obs_dim][stride] or NULL */
    int64_t stride;     /* >= num_envs, multiple of 64 recommended (any other is served too: "What a launch writes") */
    double* stats;      /* [WEDM_STAT_COUNT][stride] or NULL (statistics not kept) */
    float* reward;      /* [stride] or NULL; written when wedm_params.reward_mode != 0 */
    /* `MaterialRemovalModule.crater_volumes_um3` (material.py:133): every sampled crater volume [um^3] of an
     * environment, in spark order — crater number k (0-based since the reset) lands in
     * crater_log[(k % crater_log_capacity) * stride + env]; WEDM_I_SPARK_COUNT says how many there are.  NULL /
     * capacity 0: not kept.                                                                              */
    double* crater_log; /* [crater_log_capacity][stride] or NULL */
    int64_t crater_log_capacity;
} wedm_state_ptrs;

typedef struct wedm_geom_ptrs {
    const double* f64;  /* [WEDM_GEOM_F64_COUNT][stride] */
    const int32_t* i32; /* [WEDM_GEOM_I32_COUNT][stride] */
} wedm_geom_ptrs;

/* Action leaves of WireEDMEnv.action_space (wire_edm.py:84-98), one value per env.
 * float64 because `_apply_action` keeps the caller's precision (`float(x[0])`,
 * wire_edm.py:162-170).                                                        */
typedef struct wedm_action_ptrs {
    const double* servo;           /* -> state.target_delta   */
    const double* target_voltage;  /* -> state.target_voltage */
    const double* on_time;         /* -> state.ON_time        */
    const double* off_time;        /* -> state.OFF_time       */
    const int32_t* current_mode;   /* -> state.current_mode "I<n>" */
} wedm_action_ptrs;

/* Device-side signal trace: while wedm_step runs, the kernels copy the selected rows of the
 * state blocks (and optionally the whole wire temperature) of a contiguous range of
 * environments into caller-owned ring buffers every `every` microseconds.  Replaces the
 * per-microsecond `SimulationLogger.collect(env.state, info)` of the reference driver
 * (utils/logger.py:110-160, experiments/run_simulation.py:257) and its 1 ms voltage history
 * (run_simulation.py:262-270) without leaving the fused launch.  Sample m (1-based count of
 * microseconds stepped since wedm_bind_trace) is taken after the step when m % every == 0 and
 * lands in ring slot (m / every - 1) % capacity.  Rows are packed in ascending row order.   */
typedef struct wedm_trace_desc {
    double* f64;        /* [capacity][popcount(f64_mask)][env_count], NULL iff f64_mask == 0 */
    int32_t* i32;       /* [capacity][popcount(i32_mask)][env_count], NULL iff i32_mask == 0 */
    int8_t* i8;         /* [capacity][popcount(i8_mask) ][env_count], NULL iff i8_mask  == 0 */
    float* T;           /* [capacity][n_seg_max][env_count] or NULL (no temperature trace)   */
    uint32_t f64_mask;  /* bit r: record row r of wedm_f64_field */
    uint32_t i32_mask;  /* bit r: record row r of wedm_i32_field */
    uint32_t i8_mask;   /* bit r: record row r of wedm_i8_field  */
    int32_t env_lo;     /* first traced environment (local index) */
    int32_t env_count;  /* number of traced environments          */
    int32_t every;      /* sample period in microseconds, >= 1    */
    int32_t capacity;   /* ring capacity in samples, >= 1         */
    int32_t reserved0;
} wedm_trace_desc;

/* Variate injection (validation mode).  Instead of its Philox stream an environment consumes caller-provided
 * variates: what the reference drew from its own NumPy Generator(PCG64) at the call sites ignition.py:233,239,
 * 261,327 and material.py:127 (`env.np_random`, seeded by reset(seed), wire_edm.py:55,107), laid out by physics
 * step since the reset and by slot,  table[(step * WEDM_REPLAY_SLOTS + slot) * stride + env],  NaN where the
 * reference drew nothing in that step.  With it the device follows a native-seed run of the reference
 * (fixture F1) directly.  Runs on the global-memory kernel only.                                       */
enum wedm_replay_slot {
    WEDM_RS_DEBRIS_ROLL = 0,   /* Generator.random() compared with p_debris   (ignition.py:233) */
    WEDM_RS_RANDOM_ROLL,       /* Generator.random() compared with p_random   (ignition.py:239) */
    WEDM_RS_IGNITION_ROLL,     /* Generator.random() compared with lambda     (ignition.py:327) */
    WEDM_RS_SPARK_Y,           /* Generator.uniform(0, workpiece_height)      (ignition.py:261) */
    WEDM_RS_CRATER_UM3,        /* Generator.normal(mean, std) [um^3]          (material.py:127) */
    WEDM_REPLAY_SLOTS
};

typedef struct wedm_ctx wedm_ctx;

/* version of this header the library was built against */
int32_t wedm_abi_version(void);

/* fingerprint of the build: the first 16 hex digits of the sha256 over the kernel sources (every *.hip, *.h
 * and *.inc of sparc_amd/csrc/, this header) and the compiler flags, baked in by the build (__graft_entry__.build_hip).  Measurement
 * records (profiles/valu.json, profiles/traffic.json) carry the id of the library they were counted on, and bench.py
 * prices a live duration with a recorded instruction / byte count only when the ids agree.  "unknown" for a library
 * built by hand without -DWEDM_BUILD_ID.                                                                        */
const char* wedm_build_id(void);

/* replaces WireEDMEnv.__init__ (wire_edm.py:22-101): validates sizes, copies
 * `params`, selects the device that is current at call time.                  */
int32_t wedm_create(const wedm_params* params, int32_t num_envs, int32_t n_seg_max, wedm_ctx** out);
int32_t wedm_destroy(wedm_ctx* ctx);

/* replaces the EDMState() allocation (wire_edm.py:58,110): adopts caller-owned memory */
int32_t wedm_bind_state(wedm_ctx* ctx, const wedm_state_ptrs* state);
int32_t wedm_bind_geometry(wedm_ctx* ctx, const wedm_geom_ptrs* geom);

/* replaces WireEDMEnv.reset (wire_edm.py:106-114) for the environments whose
 * mask byte is non-zero (mask == NULL: all).  `reseed` bit 0: re-key their RNG with
 * `seed` (else their episode counter is bumped).  Module-private state is reset too
 * unless wedm_params.reset_semantics is 1 (the reference's own reset); `reseed` bit 1
 * (WEDM_RESET_FRESH) resets it whatever the semantics -- what constructing the module
 * objects does in WireEDMEnv.__init__ (wire_edm.py:60-82): a handle's first reset. */
#define WEDM_RESET_RESEED 1
#define WEDM_RESET_FRESH 2
int32_t wedm_reset(wedm_ctx* ctx, const uint8_t* mask, uint64_t seed, int32_t reseed, void* stream);

/* replaces `n_substeps` consecutive WireEDMEnv.step(action) calls
 * (wire_edm.py:116-157) with the same action.  n_substeps == 1 is the
 * reference's 1 us step.                                                      */
int32_t wedm_step(wedm_ctx* ctx, int32_t n_substeps, const wedm_action_ptrs* action, void* stream);

/* binds (table != NULL) or removes (table == NULL) the variate table described at wedm_replay_slot; `n_steps`
 * physics steps are covered (an environment stepped beyond them gets its ERROR flag set).                 */
int32_t wedm_bind_rng_replay(wedm_ctx* ctx, const double* table, int64_t n_steps);

/* binds (rows != NULL) or removes (rows == NULL) the caller-owned pulse-statistics block
 * int32 [WEDM_PULSE_COUNT][stride] described at wedm_pulse_field (same stride as the state blocks).  While it is bound,
 * wedm_step runs the kernels' pulse-counting instantiations: kernels 7, 8 and 2 (float32 stencil, no trace sample in the
 * launch) and kernel 1 for every other launch; wedm_set_kernel values without such a form make wedm_step return
 * WEDM_ERR_UNSUPPORTED.  With wedm_params.obs_dim >= 11 the control steps also write the three published counts into
 * obs columns 8, 9, 10 (float32).  Binding does not clear the block: wedm_reset does.                                */
int32_t wedm_bind_pulse_stats(wedm_ctx* ctx, int32_t* rows);

/* binds (rows != NULL) or removes (rows == NULL) the caller-owned per-environment physics parameters:
 * float64 [WEDM_ENVP_COUNT][stride] described at wedm_envp_field (same stride as the state blocks), read at the start of
 * every wedm_step (the caller may rewrite them between launches, stream-ordered).  While they are bound, wedm_step runs
 * the kernels' ENVP instantiations: kernel 2's packed form (float32 stencil, no trace sample, no pulse statistics) and
 * kernel 1 for every other launch; wedm_set_kernel values other than 0, 1 and 2 make wedm_step return
 * WEDM_ERR_UNSUPPORTED.  wedm_reset reads none of the rows.                                                            */
int32_t wedm_bind_env_params(wedm_ctx* ctx, const double* rows);

/* binds (rows != NULL) or removes (rows == NULL) the caller-owned per-environment wire material:
 * float64 [WEDM_WMAT_COUNT][stride] described at wedm_wmat_field (same stride as the state blocks), read at the start of
 * every wedm_step (the caller may rewrite them between launches, stream-ordered, together with the material's
 * WEDM_G_K_COND / WEDM_G_TUF geometry rows).  Binding needs per-environment geometry (wedm_params.per_env_geometry and
 * wedm_bind_geometry): WEDM_ERR_NOT_BOUND otherwise.  While they are bound, wedm_step runs the kernels' MAT
 * instantiations: kernel 2's packed form (float32 stencil, no trace sample, no pulse statistics; with or without
 * per-environment physics parameters) and kernel 1 for every other launch; wedm_set_kernel values other than 0, 1 and 2,
 * and injected variates (wedm_bind_rng_replay), make wedm_step return WEDM_ERR_UNSUPPORTED.  wedm_reset reads none of
 * the rows.                                                                                                            */
int32_t wedm_bind_wire_material(wedm_ctx* ctx, const double* rows);

/* binds (rows != NULL) or removes (rows == NULL) the caller-owned signal-statistics block
 * float64 [WEDM_SIG_COUNT][stride] described at wedm_sig_field (same stride as the state blocks; WEDM_ERR_NOT_BOUND before
 * wedm_bind_state).  While it is bound, wedm_step runs the kernels' SIG instantiations: kernel 2's packed form for a fused
 * launch of the float32 stencil without a trace sample and without pulse statistics (with or without per-environment
 * physics parameters and wire material), kernel 1 for every other launch; wedm_set_kernel values other than 0, 1 and 2,
 * and injected variates (wedm_bind_rng_replay), make wedm_step return WEDM_ERR_UNSUPPORTED.  The control steps also write
 * the five observation columns described at wedm_sig_field.  Binding does not clear the block: wedm_reset does.        */
int32_t wedm_bind_signal_stats(wedm_ctx* ctx, double* rows);

/* binds (desc != NULL) or removes (desc == NULL) the signal trace; resets the sample counter.
 * Terminated environments keep being sampled (their frozen state).                        */
int32_t wedm_bind_trace(wedm_ctx* ctx, const wedm_trace_desc* desc);

/* samples written since wedm_bind_trace (host-side count; the ring holds the last
 * min(count, capacity) of them, the newest in slot (count - 1) % capacity)                */
int64_t wedm_trace_samples(wedm_ctx* ctx);

/* selects the kernel used by wedm_step: 0 = auto, 1 = global-memory stencil (one pass
 * over T in HBM per substep), 2 = LDS-staged predicated stencil (any geometry),
 * 3 = LDS-staged fused stencil walking a wave-uniform tile table (uniform geometry),
 * 4 = the same with two chunks per lane advanced by packed float32 math,
 * 5 = global-memory stencil with the wire split over the four waves of a block (single
 * microseconds, any geometry), 6 = stream kernel (single microseconds, uniform geometry: the whole
 * chunk of a lane requested up front, tile walk in LDS, no barrier; the automatic choice for
 * n_substeps == 1 where one round of blocks covers the batch), 7 = register kernel (one environment per
 * lane with its whole wire in registers: no LDS, the scalar physics once per environment; uniform geometry,
 * at most 128 segments, either typing of the stencil; own instantiation for launches with a trace sample),
 * 8 = wide register kernel (4, 8 or 16 lanes per environment -- the fewest that hold the wire at 32 cells per lane --
 * with the wire in their registers and per-cell zone / contact coefficients: no LDS, no tile table; uniform geometry,
 * 9 to 512 segments, either typing of the stencil; the automatic choice for fused launches of a batch that one round of blocks
 * covers: environments x lanes <= 65 536; own instantiations for wires whose length is not a multiple of 8 and for
 * launches with a trace sample), 9 = served kernel (kernel 4's walk -- 4 or 8 lanes per environment, the wire in LDS --
 * with the float64 scalar physics of a block's environments on a FIFTH wave of the block, one lane per environment, one
 * microsecond ahead of the four walking waves where it can prove that the step does not break the wire; coefficients and
 * maxima cross through LDS; uniform geometry, float32 stencil, freeze-on-termination; launches with a trace sample take
 * kernel 4), 10 = kernel 2's cell-by-cell form by name (since round 4 kernel 2 itself is the packed form -- two virtual
 * chunks per lane advanced in float2 registers, per-cell coefficients from the lane's own indices -- wherever the stencil is
 * float32, and the same walk with float64-typed cells under stencil_mode 1; the cell-by-cell form remains for A/B timing), 11 = the served form of kernel 2 (its walk
 * on three waves of a block, the scalar physics on the fourth, as kernel 9; by name only: not faster at BASELINE configs[4]),
 * 12 = the served form of kernel 7 (two walker waves with the wire in registers + a scalar wave with all 64 lanes busy; by name
 * only: 1.666e10 against kernel 7's 1.674e10 at the headline batch, spills; at most 128 segments, no trace sample).
 * All variants produce bit-identical results.  With wedm_params.stencil_mode 1 only 0, 1, 2 (= 10), 3, 6 (launches of one microsecond
 * without a trace sample, chunks of at most 64 cells), 7 and 8 are accepted (7 / 8: the
 * register walks with every interior cell in Numba's typing -- 18 float64 operations per cell -- and, for kernel 8, a
 * 256-register instantiation at two blocks per CU for batches beyond one wave per SIMD; 3: the tile walk with per-cell
 * coefficients; no packed, served or single-microsecond form -- 0 takes kernel 7 from 20 480 environments of at most 128
 * segments, kernel 8 for other wires of 9 to 512 segments, else 3 / 2 / 1).                       */
int32_t wedm_set_kernel(wedm_ctx* ctx, int32_t variant);

/* lanes that share one environment in kernels 2, 3, 4 and 6: 0 = auto, or 1, 2, 4, 8 (16: not kernel 4); kernel 7: 1, anything
 * else = 2; kernel 8: 0 = the fewest, or 4, 8, 16 if 32 cells per lane cover the wire.  A lane count set here also keeps
 * the automatic choice (kernel 0) off the register kernels.                                                          */
int32_t wedm_set_lanes(wedm_ctx* ctx, int32_t lanes);

/* name / launch geometry of the kernel the last wedm_step used (for profiles) */
const char* wedm_last_kernel(wedm_ctx* ctx);

const char* wedm_last_error(wedm_ctx* ctx);

/* sizeof(wedm_params) the library was compiled with (layout cross-check for bindings) */
int64_t wedm_sizeof_params(void);

/* Blocks of the last launch's kernel that the occupancy API admits per compute unit at that launch's block size and
 * dynamic LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor), or a negative status.  Diagnostic: measurement scripts
 * record it next to a kernel's name; nothing in the library depends on it.                                          */
int32_t wedm_last_occupancy(wedm_ctx* ctx);

/* ---------------------------------------------------- copying environments (snapshot, restore, fork)
 * Every block of this ABI is [rows][stride] with the environment as the column, so moving the state of environment a into
 * environment b -- or into a snapshot's block, or back -- is one operation on every block: column a of every row to
 * column b.  A PLANE names one block on both sides of the copy.  The blocks map to planes like this:
 *   T [WEDM_T_QUADS(n_seg_max)][stride][4]                              rows = WEDM_T_QUADS(n_seg_max), elem_bytes 16
 *   f64, stats, crater_log, the signal block, env-param and wire-material rows   elem_bytes 8
 *   i32, obs, reward, the pulse block                                   elem_bytes 4
 *   i8                                                                  elem_bytes 1
 * Strides are in elements of elem_bytes.  src_cols / dst_cols are the columns that may be named on either side (num_envs
 * of an environment's block, not its stride: the padding columns are not environments).
 * Not state, and so no plane of any caller in this repository: a bound trace ring, the replay table, the geometry rows
 * (height and diameter belong to the slot, not to what is being simulated in it) -- except where the caller redraws the
 * geometry per episode (wedm_derive_geometry below): there the two geometry blocks are state and travel as planes.     */
#define WEDM_COPY_MAX_PLANES 16
typedef struct wedm_copy_plane {
    const void* src;     /* first row of the source block                                   */
    void* dst;           /* first row of the destination block (may be the same memory)     */
    int32_t rows;        /* rows of both blocks, >= 0                                       */
    int32_t elem_bytes;  /* 1, 4, 8 or 16; both base pointers are aligned to it             */
    int64_t src_stride;  /* elements from one row to the next, >= src_cols                  */
    int64_t dst_stride;  /* elements from one row to the next, >= dst_cols                  */
    int32_t src_cols;    /* valid source columns:      src_idx must lie in [0, src_cols)    */
    int32_t dst_cols;    /* valid destination columns: dst_idx must lie in [0, dst_cols)    */
} wedm_copy_plane;

/* For every i in [0, count) and every plane: column src_idx[i] of each of the plane's rows is copied to column dst_idx[i],
 * bit for bit (raw integer words: a NaN keeps its payload), in one launch on `stream` (more than 65 535 * 8 rows in all:
 * several).  Stateless: no wedm_ctx, the device is the current one, every byte is the caller's -- planes may lie in one
 * set of blocks (fork) or in two (snapshot, restore).  `planes` is HOST memory, read before the call returns; src_idx,
 * dst_idx and status are device pointers.
 * Bounds are checked on the device, because the index lists may be device data nobody has read: a pair with src_idx[i]
 * outside [0, src_cols) or dst_idx[i] outside [0, dst_cols) of a plane copies nothing in that plane and ORs 1 into
 * *status (status == NULL: it is skipped silently).  No index list, however wrong, makes the call read or write outside a
 * plane's rows x columns; columns [cols, stride) are never written.
 * count == 0 launches nothing and returns WEDM_OK.  WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)): planes NULL, n_planes
 * outside [1, WEDM_COPY_MAX_PLANES], count < 0, a NULL index list with count > 0, an elem_bytes other than 1 / 4 / 8 / 16, a
 * base pointer that is NULL or not aligned to elem_bytes, rows < 0, a negative column count, a stride smaller than its
 * column count.
 * PRECONDITION the call cannot check: where a plane's src and dst are the same memory, no destination index may equal a
 * source index or another destination index (one source may feed many destinations).  Otherwise the named destination
 * columns end up holding some source column's old or new value; nothing outside them is touched.                     */
int32_t wedm_copy_columns(const wedm_copy_plane* planes, int32_t n_planes, const int32_t* src_idx, const int32_t* dst_idx,
                          int32_t count, int32_t* status, void* stream);

/* ---------------------------------------------------- the wire's temperature profile, per environment
 * The wire is the largest piece of an environment's state; the observation carries one scalar of it (its maximum).  This call
 * reduces every named environment's wire, whatever its geometry, in one launch without temporaries: the mean over the
 * workpiece zone, the mean and the maximum over the wire, the hottest cell, and the wire pooled into `bins` bins (maximum
 * and mean of each).  Let n be the environment's n_seg and t[0..n) its cells (t[s] = T[WEDM_T_INDEX(s, stride, env)]):
 *   every MEAN is the float64 sum of the float32 cells, divided in float64 by the number of cells, rounded once to float32.
 *     Finite temperatures in [1, 65536) are multiples of 2^-23, and at most 2^11 such values below 2^16 sum exactly in
 *     float64 (16 + 11 + 23 = 50 bits): over such cells the ORDER OF THE SUM DOES NOT MATTER, every order gives the same
 *     bits, and the kernel reduces across lanes and waves as it likes.  Outside that range (or past 2^11 cells per mean) the
 *     order is unspecified;
 *   ZONE_MEAN  the mean over [az_start, az_end) if 0 <= az_start < az_end <= n, else over the whole wire (wire.py:390-394);
 *   WIRE_MEAN, WIRE_MAX  over [0, n);
 *   HOT_CELL   the lowest index that holds the maximum, as float32;
 *   bin b of B covers the cells [lo, hi), lo = floor(b * n / B), hi = max(lo + 1, floor((b + 1) * n / B)): for n >= B a
 *     partition of the wire, for n < B nearest-cell replication; a bin is never empty and never reaches past n.
 * A NaN cell makes the maxima and means it takes part in unspecified; it never makes the call read or write outside its
 * blocks.  Cells past an environment's own n_seg (up to n_seg_max, and the last quad's padding) and the columns
 * [num_envs, stride) of T never reach a result.                                                                       */
#define WEDM_PROFILE_MAX_BINS 64
enum wedm_profile_field { WEDM_PR_ZONE_MEAN = 0, WEDM_PR_WIRE_MEAN, WEDM_PR_WIRE_MAX, WEDM_PR_HOT_CELL, WEDM_PR_FIXED };
/* rows of out: the WEDM_PR_FIXED rows, then bins rows BIN_MAX[b], then bins rows BIN_MEAN[b] */
#define WEDM_PROFILE_ROWS(bins) (WEDM_PR_FIXED + 2 * (bins))
typedef struct wedm_profile_desc {
    const float* T;            /* [WEDM_T_QUADS(n_seg_max)][stride][4] */
    int64_t stride;            /* of T and of geom_i32 */
    int32_t num_envs, n_seg_max;
    int32_t n_seg, az_start, az_end;   /* uniform geometry; read when geom_i32 == NULL */
    const int32_t* geom_i32;   /* [WEDM_GEOM_I32_COUNT][stride] or NULL: rows N_SEG, AZ_START, AZ_END are read */
    int32_t bins;              /* 0 .. WEDM_PROFILE_MAX_BINS */
    float* out;                /* [WEDM_PROFILE_ROWS(bins)][out_stride] */
    int64_t out_stride;
    int32_t out_cols;          /* columns of out that may be written: count <= out_cols <= out_stride */
} wedm_profile_desc;

/* Output column i (0 <= i < count) describes environment env_idx[i]; with env_idx == NULL, environment i.  One launch on
 * `stream`.  Stateless like wedm_copy_columns: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory,
 * read before the call returns; env_idx and status are device pointers.
 * Checked on the device (the index list and the geometry rows may be device data nobody has read): an env_idx[i] outside
 * [0, num_envs) writes nothing to column i and ORs 1 into *status; a geometry row with n_seg outside [1, n_seg_max] writes
 * nothing to column i and ORs 2 (status == NULL: both are skipped silently).  Columns [count, out_stride) of out are never
 * written.  count == 0 launches nothing and returns WEDM_OK.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)): desc NULL; T or out NULL, or T not 16-byte aligned; bins outside
 * [0, WEDM_PROFILE_MAX_BINS]; count < 0 or count > out_cols; out_cols > out_stride; stride < num_envs; num_envs < 1;
 * n_seg_max < 1; with geom_i32 == NULL an n_seg outside [1, n_seg_max]; env_idx == NULL with count > num_envs.           */
int32_t wedm_wire_profile(const wedm_profile_desc* desc, const int32_t* env_idx, int32_t count, int32_t* status, void* stream);

/* ---------------------------------------------------- geometry rows derived on the device (a new workpiece per episode)
 * The any-geometry step kernels read the geometry rows (wedm_bind_geometry) at the start of every launch, and a reset
 * re-initialises the whole wire.  An environment whose 8 + 6 rows are rewritten just before the launch that resets it is
 * therefore a fresh environment of the new geometry.  This call rewrites them from per-environment device arrays, with the
 * bits the host derivation writes.  The derivation is split:
 *   what depends on the wire DIAMETER (and the wire material) only comes from the caller's combination table, row
 *     material_idx * n_diameters + diameter_idx, WEDM_GEOMC_COUNT doubles per row (enum below): the six geometry values that
 *     do not depend on the height, copied verbatim, and PI_R = pi * (diameter / 2) [mm];
 *   what depends on the HEIGHT h is computed (float64, no contraction, `//` = Python's float floor-division):
 *     n    = max(1, (int) trunc(((buffer_len_bottom + h) + buffer_len_top) / segment_len))
 *     ze   = min(zone_start0 + (int) (h // segment_len), n);     zs = min(zone_start0, ze)
 *     az_s = min(zs, n - 1);   az_e = min(ze, n)
 *     ct   = min(n - 1, (int) trunc(((buffer_len_bottom + h) + contact_offset_top) / segment_len));  ct = min(n - 1, max(ct, ze))
 *     cb   = max(0, min(contact_bottom0, zs - 1))
 *     rows: HEIGHT = h, CAVITY_COEFF = PI_R * h, KERF_BASE / K_COND / TUF / A_SURF / S_AREA / JOULE_GEOM from the table;
 *           N_SEG = n, ZONE_START = zs, AZ_START = az_s, AZ_END = az_e, CONTACT_BOTTOM = cb, CONTACT_TOP = ct.
 *   zone_start0 = int(buffer_len_bottom // segment_len) and contact_bottom0 = max(0, int((buffer_len_bottom -
 *   contact_offset_bottom) / segment_len)) are the caller's (they do not depend on the environment).                     */
enum wedm_geomc_field {
    WEDM_GC_K_COND = 0, WEDM_GC_TUF, WEDM_GC_A_SURF, WEDM_GC_S_AREA, WEDM_GC_JOULE_GEOM, WEDM_GC_KERF_BASE, WEDM_GC_PI_R,
    WEDM_GEOMC_COUNT
};
typedef struct wedm_geom_derive_desc {
    double segment_len, buffer_len_bottom, buffer_len_top, contact_offset_top;   /* [mm], WireModuleParameters */
    int32_t zone_start0, contact_bottom0;
    int32_t num_envs, n_seg_max;   /* n_seg_max: the capacity of the wire block the rows are for */
    int64_t stride;                /* of geom_f64 and geom_i32 */
    const double* combo;           /* device, [n_materials * n_diameters][WEDM_GEOMC_COUNT] */
    int32_t n_diameters, n_materials;
    double* geom_f64;              /* device, [WEDM_GEOM_F64_COUNT][stride] */
    int32_t* geom_i32;             /* device, [WEDM_GEOM_I32_COUNT][stride] */
} wedm_geom_derive_desc;

/* For every environment e < num_envs with mask[e] != 0 (mask == NULL: all) column e of the 14 geometry rows is written as
 * above from height[e], diameter_idx[e] and material_idx[e] (material_idx == NULL: 0).  One launch on `stream`.  Stateless
 * like wedm_copy_columns: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory, read before the call
 * returns; height, diameter_idx, material_idx, mask and status are device pointers with one element per environment (status:
 * one word).  The mask is a device array because the caller may hold it without ever having read it.
 * Checked on the device: a height that is NaN, infinite or <= 0 ORs 1 into *status; else a height whose n would exceed
 * n_seg_max ORs 2 (tested in float64, before the conversion: such a row would send a step kernel past its wire); an index
 * outside the table ORs 4.  Any of them leaves the 14 values of that column as they were (status == NULL: skipped silently).
 * Never written: columns [num_envs, stride), unmasked columns, anything outside the two blocks.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)): desc, height, diameter_idx, combo, geom_f64 or geom_i32 NULL; geom_f64,
 * combo or height not 8-byte aligned; num_envs < 1; stride < num_envs; n_seg_max outside [1, 2^29]; n_diameters or
 * n_materials < 1; a segment_len that is not finite and positive; a buffer length that is not finite and >= 0; a
 * contact_offset_top that is not finite; zone_start0 or contact_bottom0 outside [0, 2^29].                              */
int32_t wedm_derive_geometry(const wedm_geom_derive_desc* desc, const double* height, const int32_t* diameter_idx,
                             const int32_t* material_idx, const uint8_t* mask, int32_t* status, void* stream);

/* ------------------------------------------- seeded per-episode domain randomisation, drawn on the device (one launch)
 * A sampler is a 64-bit seed, a table of WEDM_DRAW_SLOTS slots and one int32 draw_count[stride] device array.  What
 * environment e, of global id g = env_id_offset + e (mod 2^32), receives for its k-th draw is a pure function of (seed, g, k):
 * no batch size, rank, launch shape or call history enters it.  With k = draw_count[e] before the call, the variate of slot s
 * is word (s & 3) -- x, y, z, w in that order -- of
 *     W(q) = Philox4x32-10(counter = {k, 0, g, 0x80000000 + q}, key = {seed & 0xffffffff, seed >> 32}),   q = s >> 2,
 * the generator of the step kernels (counter {time, episode, global env id, stream}; multipliers 0xD2511F53 on word 0 and
 * 0xCD9E8D57 on word 2, Weyl key increments 0x9E3779B9 / 0xBB67AE85, ten rounds).  The physics uses streams 0 .. 64 of that
 * counter, so a draw never repeats a variate of the physics, whatever the two seeds are.
 * Slots are fixed: enabling one more never changes another's draw.  Slot s < 15 is user-facing physics parameter s in the
 * order of enum wedm_draw_slot_id (the row order of envp_src); 15 the wire material; 16 the workpiece height; 17 the index of
 * the wire diameter.  A slot's kind says what is made of its word w (uint32):
 *   WEDM_DRAW_NONE     nothing is drawn and nothing is written for that name;
 *   WEDM_DRAW_UNIFORM  (slots 0 .. 14 and 16) float64, no contraction:  u = ((double) w + 0.5) * 2^-32;  x = lo + span * u
 *                      (span = hi - lo, computed by the caller);  x = min(max(x, lo), hi).  For WEDM_DS_OMEGA_N the low 27
 *                      bits of x's mantissa are then cleared, so that x * x is exact and equals C pow(x, 2);
 *   WEDM_DRAW_CHOICE   (slots 15 and 17) i = (uint32) (((uint64) w * k) >> 32), one of k values; no float is involved.
 * For every environment e < num_envs with mask[e] != 0 (mask == NULL: all) the call writes, in column e only:
 *   envp_src[s][e] = x for every drawn slot s < 15, and every row of envp_rows that depends on a drawn name:
 *     the row of the same meaning = x (WEDM_EP_OMEGA_N too);   DEBRIS_REMOVAL_PER_US = eff * base_flow_rate * 1e-6;
 *     DAMPING_COEFF = -2.0 * zeta * omega_n (when either is drawn);   STIFFNESS_COEFF = -(omega_n * omega_n);
 *     MAX_JERK_DT = max_jerk * dt_s  -- left to right, an operand that is not drawn read from envp_src;
 *   material_index[e] = i of slot 15, the WEDM_WMAT_COUNT rows wmat_rows[r][e] = wmat_table[i][r][e] and, when `dynamic` is
 *     0, the WEDM_GEOM_F64_COUNT rows geom_f64[r][e] = wmat_geom_table[i][r][e];
 *   height[e] = x of slot 16, diameter_index[e] = i of slot 17 and, when `dynamic` is 1 and any of the slots 15 .. 17 is
 *     drawn, the 8 + 6 geometry rows of wedm_derive_geometry (descriptor `geom`) for the environment's height, diameter index
 *     and material index (drawn or stored; material 0 when material_index == NULL);
 *   draw_count[e] = k + 1.
 * Never written: unmasked columns, columns [num_envs, stride), anything outside the named blocks.  No block is gathered
 * again across the stride.  The ranges are checked on the host so that no derivation can be refused: *geom_status is ORed
 * only if a STORED height or index is bad (the bits of wedm_derive_geometry).                                             */
enum wedm_draw_slot_id {
    WEDM_DS_BASE_CRITICAL_DENSITY = 0, WEDM_DS_GAP_COEFFICIENT, WEDM_DS_MAX_CRITICAL_DENSITY, WEDM_DS_HARD_SHORT_GAP,
    WEDM_DS_SIGMOID_STEEPNESS, WEDM_DS_SPARK_VOLTAGE_FACTOR, WEDM_DS_DEBRIS_REMOVAL_EFFICIENCY, WEDM_DS_DIELECTRIC_TEMPERATURE,
    WEDM_DS_PLASMA_EFFICIENCY, WEDM_DS_BASE_CONVECTION_COEFFICIENT, WEDM_DS_OMEGA_N, WEDM_DS_ZETA, WEDM_DS_MAX_ACCELERATION,
    WEDM_DS_MAX_JERK, WEDM_DS_MAX_SPEED,
    WEDM_DS_MATERIAL, WEDM_DS_HEIGHT, WEDM_DS_DIAMETER,
    WEDM_DRAW_SLOTS
};
#define WEDM_DRAW_ENVP_SLOTS 15          /* rows of envp_src */
#define WEDM_DRAW_STREAM0 0x80000000u    /* Philox stream of call q: WEDM_DRAW_STREAM0 + q */
enum wedm_draw_kind { WEDM_DRAW_NONE = 0, WEDM_DRAW_UNIFORM = 1, WEDM_DRAW_CHOICE = 2 };
typedef struct wedm_draw_slot {
    int32_t kind;          /* enum wedm_draw_kind */
    int32_t k;             /* CHOICE: the number of values (>= 1) */
    double lo, hi, span;   /* UNIFORM: the bounds and hi - lo */
} wedm_draw_slot;
typedef struct wedm_draw_desc {
    uint64_t seed;
    uint32_t env_id_offset;        /* global id of environment 0 */
    int32_t num_envs;
    int64_t stride;                /* of every per-environment block and array below */
    wedm_draw_slot slot[WEDM_DRAW_SLOTS];
    double base_flow_rate, dt_s;   /* the uniform operands of the derived rows */
    double* envp_src;              /* device, [WEDM_DRAW_ENVP_SLOTS][stride]; needed when a slot < 15 is drawn */
    double* envp_rows;             /* device, [WEDM_ENVP_COUNT][stride]; the same */
    int64_t* material_index;       /* device, [stride]; needed when slot 15 is drawn, read otherwise (NULL: material 0) */
    const double* wmat_table;      /* device, [k of slot 15][WEDM_WMAT_COUNT][stride]; needed when slot 15 is drawn */
    double* wmat_rows;             /* device, [WEDM_WMAT_COUNT][stride]; the same */
    const double* wmat_geom_table; /* device, [k of slot 15][WEDM_GEOM_F64_COUNT][stride]; slot 15 drawn and dynamic == 0 */
    double* geom_f64;              /* device, [WEDM_GEOM_F64_COUNT][stride]; the same (dynamic == 1: geom.geom_f64 is used) */
    double* height;                /* device, [stride]; dynamic == 1 */
    int32_t* diameter_index;       /* device, [stride]; dynamic == 1 */
    int32_t* geom_status;          /* device, one word, or NULL; dynamic == 1 */
    int32_t dynamic;               /* 1: geometry rows are derived (wedm_derive_geometry's `geom`); 0: selected from the table */
    int32_t reserved;
    wedm_geom_derive_desc geom;    /* dynamic == 1; its num_envs and stride must equal this descriptor's */
} wedm_draw_desc;

/* One launch on `stream`.  Stateless like wedm_derive_geometry: no wedm_ctx, the current device, caller-owned memory.  `desc`
 * is HOST memory, read before the call returns; mask (uint8 per environment, or NULL) and draw_count are device pointers.
 * A descriptor with no drawn slot still advances the counts under the mask.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc or draw_count NULL; num_envs < 1; stride < num_envs;
 * a kind that its slot does not take; a UNIFORM slot whose lo, hi or span is not finite, or lo > hi; a CHOICE slot with
 * k < 1; a block that a drawn slot needs NULL or not aligned to its element; slots 16 or 17 drawn with dynamic == 0; with
 * dynamic == 1: a `geom` that wedm_derive_geometry would refuse or whose num_envs / stride differ, k of slot 15 other than
 * geom.n_materials, k of slot 17 above geom.n_diameters, a height range with lo <= 0 or whose hi has more than n_seg_max
 * cells.                                                                                                                 */
int32_t wedm_draw_episode(const wedm_draw_desc* desc, const uint8_t* mask, int32_t* draw_count, void* stream);

/* ---------------------------------------------------- running observation and reward normalisation, reduced on the device
 * What a policy is fed: the observation columns standardised by running moments over every environment and every step so
 * far, the reward scaled by the running deviation of the discounted return, and the episode return / length bookkeeping
 * (Gymnasium's NormalizeObservation, NormalizeReward and RecordEpisodeStatistics), without leaving the device.  This is the
 * one reduction ACROSS environments of this ABI, and it is defined so that its bits depend on the values and their global
 * environment indices alone: not on block size, grid, scheduling, or on how a batch is split over devices.
 *
 * COLUMNS.  C = D + 1: the D observation columns (plane 0's rows, then plane 1's), then the discounted return.
 * MOMENTS.  A triple (n, m, S) of float64: count, mean, sum of squared deviations.  EMPTY = (0, 0, 0); the leaf of a value x
 *   is (1, (double) x, 0).
 * MERGE.  merge(a, b), every operation rounded to float64, nothing fused, in this order with these parentheses:
 *     nb == 0: a;   na == 0: b;   otherwise
 *     n = na + nb;   d = mb - ma;   m = ma + d * (nb / n);   S = Sa + Sb + d * d * (na * nb / n).
 *   merge is not commutative in its bits: the left argument is always the node of the lower index.
 * BATCH MOMENT of a column: the pairwise tree over the leaves by GLOBAL environment index g = 256 * tile_offset + e.  Level 0
 *   is the leaves (EMPTY for an environment the mask leaves out, and past the batch's end); node j of level k + 1 is
 *   merge(node 2j, node 2j + 1) of level k; the tree is padded with EMPTY to a power of two.  EMPTY is merge's identity (it
 *   returns the other argument's bits), so the padding changes nothing.  A TILE is 256 consecutive environments (eight
 *   levels); tile t's node is partials[t]; the levels above run over the tile index.
 * RUNNING STATISTICS, per column: stats_out = merge(stats_in, batch); var = S / n.  A fresh normaliser holds (1e-4, 0, 1e-4):
 *   count 1e-4, mean 0, variance 1.
 * PER ENVIRONMENT, in a call with WEDM_NORM_STEP, for the environments the mask includes (mask == NULL: all), float64:
 *     ret = ret * gamma + (double) reward          -- this new ret is the leaf of column D
 *     ep_return += (double) reward;   ep_length += 1
 *     where terminated | truncated:  last_return = ep_return;  last_length = ep_length;  ep_count += 1;  finished = 1;
 *                                    then ep_return = 0, ep_length = 0, ret = 0;      elsewhere finished = 0.
 *   An environment the mask leaves out keeps every one of these rows.
 * OUTPUTS, for every environment below num_envs, masked or not, from stats_out:
 *     obs_out[e][c] = (float) clamp(((double) x - m_c) / sqrt(var_c + eps), -clip_obs, clip_obs); x itself where skip[c] != 0;
 *     reward_out[e] = (float) clamp((double) reward / sqrt(var_D + eps), -clip_reward, clip_reward)   (WEDM_NORM_STEP only),
 *   clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v): a clip of +inf clips nothing.  obs_out is row-major [num_envs][D].
 * FLAGS.
 *   WEDM_NORM_UPDATE  absent: stats_out = stats_in (evaluation mode); no partial is read or written.
 *   WEDM_NORM_STEP    absent: observation only, as after a reset: the leaves of column D are EMPTY (its statistics pass
 *                     through), no reward is written, no per-environment row is read or written.
 *   WEDM_NORM_REDUCE / WEDM_NORM_APPLY  the two phases of a call; neither set means both, in this order.
 *                     REDUCE updates ret and writes this batch's tile partials at partials[tile_offset + t], t < ceil(num_envs / 256).
 *                     APPLY folds all n_tiles_total partials and writes stats_out, the outputs and the episode rows (it reads
 *                     the ret REDUCE left and zeroes it where an episode ended).  Each phase runs once per shard per step:
 *                     a sharded batch reduces every shard into its own tiles of one workspace (an all-gather of
 *                     [tiles][3][C] doubles between devices) and then applies every shard: statistics and outputs carry
 *                     the bits of the whole-batch call.  A shard that is not the last holds a multiple of 256 environments.
 * A NaN input makes the numbers it reaches unspecified; it never makes the call touch memory outside its blocks.        */
#define WEDM_NORM_MAX_COLUMNS 160   /* C = D + 1 <= 160: 16 environment columns + the 132 rows of a 64-bin wire profile fit */
#define WEDM_NORM_MAX_TILES 4096    /* n_tiles_total <= 4096: 1 048 576 environments over all shards */
#define WEDM_NORM_TILE 256
enum wedm_norm_flag { WEDM_NORM_UPDATE = 1, WEDM_NORM_STEP = 2, WEDM_NORM_REDUCE = 4, WEDM_NORM_APPLY = 8 };
enum wedm_norm_moment { WEDM_NM_COUNT = 0, WEDM_NM_MEAN, WEDM_NM_M2, WEDM_NORM_MOMENTS };
typedef struct wedm_norm_plane {
    const float* rows;   /* [n_rows][stride], struct-of-arrays as the environment's obs block and the wire-profile block lie */
    int32_t n_rows;      /* plane 1 may have 0 rows (rows is then not read) */
    int32_t reserved;
    int64_t stride;      /* >= num_envs */
} wedm_norm_plane;
typedef struct wedm_norm_desc {
    wedm_norm_plane plane[2];      /* D = plane[0].n_rows + plane[1].n_rows, in [1, WEDM_NORM_MAX_COLUMNS - 1] */
    const float* reward;           /* [num_envs]; STEP */
    const uint8_t* terminated;     /* [num_envs]; STEP */
    const uint8_t* truncated;      /* [num_envs]; STEP */
    const uint8_t* mask;           /* [num_envs] or NULL: every environment takes part */
    const uint8_t* skip;           /* [D] or NULL: no column is skipped */
    float* obs_out;                /* [num_envs][D] */
    float* reward_out;             /* [num_envs]; STEP */
    double* ret;                   /* [num_envs] each; STEP */
    double* ep_return;
    double* last_return;
    int32_t* ep_length;
    int32_t* last_length;
    int32_t* ep_count;
    uint8_t* finished;
    const double* stats_in;        /* [WEDM_NORM_MOMENTS][C] */
    double* stats_out;             /* [WEDM_NORM_MOMENTS][C]; must not overlap stats_in */
    double* partials;              /* [n_tiles_total][WEDM_NORM_MOMENTS][C]; UPDATE */
    int32_t tile_offset;           /* global index of this batch's tile 0 */
    int32_t n_tiles_total;         /* tiles of the workspace: tile_offset + ceil(num_envs / 256) <= n_tiles_total <= WEDM_NORM_MAX_TILES */
    double gamma, eps, clip_obs, clip_reward;
    int32_t flags;                 /* enum wedm_norm_flag */
    int32_t num_envs;
} wedm_norm_desc;

/* At most three launches on `stream` (REDUCE: one; APPLY: the fold of the partials into stats_out, then the outputs), none
 * of which waits for another block: no spin, no cooperative launch, no floating-point atomic.  Stateless like
 * wedm_wire_profile: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory, read before the call
 * returns; everything it names is device memory.  Written: obs_out, reward_out, stats_out, partials[tile_offset ..
 * tile_offset + ceil(num_envs / 256)), elements [0, num_envs) of the per-environment rows -- nothing else, and none of the
 * source planes, whose columns [num_envs, stride) are not read either.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; a pointer that the flags need NULL (the planes'
 * rows, obs_out, stats_in, stats_out for APPLY; partials with UPDATE; reward and ret with STEP, and for APPLY with STEP
 * terminated, truncated, reward_out and the other six per-environment rows); D outside [1, WEDM_NORM_MAX_COLUMNS - 1] or a
 * negative n_rows; a stride < num_envs; stats_in and stats_out overlapping; tile_offset < 0, n_tiles_total outside
 * [1, WEDM_NORM_MAX_TILES] or the batch's tiles reaching past it; num_envs < 1; flag bits that are not defined.             */
int32_t wedm_normalize(const wedm_norm_desc* desc, void* stream);

/* ------------------------------------------------- rollout advantages and returns (GAE), computed on the device
 * What an on-policy trainer (PPO, A2C) makes of T control steps of a batch: generalised advantage estimates, returns, the
 * mask of the steps that count, and the advantages standardised over the rollout -- in float64 with every rounding fixed
 * here, so that the bits depend on the values and their global environment indices alone, as wedm_normalize's do.
 *
 * BLOCKS.  Struct-of-arrays [T][stride], environment-minor; the inputs share in_stride, the outputs out_stride, both
 *   >= num_envs; columns [num_envs, stride) are neither read nor written.
 * NEXT-STEP AUTORESET.  The step after a terminated / truncated one resets and steps in one launch: its stored observation
 *   (and value) is the FINAL observation of the finished episode -- what a truncated step bootstraps from -- but the step
 *   itself pairs an observation of episode k with a reward of episode k + 1.  WEDM_GAE_SKIP_AFTER_DONE leaves it out.
 * PER ENVIRONMENT e, for t = T - 1 down to 0, float64, every operation rounded, nothing fused, parentheses as written:
 *     done_t  = terminated[t][e] | truncated[t][e]
 *     before  = t > 0 ? done_{t-1} : prev_done_in[e]                         (prev_done_in == NULL: 0)
 *     skip_t  = (flags & WEDM_GAE_SKIP_AFTER_DONE) && before
 *     nv_t    = t == T - 1 ? (double) last_value[e] : (double) value[t+1][e]
 *     delta_t = ((double) reward[t][e] + (terminated[t][e] ? 0.0 : gamma * nv_t)) - (double) value[t][e]
 *     A_t     = skip_t ? 0.0 : delta_t + (done_t ? 0.0 : gl * A_{t+1})        gl = gamma * lambda, formed once; A_T = 0
 *     advantage[t][e] = (float) A_t;  returns[t][e] = (float) (A_t + (double) value[t][e]);  valid[t][e] = !skip_t
 *     prev_done_out[e] = done_{T-1}
 *   A truncated step bootstraps from value[t+1], a terminated one from nothing; a skipped step contributes nothing, and the
 *   done before it has already cut the chain.
 * MOMENTS (WEDM_GAE_NORMALIZE).  The environment's triple (n, m, S) is Welford over its valid steps in the order of the
 *   scan (t descending), from EMPTY:   x = (double) advantage[t][e]  (the rounded float: what APPLY reads again);
 *     n = n + 1;   d = x - m;   m = m + d / n;   S = S + d * (x - m).
 *   The batch moment is wedm_normalize's pairwise tree of these triples (its merge, the lower index on the left, padded
 *   with EMPTY) by GLOBAL environment index 256 * tile_offset + e: tile t's node is partials[tile_offset + t], the levels
 *   above run over the tile index.  Then moments = (n, m, S) and
 *     advantage_norm[t][e] = valid[t][e] ? (float) (((double) advantage[t][e] - m) / sqrt(S / n + eps)) : 0;
 *   with n == 0 every advantage_norm is 0 and moments is EMPTY: no NaN.
 * FLAGS.
 *   WEDM_GAE_SKIP_AFTER_DONE  absent: no step is skipped, valid is all 1, prev_done_in is not read.
 *   WEDM_GAE_NORMALIZE        absent: partials, moments and advantage_norm are neither read nor written.
 *   WEDM_GAE_SCAN / WEDM_GAE_APPLY  the two phases; neither set means both, in this order.  SCAN writes advantage, returns,
 *                     valid, prev_done_out and (NORMALIZE) this batch's tile partials; APPLY (NORMALIZE only: without it
 *                     nothing is launched) folds all n_tiles_total partials and writes moments and advantage_norm.  A sharded
 *                     batch scans every shard into its own tiles of one workspace, then applies every shard; a shard that
 *                     is not the last holds a multiple of 256 environments.
 * A NaN input reaches numbers only; it never makes the call touch memory outside its blocks.                            */
#define WEDM_GAE_MAX_STEPS 65536
enum wedm_gae_flag { WEDM_GAE_SKIP_AFTER_DONE = 1, WEDM_GAE_NORMALIZE = 2, WEDM_GAE_SCAN = 4, WEDM_GAE_APPLY = 8 };
typedef struct wedm_gae_desc {
    const float* reward;           /* [T][in_stride] */
    const float* value;            /* [T][in_stride] */
    const float* last_value;       /* [num_envs]: the estimate at the observation after step T - 1 */
    const uint8_t* terminated;     /* [T][in_stride] */
    const uint8_t* truncated;      /* [T][in_stride] */
    const uint8_t* prev_done_in;   /* [num_envs] or NULL (zeros): done of the step before step 0 */
    float* advantage;              /* [T][out_stride] */
    float* returns;                /* [T][out_stride] */
    float* advantage_norm;         /* [T][out_stride]; NORMALIZE */
    uint8_t* valid;                /* [T][out_stride] */
    uint8_t* prev_done_out;        /* [num_envs] or NULL; may be prev_done_in */
    double* partials;              /* [n_tiles_total][WEDM_NORM_MOMENTS]; NORMALIZE */
    double* moments;               /* [WEDM_NORM_MOMENTS]; NORMALIZE, APPLY */
    int64_t in_stride;             /* >= num_envs, in elements */
    int64_t out_stride;            /* >= num_envs, in elements */
    double gamma, lam, eps;        /* lam: the lambda of the definition */
    int32_t T;                     /* in [1, WEDM_GAE_MAX_STEPS] */
    int32_t num_envs;
    int32_t tile_offset;           /* global index of this batch's tile 0 */
    int32_t n_tiles_total;         /* tile_offset + ceil(num_envs / 256) <= n_tiles_total <= WEDM_NORM_MAX_TILES */
    int32_t flags;                 /* enum wedm_gae_flag */
    int32_t reserved;
} wedm_gae_desc;

/* At most three launches on `stream` (SCAN: one; APPLY: the fold of the partials into moments, then advantage_norm), none
 * of which waits for another block: no spin, no cooperative launch, no floating-point atomic.  Stateless like
 * wedm_normalize: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory, read before the call
 * returns; everything it names is device memory.  Written: the output blocks' columns [0, num_envs) of rows [0, T),
 * prev_done_out, partials[tile_offset .. tile_offset + ceil(num_envs / 256)), moments -- nothing else.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; a pointer that the flags need NULL or not
 * aligned to its element (SCAN: reward, value, last_value, terminated, truncated, advantage, returns, valid, and partials
 * with NORMALIZE; APPLY with NORMALIZE: advantage, valid, advantage_norm, partials, moments); num_envs < 1; T outside
 * [1, WEDM_GAE_MAX_STEPS]; a stride < num_envs; tile_offset < 0, n_tiles_total outside [1, WEDM_NORM_MAX_TILES] or the
 * batch's tiles reaching past it; gamma, lam or eps not finite; flag bits that are not defined; an output block (first
 * to last byte that the call may write) overlapping an input block, other than prev_done_out with prev_done_in.          */
int32_t wedm_gae(const wedm_gae_desc* desc, void* stream);

/* ------------------------------------------------- policy action head: sample, log-probability, gradient
 * What stands between a policy network's output row and the environment's action, and what an on-policy update evaluates
 * again at the stored actions: four bounded continuous leaves (servo, target_voltage, ON_time, OFF_time: a tanh-squashed
 * Gaussian each, mapped affinely to [lo, hi]) and current_mode, one of M listed modes (a categorical) -- in float64 on
 * the float32 inputs, every operation rounded, nothing fused, parentheses as written, exp and log the portable ones of the
 * kernels (IEEE basic operations only: the CPU oracle's wedm_oracle_exp / wedm_oracle_log with MATH_PORTABLE), so that a
 * sampled action is a pure function of (seed, global environment id, step number t, the row) and its bits do not depend
 * on the launch, on how a batch is sharded or on the device.
 *
 * ROW r: P = 8 + M float32 at params + r * param_stride:  mu_0..3, ls_0..3 (log standard deviations, used as given),
 *   l_0..M-1 (logits).  The stored action of the row is u_0..3 (float32, the PRE-SQUASH values, u + 4 r) and
 *   k = mode_index[r], clamped to [0, M - 1] before any use.
 * CONSTANTS.  LN2 = 0.6931471805599453, HALF_LOG_2PI = 0.9189385332046727, HALF_LOG_2PIE = 1.4189385332046727 (the
 *   doubles nearest to these decimals).  span_i = hi_i - lo_i, formed on the device; log_span_i is passed in (the host
 *   computes log(hi_i - lo_i) once; device and host definition use the passed value).
 * CONTINUOUS COMPONENT i (mu, ls, u: the row's values as doubles):
 *     sigma = pexp(ls);   z = (u - mu) / sigma
 *     a = |u|;   e = pexp(-2.0 * a);   s = u >= 0 ? 1.0 / (1.0 + e) : e / (1.0 + e)              (= (tanh(u) + 1) / 2)
 *     x = lo + span * s;   x = x > lo ? x : lo;   action_i = x < hi ? x : hi            (a NaN becomes lo: always in bounds)
 *     logjac = ((log_span + LN2) - 2.0 * a) - 2.0 * plog(1.0 + e)                                     (log |d action / d u|)
 *     c_i = (((-0.5 * z) * z - ls) - HALF_LOG_2PI) - logjac
 *   pexp = portable_exp; plog(x) = x is NaN ? x : portable_log(x) (portable_log reads its argument's bits).
 * MODE.
 *     m = l_0;  for j = 1 .. M - 1: m = l_j > m ? l_j : m                                      (a NaN logit is never taken)
 *     d_j = l_j - m;   w_j = pexp(d_j);   W = 0.0, S = 0.0;  for j = 0 .. M - 1: W = W + w_j, S = S + w_j * d_j
 *     logW = plog(W);   logp_j = d_j - logW;   p_j = w_j / W;   H = logW - S / W
 * OUTPUTS.  f32(x) = x is NaN ? the float32 with bits 0x7FC00000 : (float) x  -- every float32 this call stores goes
 *   through it, so a NaN carries no sign or payload of the operation that made it.
 *     log_prob[r] = f32((((c_0 + c_1) + c_2) + c_3) + logp_k)
 *     entropy[r]  = f32(((((ls_0 + HALF_LOG_2PIE) + (ls_1 + HALF_LOG_2PIE)) + (ls_2 + HALF_LOG_2PIE)) + (ls_3 + HALF_LOG_2PIE)) + H)
 *   The entropy is that of the base Gaussian plus the categorical's, not of the squashed variable (which has no closed form).
 * WEDM_HEAD_SAMPLE (rows == the batch's environments; g = env_id_offset + r modulo 2^32).  Philox4x32-10 of the step
 *   kernels: key {seed & 0xffffffff, seed >> 32}, counter {t & 0xffffffff, t >> 32, g, stream}; t: the caller's 64-bit step
 *   number.  Streams from 0xC0000000 are the head's (the physics uses 0 .. 64, wedm_draw_episode 0x80000000 ..).
 *     n_i = the polar method of the step kernels (its 53-bit pairs, v1 * sqrt(-2.0 * portable_log(q) / q) at the first
 *           attempt j < 64 with 0 < q < 1, else 0.0) on streams 0xC0000000 + 64 i + j
 *     u_i = f32(mu_i + sigma_i * n_i)         -- everything else (the action, log_prob) is computed from this rounded u_i
 *     v = ((double) word x of stream 0xC0000000 + 256 + 0.5) * 2^-32;   tau = v * W
 *     k = the first j with c_j > tau, where c_0 = 0.0 + w_0, c_j = c_{j-1} + w_j;  none: M - 1
 *   WEDM_HEAD_DETERMINISTIC: u_i = mu_i;  k = 0, b = l_0;  for j = 1 .. M - 1: if (l_j > b) b = l_j, k = j (the first
 *   largest; none compares greater: 0).  Nothing is drawn.
 *   Written: action[i][r] = action_i (float64), current_mode[r] = modes[k], u, mode_index[r] = k, log_prob, entropy.
 * WEDM_HEAD_EVALUATE reads params, u, mode_index; writes log_prob, entropy.
 * WEDM_HEAD_BACKWARD reads the same, g_log_prob[r] and g_entropy[r] (float32; g_entropy NULL: 0.0) as doubles glp, gen;
 *   writes grad_params + r * grad_stride, P float32:
 *     d mu_i = f32(glp * (z / sigma));   d ls_i = f32(glp * (z * z - 1.0) + gen)
 *     d l_j  = f32(glp * ((j == k ? 1.0 : 0.0) - p_j) - gen * (p_j * (logp_j + H)))
 * Columns [P, stride) of params and grad_params are neither read nor written.  A NaN or an infinity in a row reaches
 * numbers only: no index is formed from data without a clamp.                                                           */
#define WEDM_HEAD_MAX_MODES 19
#define WEDM_HEAD_STREAM0 0xC0000000u
enum wedm_head_op { WEDM_HEAD_SAMPLE = 0, WEDM_HEAD_EVALUATE = 1, WEDM_HEAD_BACKWARD = 2 };
enum wedm_head_flag { WEDM_HEAD_DETERMINISTIC = 1 };
typedef struct wedm_head_desc {
    const float* params;           /* [rows][param_stride] */
    float* u;                      /* [rows][4], 16-byte aligned; SAMPLE writes it, the others read it */
    int32_t* mode_index;           /* [rows]; SAMPLE writes it, the others read it */
    double* action[4];             /* [rows] each: servo, target_voltage, ON_time, OFF_time; SAMPLE */
    int32_t* current_mode;         /* [rows]; SAMPLE */
    float* log_prob;               /* [rows]; SAMPLE, EVALUATE */
    float* entropy;                /* [rows]; SAMPLE, EVALUATE */
    const float* g_log_prob;       /* [rows]; BACKWARD */
    const float* g_entropy;        /* [rows] or NULL (zeros); BACKWARD */
    float* grad_params;            /* [rows][grad_stride]; BACKWARD */
    int64_t param_stride;          /* >= 8 + n_modes, in elements */
    int64_t grad_stride;           /* >= 8 + n_modes, in elements; BACKWARD */
    uint64_t seed;                 /* SAMPLE */
    uint64_t t;                    /* SAMPLE: the step number */
    double lo[4], hi[4];           /* finite, lo < hi */
    double log_span[4];            /* log(hi - lo), finite */
    int32_t modes[WEDM_HEAD_MAX_MODES]; /* the mode numbers, [0, n_modes) used */
    int32_t n_modes;               /* M, in [1, WEDM_HEAD_MAX_MODES] */
    int32_t rows;                  /* >= 1 */
    uint32_t env_id_offset;        /* SAMPLE: global id of row 0 */
    int32_t op;                    /* enum wedm_head_op */
    int32_t flags;                 /* enum wedm_head_flag; SAMPLE only */
} wedm_head_desc;

/* One launch on `stream`, one lane per row, no block waits for another: no atomic, no spin, no cooperative launch.
 * Stateless like wedm_gae: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory, read before the
 * call returns; everything it names is device memory.  Written: what the op lists above -- nothing else.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; op not one of the three; flag bits that are
 * not defined, or a flag with another op than SAMPLE; rows < 1; n_modes outside [1, WEDM_HEAD_MAX_MODES]; a stride that the op
 * uses below 8 + n_modes; a bound or log_span that is not finite, or hi <= lo; a pointer that the op needs NULL, or any
 * pointer not aligned to its element (u: to 16 bytes); an output block of the op (first to last byte that the call may
 * write) overlapping one of its input blocks.                                                                          */
int32_t wedm_policy_head(const wedm_head_desc* desc, void* stream);

/* ------------------------------------------------- PPO clipped loss and its gradient, one call per minibatch
 * What an on-policy update makes of a minibatch: the clipped surrogate, the value loss (optionally clipped), the entropy
 * bonus, their means over the rows that count, the diagnostics (approximate KL, clip fraction) and the gradient of the
 * loss with respect to the policy's parameter rows and the value estimates -- in one pass over the rows, in float64 on
 * the float32 inputs, every operation rounded, nothing fused, parentheses as written, with wedm_policy_head's pexp, plog
 * and f32.  The means are a fixed pairwise tree over the row number, so the bits of every output depend on the values
 * and the rows' order alone: not on the launch, the device or a library's reduction.
 *
 * ROWS.  B = rows.  Dense by row r: params + r * param_stride (the head's row [mu x 4, ls x 4, l x M], P = 8 + M) and
 *   value[r].  STORED inputs are read at src = index ? index[r] : r (index: int64 [B] or NULL): u + 4 src, mode_index[src]
 *   (clamped to [0, M - 1] as in the head), old_log_prob[src], advantage[src], returns[src], old_value[src] (read only with
 *   WEDM_PPO_CLIP_VALUE), valid[src] (uint8, or NULL).  n_src is the length of the stored blocks (== rows when index is
 *   NULL).  A row is LIVE iff 0 <= src < n_src and (valid == NULL or valid[src] != 0).  A src outside [0, n_src) is
 *   never dereferenced: its row is not live and is BAD.
 * A LIVE ROW (old, A, v, R, ov: old_log_prob, advantage, value, returns, old_value as doubles):
 *     lp64, ent64: the unrounded log_prob and entropy of wedm_policy_head's definition
 *     lp = (double) f32(lp64)       -- the float32 that EVALUATE stores: with old taken from SAMPLE at unchanged parameters
 *                                      lr is exactly 0 and ratio exactly 1
 *     lr = lp - old;   ratio = pexp(lr);   lo_c = 1.0 - clip;   hi_c = 1.0 + clip
 *     rc = ratio < lo_c ? lo_c : (ratio > hi_c ? hi_c : ratio)
 *     s1 = ratio * A;   s2 = rc * A;   clipped = s2 < s1
 *     pol = -(clipped ? s2 : s1);   dlp = clipped ? 0.0 : -(A * ratio)
 *     kl = (ratio - 1.0) - lr;   cf = (ratio < lo_c || ratio > hi_c) ? 1.0 : 0.0
 *     e = v - R;   vl = e * e;   dv = e
 *     WEDM_PPO_CLIP_VALUE:  d = v - ov;   dc = d < -clip_value ? -clip_value : (d > clip_value ? clip_value : d)
 *                           ec = (ov + dc) - R;   vlc = ec * ec;   if (vlc > vl) { vl = vlc;  dv = (dc == d) ? ec : 0.0; }
 *     vloss = 0.5 * vl
 *   Every comparison is the chain as written: a NaN falls through it as the text says, not as fmin would have it.
 * SUMS.  Seven doubles per row, [live, bad, pol, vloss, ent64, kl, cf] (live and bad: 1.0 or 0.0); a row that is not live
 *   holds +0.0 in all but its bad flag.  Each is added by the pairwise tree over r with plain additions, the lower index on
 *   the left: rows are padded with +0.0 to tiles of 256; a tile's eight levels come first (tile t's node is
 *   partials[t][0 .. 7)), then the pairwise tree over the tile index, padded with +0.0 to the smallest power of two that
 *   holds the tiles.  tiles = ceil(rows / 256) <= WEDM_NORM_MAX_TILES.
 * STATS.  stats[8] = [n, n_bad, loss, policy_loss, value_loss, entropy, approx_kl, clip_fraction]:  n and n_bad are the
 *   sums of live and bad;  s = n > 0 ? 1.0 / n : 0.0;  the five means are sum * s;
 *   loss = (policy_loss + vf_coef * value_loss) - ent_coef * entropy.  With n == 0 everything is 0: no NaN.
 * GRADIENT of loss (the float32 rounding of lp taken as the identity), written only where the pointer is given:
 *     live row:  grad_params + r * grad_stride, P float32: WEDM_HEAD_BACKWARD's formulas with glp = dlp * s and
 *                gen = -ent_coef * s, each entry rounded once through f32;  grad_value[r] = f32((vf_coef * dv) * s)
 *     other rows: zeros in both.   Columns [P, grad_stride) are not touched.
 * A NaN is stored in partials and stats as 0x7FF8000000000000 and in a float32 as 0x7FC00000.
 * PHASES.  s must be known before a gradient is written.  Without valid and without index n == rows and the call is MAIN
 *   (the rows: partials and the gradient) then FOLD (partials -> stats).  Otherwise COUNT comes first: it zeroes count[0 .. 2)
 *   and counts the live rows into count[0] and the bad ones into count[1] with integer atomics (order-free), and MAIN
 *   reads count[0].  WEDM_PPO_COUNT / _MAIN / _FOLD select phases; none set means all, in this order.  COUNT without valid
 *   and index launches nothing.                                                                                         */
#define WEDM_PPO_SUMS 7
#define WEDM_PPO_STATS 8
#define WEDM_PPO_COUNT_WORDS 2
enum wedm_ppo_flag { WEDM_PPO_CLIP_VALUE = 1, WEDM_PPO_COUNT = 2, WEDM_PPO_MAIN = 4, WEDM_PPO_FOLD = 8 };
enum wedm_ppo_sum { WEDM_PS_LIVE = 0, WEDM_PS_BAD, WEDM_PS_POLICY, WEDM_PS_VALUE, WEDM_PS_ENTROPY, WEDM_PS_KL, WEDM_PS_CLIPPED };
enum wedm_ppo_stat { WEDM_PT_N = 0, WEDM_PT_N_BAD, WEDM_PT_LOSS, WEDM_PT_POLICY, WEDM_PT_VALUE, WEDM_PT_ENTROPY, WEDM_PT_KL,
                     WEDM_PT_CLIP_FRACTION };
typedef struct wedm_ppo_desc {
    const float* params;           /* [rows][param_stride] */
    const float* value;            /* [rows] */
    const int64_t* index;          /* [rows] or NULL: src = r */
    const float* u;                /* [n_src][4], 16-byte aligned */
    const int32_t* mode_index;     /* [n_src] */
    const float* old_log_prob;     /* [n_src] */
    const float* advantage;        /* [n_src] */
    const float* returns;          /* [n_src] */
    const float* old_value;        /* [n_src]; CLIP_VALUE */
    const uint8_t* valid;          /* [n_src] or NULL: every row in range is live */
    float* grad_params;            /* [rows][grad_stride] or NULL */
    float* grad_value;             /* [rows] or NULL */
    double* partials;              /* [ceil(rows / 256)][WEDM_PPO_SUMS]; MAIN writes, FOLD reads */
    double* stats;                 /* [WEDM_PPO_STATS]; FOLD */
    int32_t* count;                /* [WEDM_PPO_COUNT_WORDS]: live and bad rows; with valid or index: COUNT writes, MAIN reads */
    int64_t param_stride;          /* >= 8 + n_modes, in elements */
    int64_t grad_stride;           /* >= 8 + n_modes, in elements */
    int64_t n_src;                 /* >= 1 */
    double clip, vf_coef, ent_coef, clip_value; /* finite; clip >= 0, clip_value >= 0 */
    double lo[4], hi[4];           /* finite, lo < hi */
    double log_span[4];            /* log(hi - lo), finite */
    int32_t n_modes;               /* M, in [1, WEDM_HEAD_MAX_MODES] */
    int32_t rows;                  /* >= 1, at most WEDM_NORM_MAX_TILES * 256 */
    int32_t flags;                 /* enum wedm_ppo_flag */
    int32_t reserved;
} wedm_ppo_desc;

/* At most four launches on `stream` with valid or index (COUNT: two; MAIN; FOLD) and two without, none of which waits for
 * another block: no spin, no cooperative launch, no floating-point atomic.  Stateless like wedm_policy_head: no wedm_ctx,
 * the current device, caller-owned memory.  `desc` is HOST memory, read before the call returns; everything it names is
 * device memory.  Written: grad_params' columns [0, P) of rows [0, rows), grad_value, partials, stats, count -- each by its
 * phase, nothing else.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined; rows < 1 or
 * more than WEDM_NORM_MAX_TILES tiles; n_src < 1; n_modes outside [1, WEDM_HEAD_MAX_MODES]; a stride below 8 + n_modes;
 * clip, vf_coef, ent_coef, clip_value, a bound or a log_span that is not finite; clip < 0 or clip_value < 0; hi <= lo; a
 * needed pointer NULL (params, value, u, mode_index, old_log_prob, advantage, returns and partials for MAIN; old_value with
 * CLIP_VALUE; partials and stats for FOLD; count with valid or index for COUNT and MAIN); a pointer not aligned to its
 * element (u: 16 bytes; index, partials, stats: 8); an output block (first to last byte that the call may write)
 * overlapping an input block.                                                                                          */
int32_t wedm_ppo_loss(const wedm_ppo_desc* desc, void* stream);

/* ------------------------------------------------- the actor-critic network: forward and backward, defined to the bit
 * A two-hidden-layer MLP between an observation row and the head's parameter row plus a value estimate.  Every value is a
 * float32, every fma below is ONE IEEE float32 fused multiply-add, every other operation is a float32 operation rounded
 * once, parentheses as written.  The definition is a set of k-ordered fma chains, which is what gfx950's float32 matrix
 * instructions compute and what a CPU reproduces: the bits of every output depend on the values and the rows' order alone.
 *
 * SHAPES.  D observation columns, 1 <= D <= WEDM_NORM_MAX_COLUMNS;  H1, H2 multiples of 16 in [16, WEDM_NET_MAX_HIDDEN];
 *   P = 8 + n_modes;  O = P + 1 in [10, 28].
 * PARAMETERS.  theta is one flat block without padding: W1[D][H1], b1[H1], W2[H1][H2], b2[H2], W3[H2][O], b3[O], matrices
 *   row-major with the input index k outermost.  n_theta = (D + 1) H1 + (H1 + 1) H2 + (H2 + 1) O.  A gradient has the
 *   same layout.
 * ROWS.  src = index ? index[r] : r.  A src outside [0, n_src) is never dereferenced: the row's inputs x_k are +0.0 and its
 *   incoming gradient go_j is +0.0; the chains run as written for such a row.
 * INPUT.  o = obs[src * obs_stride + k];   x_k = (o != o) ? +0.0 : (o < -FLT_MAX ? -FLT_MAX : (o > FLT_MAX ? FLT_MAX : o))
 * LAYER (in[K], W[K][N], b[N]) -> a[N]:   a_j = b_j;  for k = 0 .. K - 1:  a_j = fma(in_k, W[k][j], a_j)
 *   h1 = act(layer(x, W1, b1));   h2 = act(layer(h1, W2, b2));   out = layer(h2, W3, b3)
 *   params[r * param_stride + j] = out_j for j < P;   value[r] = out_P.
 * ACTIVATION (descriptor field `activation`).
 *   WEDM_NET_RELU:  act(a) = a > 0 ? a : +0.0;   act'(h) = h > 0 ? 1.0f : 0.0f
 *   WEDM_NET_TANH:  act'(h) = fma(-h, h, 1.0f), and act(a) is, with u(x) the bits of x and f(b) the float of bits b:
 *     m  = f(u(a) & 0x7FFFFFFF);           z = m + m
 *     t  = fma(z, 0x1.715476p+0f, 12582912.0f);   n = t - 12582912.0f       -- n = round(z log2 e), its integer in t's bits
 *     r  = fma(n, -0x1.62e400p-1f, z);     r = fma(n, -0x1.7f7d1cp-20f, r)  -- z - n ln 2, ln 2 in two parts
 *     p  = fma(r, 0x1.a01a02p-16f, 0x1.a01a02p-13f)                         -- 1/40320, 1/5040
 *     p  = fma(r, p, 0x1.6c16c2p-10f);  p = fma(r, p, 0x1.111112p-7f);  p = fma(r, p, 0x1.555556p-5f)  -- 1/720 1/120 1/24
 *     p  = fma(r, p, 0x1.555556p-3f);   p = fma(r, p, 0.5f)                                          -- 1/6, 1/2
 *     q  = fma(r * r, p, r)                                                 -- expm1(r)
 *     s  = f((u(t) << 23) + 0x3F800000)                                     -- 2^n (32-bit wrap-around arithmetic)
 *     e  = fma(s, q, s - 1.0f);            d = e + 2.0f                     -- expm1(2 m)
 *     g  = m < 0.5f ? e / d : 1.0f - 2.0f / d;      g = m > 10.0f ? 1.0f : g
 *     act(a) = f(u(g) | (u(a) & 0x80000000))
 *   It is odd, |act(a)| <= 1, act(+-0) = +-0, it saturates to +-1 beyond |a| = 10 and a NaN gives a NaN (every comparison
 *   is false for it).  The division is the correctly rounded float32 division.
 * BACKWARD.  go[r][0 .. O) = the P entries at grad_params + r * grad_stride, then grad_value[r].  h1, h2 are recomputed by
 *   the forward definition.
 *     dh2_k = chain from +0.0 over j = 0 .. O - 1 of fma(go_j, W3[k][j], .);    da2_k = dh2_k * act'(h2_k)
 *     dh1_k = chain from +0.0 over j = 0 .. H2 - 1 of fma(da2_j, W2[k][j], .);  da1_k = dh1_k * act'(h1_k)
 *     dW3[k][j] = SUM_r (h2[r][k], go[r][j]);   dW2[k][j] = SUM_r (h1[r][k], da2[r][j]);   dW1[k][j] = SUM_r (x[r][k], da1[r][j])
 *     db3[j] = SUM_r (1.0f, go[r][j]);          db2[j] = SUM_r (1.0f, da2[r][j]);          db1[j] = SUM_r (1.0f, da1[r][j])
 * ROW SUM.  SUM_r (u_r, v_r):  rows [64 c, 64 c + 64) form chunk c, whose node is the chain from +0.0 over r ascending of
 *   fma(u_r, v_r, .); rows at or past `rows` are absent from it.  Chunk nodes are added with plain float32 additions, the
 *   lower index on the left, by wedm_ppo_loss's pairwise tree: two levels inside a tile of 256 rows (four chunks) give
 *   partials[tile][n_theta], then the tree over the tile index, padded to the smallest power of two that holds the tiles.
 *   At every level a node whose right child holds no row is its left child unchanged (no +0.0 is added, which would turn
 *   a -0.0 into +0.0).  tiles = ceil(rows / 256) <= WEDM_NORM_MAX_TILES.
 * NaN.  Every float32 the call stores (params, value, partials, grad_theta) holds a NaN as 0x7FC00000.
 * PHASES.  WEDM_NET_FORWARD: one launch, writes params' columns [0, P) and value.  WEDM_NET_BACKWARD: MAIN, one launch,
 *   rows -> partials.  WEDM_NET_FOLD: one launch, partials -> grad_theta; with WEDM_NET_ACCUMULATE
 *   grad_theta[e] = grad_theta[e] + root[e], one float32 addition, else grad_theta[e] = root[e].  At least one of the
 *   three must be set; they run in this order.                                                                          */
#define WEDM_NET_MAX_HIDDEN 128
enum wedm_net_flag { WEDM_NET_FORWARD = 1, WEDM_NET_BACKWARD = 2, WEDM_NET_FOLD = 4, WEDM_NET_ACCUMULATE = 8 };
enum wedm_net_activation { WEDM_NET_RELU = 0, WEDM_NET_TANH = 1 };
typedef struct wedm_net_desc {
    const float* theta;            /* [n_theta]; FORWARD, BACKWARD */
    const float* obs;              /* [n_src][obs_stride]; FORWARD, BACKWARD */
    const int64_t* index;          /* [rows] or NULL: src = r */
    float* params;                 /* [rows][param_stride]; FORWARD writes */
    float* value;                  /* [rows]; FORWARD writes */
    const float* grad_params;      /* [rows][grad_stride]; BACKWARD reads */
    const float* grad_value;       /* [rows]; BACKWARD reads */
    float* partials;               /* [ceil(rows / 256)][n_theta]; BACKWARD writes, FOLD reads */
    float* grad_theta;             /* [n_theta]; FOLD writes (ACCUMULATE: reads and writes) */
    int64_t obs_stride;            /* >= obs_dim, in elements */
    int64_t param_stride;          /* >= 8 + n_modes, in elements */
    int64_t grad_stride;           /* >= 8 + n_modes, in elements */
    int64_t n_src;                 /* >= 1: the rows of obs */
    int32_t obs_dim;               /* D, in [1, WEDM_NORM_MAX_COLUMNS] */
    int32_t hidden1, hidden2;      /* H1, H2: multiples of 16 in [16, WEDM_NET_MAX_HIDDEN] */
    int32_t n_modes;               /* M, in [1, WEDM_HEAD_MAX_MODES] */
    int32_t activation;            /* enum wedm_net_activation */
    int32_t rows;                  /* >= 1, at most WEDM_NORM_MAX_TILES * 256 */
    int32_t flags;                 /* enum wedm_net_flag */
    int32_t reserved;
} wedm_net_desc;

/* At most three launches on `stream` (FORWARD; BACKWARD's MAIN; FOLD), none of which waits for another block: no spin, no
 * cooperative launch, no atomic.  Stateless like wedm_ppo_loss: no wedm_ctx, the current device, caller-owned memory.
 * `desc` is HOST memory, read before the call returns; everything it names is device memory.  Written: params' columns
 * [0, P) of rows [0, rows), value, partials, grad_theta -- each by its phase, nothing else.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined or no phase;
 * rows < 1 or more than WEDM_NORM_MAX_TILES tiles; n_src < 1; obs_dim, hidden1, hidden2, n_modes or activation out of
 * range; a stride below its row's length; a needed pointer NULL (theta, obs for FORWARD and BACKWARD; params, value for
 * FORWARD; grad_params, grad_value for BACKWARD; partials for BACKWARD and FOLD; grad_theta for FOLD); a pointer not
 * aligned to its element (index: 8); an output block (first to last byte that the call may write) overlapping an input
 * block.                                                                                                               */
int32_t wedm_policy_net(const wedm_net_desc* desc, void* stream);

/* ------------------------------------------------- Adam with gradient clipping and a KL gate, one call per minibatch
 * The step from a gradient to the next parameters: the gradient's global norm by wedm_ppo_loss's pairwise tree, the clipping
 * factor, the decision whether this minibatch is applied at all (a gradient that is not finite, or an approximate KL over
 * its limit, which closes a latch for the rest of the update), Adam's moments and the decoupled weight decay of AdamW --
 * without the host ever reading a device value.  All arithmetic is float64 on the float32 inputs, every operation rounded
 * once, nothing fused, parentheses as written; f32 is wedm_policy_head's; sqrt and / are the correctly rounded float64 ones.
 * The bits of every output depend on the values and the elements' order alone.
 *
 * BLOCKS.  theta[n], m[n], v[n]: float32, read and written.  grad[n]: float32, read only.  partials[ceil(n / 256)]: double,
 *   written.  state[WEDM_OPT_STATE]: double, read and written: [B1POW, B2POW, T, SKIPPED_NONFINITE, SKIPPED_KL, LATCH, 0, 0]
 *   (enum wedm_opt_state); a fresh state is [1, 1, 0, 0, 0, 0, 0, 0].  info[WEDM_OPT_INFO]: double, written:
 *   [SUMSQ, NORM, SCALE, LR, APPLIED, KL, BC1, BC2] (enum wedm_opt_info).  kl: ONE double, read only, only with
 *   WEDM_OPT_KL_GATE (in practice &stats[WEDM_PT_KL] of wedm_ppo_loss).  1 <= n <= WEDM_NORM_MAX_TILES * 256.
 * NORM.  q_e = (double) grad[e] * (double) grad[e], which is exact.  S is the pairwise tree over e with plain additions, the
 *   lower index on the left: elements are padded with +0.0 to tiles of 256, a tile's eight levels give partials[t], then the
 *   tree over the tile index, padded with +0.0 to the smallest power of two that holds the tiles.  Every leaf is >= +0.0 or a
 *   NaN, and the sum cannot overflow a double: S < +inf holds exactly when every gradient entry is finite.
 * DECIDE, one decision per call (CLIP, KL_GATE, NEW_UPDATE: the flag is set):
 *     latch = state[LATCH];   if (NEW_UPDATE) latch = 0.0
 *     klv   = KL_GATE ? kl[0] : 0.0
 *     if (KL_GATE && latch == 0.0 && !(klv <= kl_limit)) latch = 1.0         -- a NaN closes the gate too
 *     finite = S < +inf                                                       -- false for a NaN
 *     norm = sqrt(S);   c = 1.0;   if (CLIP) { c = max_norm / (norm + 1e-6);  if (!(c < 1.0)) c = 1.0; }
 *     if (latch != 0.0)   SKIPPED_KL += 1.0
 *     else if (!finite)   SKIPPED_NONFINITE += 1.0
 *     else              { T += 1.0;  B1POW = B1POW * beta1;  B2POW = B2POW * beta2; }
 *     applied = (latch == 0.0 && finite) ? 1.0 : 0.0
 *     bc1 = 1.0 - B1POW;   bc2 = 1.0 - B2POW                                  -- from the state after the decision
 *     info = [S, norm, c, lr, applied, klv, bc1, bc2];   state[LATCH] = latch;   state[6] = state[7] = 0.0
 *   The bias corrections are running products held in the state: no pow.  The latch stays closed until a call carries
 *   NEW_UPDATE: "stop this update's remaining minibatches and epochs" without the host looking.
 * APPLY reads SCALE (c), APPLIED, BC1 and BC2 from info and the other scalars from the descriptor.  It runs only when
 *   info[APPLIED] == 1.0; otherwise no byte of theta, m, v is written.  Per element:
 *     g = (double) grad[e] * c;     p = (double) theta[e]
 *     if (weight_decay != 0.0) p = p - (lr * weight_decay) * p                -- decoupled, as AdamW
 *     mf = f32(beta1 * (double) m[e] + (1.0 - beta1) * g)
 *     vf = f32(beta2 * (double) v[e] + (1.0 - beta2) * (g * g))
 *     mh = (double) mf / bc1;    vh = (double) vf / bc2
 *     p  = p - lr * (mh / (sqrt(vh) + eps))
 *     theta[e] = f32(p);   m[e] = mf;   v[e] = vf
 *   The moments that are used are the float32 values that are stored: a resumed run sees what the uninterrupted one saw.  A
 *   gradient near FLT_MAX makes vf +inf, which stays: mh / inf = 0 and theta stands still.
 * A NaN is stored in partials, state and info as 0x7FF8000000000000 and in a float32 as 0x7FC00000.
 * PHASES.  WEDM_OPT_NORM (grad -> partials), WEDM_OPT_DECIDE (partials, kl, state -> state, info), WEDM_OPT_APPLY; none of
 *   the three set means all three, in this order.  Without a phase bit and with n <= WEDM_OPT_ONE_BLOCK_MAX the call is ONE
 *   launch of one block that does all three; any phase bit selects the launches per phase.  Both give the same bytes in every
 *   block, partials included.                                                                                             */
#define WEDM_OPT_STATE 8
#define WEDM_OPT_INFO 8
/* One block against three launches is a pure speed choice (the bytes are the same).  Measured on an MI355X, back-to-back
 * calls (tools/optimizer_cost.py): one block takes 4.0 / 5.5 / 8.5 / 12.2 / 14.4 / 25.8 / 94 us at
 * n = 1 024 / 2 048 / 4 096 / 6 418 / 8 192 / 16 384 / 65 536, the three launches 8.6 to 14 us at every one of them: one
 * block wins up to 4 096 and not from 6 418 on.  A diagnostic build may define another value, at most 65 536.            */
#ifndef WEDM_OPT_ONE_BLOCK_MAX
#define WEDM_OPT_ONE_BLOCK_MAX 4096
#endif
enum wedm_opt_flag { WEDM_OPT_CLIP = 1, WEDM_OPT_KL_GATE = 2, WEDM_OPT_NEW_UPDATE = 4, WEDM_OPT_NORM = 8, WEDM_OPT_DECIDE = 16,
                     WEDM_OPT_APPLY = 32 };
enum wedm_opt_state { WEDM_OS_B1POW = 0, WEDM_OS_B2POW, WEDM_OS_T, WEDM_OS_SKIPPED_NONFINITE, WEDM_OS_SKIPPED_KL, WEDM_OS_LATCH };
enum wedm_opt_info { WEDM_OI_SUMSQ = 0, WEDM_OI_NORM, WEDM_OI_SCALE, WEDM_OI_LR, WEDM_OI_APPLIED, WEDM_OI_KL, WEDM_OI_BC1,
                     WEDM_OI_BC2 };
typedef struct wedm_opt_desc {
    float* theta;                  /* [n]; APPLY reads and writes */
    float* m;                      /* [n]; APPLY reads and writes */
    float* v;                      /* [n]; APPLY reads and writes */
    const float* grad;             /* [n]; NORM, APPLY */
    double* partials;              /* [ceil(n / 256)]; NORM writes, DECIDE reads */
    double* state;                 /* [WEDM_OPT_STATE]; DECIDE reads and writes */
    double* info;                  /* [WEDM_OPT_INFO]; DECIDE writes, APPLY reads */
    const double* kl;              /* one double; DECIDE with KL_GATE */
    double lr;                     /* finite, >= 0 */
    double beta1, beta2;           /* in [0, 1) */
    double eps;                    /* finite, > 0 */
    double weight_decay;           /* finite, >= 0 */
    double max_norm;               /* finite, > 0; CLIP */
    double kl_limit;               /* finite, >= 0; KL_GATE */
    int32_t n;                     /* >= 1, at most WEDM_NORM_MAX_TILES * 256 */
    int32_t flags;                 /* enum wedm_opt_flag */
} wedm_opt_desc;

/* One launch on `stream`, or at most three (NORM, DECIDE, APPLY: one each), none of which waits for another block: no spin,
 * no cooperative launch, no atomic.  Stateless like wedm_ppo_loss: no wedm_ctx, the current device, caller-owned memory.
 * `desc` is HOST memory, read before the call returns; everything it names is device memory.  Written: theta, m, v,
 * partials, state, info -- each by its phase, nothing else.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined; n < 1 or more
 * than WEDM_NORM_MAX_TILES tiles; lr, eps or weight_decay not finite, lr < 0, eps <= 0, weight_decay < 0; beta1 or beta2
 * outside [0, 1); with CLIP a max_norm that is not finite or <= 0; with KL_GATE a kl_limit that is not finite or < 0; a needed
 * pointer NULL (grad, partials for NORM; partials, state, info for DECIDE, and kl with KL_GATE; theta, m, v, grad, info for
 * APPLY); a pointer not aligned to its element (partials, state, info, kl: 8); an output block (theta, m, v, partials,
 * state, info: first to last byte that the call may touch) overlapping an input block (grad, kl) or another output block. */
int32_t wedm_adam(const wedm_opt_desc* desc, void* stream);

/* ------------------------------------------------- the rows of a rollout dealt into minibatches: a seeded permutation
 * Which rows go into which minibatch of an epoch, as a function of (valid, n_parts, seed, draw) alone: the same bits on every
 * device, nothing a checkpoint has to carry but three integers, the live rows spread evenly over the parts.  Integers only.
 * This is NOT a uniformly random permutation: it is a keyed bijection (a balanced Feistel network over the bits of the live
 * count, walked back into range), good enough to shuffle minibatches; the tests hold it to a chi-square of the row-by-part
 * membership counts that a uniform shuffle meets.
 *
 * BLOCKS.  valid[rows]: uint8, read only, a row is LIVE iff its byte is not zero; NULL: every row is live.  index[rows]: int64,
 *   written.  count[2]: int64, written: {V, rows - V}.  tile_counts[tiles], tile_base[tiles]: int32, the workspace, with
 *   tiles = ceil(rows / WEDM_MB_TILE).  1 <= rows <= WEDM_MB_MAX_ROWS, 1 <= n_parts <= min(rows, WEDM_MB_MAX_PARTS).
 * RANKS.  V is the number of live rows.  k(r), for a live row r, is the number of live rows below r; q(r), for a dead row r,
 *   the number of dead rows below r.
 * KEYS.  K[4 c + i], c = 0, 1, is word i of Philox4x32-10 with key (seed lo, seed hi) and counter (draw lo, draw hi, 0,
 *   WEDM_MB_STREAM0 + c).
 * E, a bijection of [0, 2^b), where b is the bit length of V - 1 (b = 0 for V <= 1): hl = b >> 1, hh = b - hl,
 *   lo = x & (2^hl - 1), hi = x >> hl; rounds i = 0 ... 7, an even one hi ^= mix(lo ^ K[i]) & (2^hh - 1), an odd one
 *   lo ^= mix(hi ^ K[i]) & (2^hl - 1); E(x) = hi << hl | lo.  mix is the 32-bit finaliser
 *     x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16.
 *   Every round is an xor of one half with a function of the other: a bijection for every b, odd widths and b = 1 included.
 * PI, the permutation of [0, V) by cycle walking: PI(k) is the first of E(k), E(E(k)), ... that is below V.  The walk ends
 *   (k lies on its own cycle and k < V), and since 2^b < 2 V it takes under two applications on average.
 * PLACE.  The list position of row r is j(r) = PI(k(r)) for a live row and V + q(r) for a dead one.  Positions are dealt
 *   round-robin: part p = j mod n_parts, slot s = j div n_parts.  Part p holds cnt_p = ceil((rows - p) / n_parts) rows from
 *   off_p = p * (rows div n_parts) + min(p, rows mod n_parts) on -- sizes and offsets of a split of `rows` entries into
 *   n_parts as even as they go, the larger ones first, which the host knows without reading anything --, and
 *   index[off_p + s] = r.  So index is a permutation of [0, rows), in every part the live rows come first, and part p holds
 *   ceil((V - p) / n_parts) of them (zero for p >= V): the parts' live counts differ by at most one.
 * WORKSPACE.  tile_counts[t] is the number of live rows among rows [1024 t, 1024 t + 1024); tile_base[t] the sum of the
 *   counts below t.
 * PHASES.  WEDM_MB_COUNT (valid -> tile_counts), WEDM_MB_OFFSETS (tile_counts -> tile_base, count), WEDM_MB_SCATTER (valid,
 *   tile_base, count -> index); none of the three set means all three, in this order.  A SCATTER over a workspace that no
 *   COUNT and OFFSETS of the same `valid` wrote stores nothing outside index and ends: a row whose rank or position falls
 *   outside what count[0], clamped to [0, rows], allows is left out.                                                     */
#define WEDM_MB_STREAM0 0xE0000000u     /* clear of WEDM_DRAW_STREAM0 + q and WEDM_HEAD_STREAM0 + ... */
#define WEDM_MB_TILE 1024
#define WEDM_MB_MAX_ROWS (1 << 26)
#define WEDM_MB_MAX_PARTS 4096
enum wedm_mb_flag { WEDM_MB_COUNT = 1, WEDM_MB_OFFSETS = 2, WEDM_MB_SCATTER = 4 };
typedef struct wedm_mb_desc {
    const uint8_t* valid;          /* [rows] or NULL (every row live); COUNT, SCATTER */
    int64_t* index;                /* [rows]; SCATTER writes */
    int64_t* count;                /* [2]; OFFSETS writes, SCATTER reads */
    int32_t* tile_counts;          /* [ceil(rows / 1024)]; COUNT writes, OFFSETS reads */
    int32_t* tile_base;            /* [ceil(rows / 1024)]; OFFSETS writes, SCATTER reads */
    uint64_t seed;                 /* the Philox key */
    uint64_t draw;                 /* the number of this permutation */
    int32_t rows;                  /* in [1, WEDM_MB_MAX_ROWS] */
    int32_t n_parts;               /* in [1, min(rows, WEDM_MB_MAX_PARTS)] */
    int32_t flags;                 /* enum wedm_mb_flag */
} wedm_mb_desc;

/* At most three launches on `stream` (COUNT, OFFSETS, SCATTER: one each), none of which waits for another block: no spin, no
 * cooperative launch, no atomic.  Stateless like wedm_adam: no wedm_ctx, the current device, caller-owned memory.  `desc` is
 * HOST memory, read before the call returns; everything it names is device memory.  Written: index, count, tile_counts,
 * tile_base -- each by its phase, nothing else; `valid` is never written.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined; rows outside
 * [1, WEDM_MB_MAX_ROWS]; n_parts outside [1, min(rows, WEDM_MB_MAX_PARTS)]; a needed pointer NULL (tile_counts for COUNT;
 * tile_counts, tile_base, count for OFFSETS; tile_base, count, index for SCATTER); a pointer not aligned to its element (index,
 * count: 8; tile_counts, tile_base: 4; valid: any address); a block that is written or part of the workspace (index, count,
 * tile_counts, tile_base: first to last byte that the call may touch) overlapping valid or another such block.            */
int32_t wedm_minibatch_index(const wedm_mb_desc* desc, void* stream);

/* ------------------------------------------------- the log of finished episodes: an ordered ring, per-episode sums
 * One call per control step, after the step: every environment whose episode ended in it appends one RECORD to a ring of
 * `capacity` slots, in the order of the global environment index, without the host learning how many there were.
 *
 * PLANES.  A plane is a [n_rows][src_stride] block of elem_bytes 1, 4 or 8 with the environment as the column, and of a kind:
 *   WEDM_ELOG_LAST      the element as it lies when the episode ends, copied as raw words (a NaN keeps its payload);
 *                       dst is [n_rows][capacity] of elem_bytes;
 *   WEDM_ELOG_SUM_F32 / _SUM_F64 / _SUM_I32   the sum over the episode's control steps of a float (elem_bytes 4), a double
 *                       (8) or an int32_t (4) row, held in the caller's accumulator acc [n_rows][num_envs] of 8 bytes
 *                       (double; int64_t for SUM_I32); dst is [n_rows][capacity] of 8 bytes of the accumulator's type.
 *                       float:  acc = acc + (double) x   (one rounding, nothing fused);   int32: int64 addition.
 * PER ENVIRONMENT e of [0, num_envs), g = 256 * tile_offset + e its GLOBAL index (the tile convention of wedm_normalize):
 *     live(e)   = mask == NULL || mask[e] != 0
 *     finish(e) = live(e) && ((terminated[e] | (truncated == NULL ? 0 : truncated[e])) != 0)
 *   every live environment first adds this step's SUM rows to its accumulators; a finishing one then forms a record:
 *     k = the number of finishing environments of lower global index in this call
 *       = tile_counts[0] + ... + tile_counts[tile_offset + e / 256 - 1] + the finishing e' < e of e's own tile,
 *     n = tile_counts[0] + ... + tile_counts[n_tiles_total - 1]        (all finishing environments of this call),
 *     a = head[0] + k  (the record's absolute number),   slot = a mod capacity, in [0, capacity),
 *   and the record is WRITTEN iff k >= n - capacity: a call that finishes more episodes than the ring holds keeps the
 *   newest `capacity` of them, and no two lanes ever write one slot (the result does not depend on block scheduling).
 *   A written record holds, at column `slot`: every LAST row's element of column e, every SUM accumulator of e (this step
 *   included), env_out = env_id_offset + e, stamp_out = stamp.  Every finishing environment's accumulators are then zero,
 *   whether its record was written or dropped.  After all records: head[0] += n, head[1] = n.
 *   Never written: a slot no record names, an accumulator of an environment that is not live, columns [num_envs, stride),
 *   any source plane, tile_counts outside this batch's tiles.
 * PHASES, as wedm_gae has them; none of the three set means all three, in this order:
 *   WEDM_ELOG_COUNT    writes tile_counts[tile_offset + t], the finishing environments of this batch's tile t;
 *   WEDM_ELOG_SCATTER  reads head[0] and tile_counts[0 .. n_tiles_total), updates accumulators and writes records;
 *   WEDM_ELOG_COMMIT   reads tile_counts[0 .. n_tiles_total) and advances head.
 *   A sharded batch COUNTs every shard into its own tiles of one workspace, then SCATTERs every shard, then COMMITs once;
 *   a shard that is not the last holds a multiple of 256 environments.  The log then carries the bytes of the whole-batch
 *   call.  Every tile of the workspace belongs to some shard of the call: n is the sum over all of them.              */
#define WEDM_ELOG_MAX_PLANES 32
#define WEDM_ELOG_MAX_ROWS 96       /* rows of all planes together */
enum wedm_elog_kind { WEDM_ELOG_LAST = 0, WEDM_ELOG_SUM_F32 = 1, WEDM_ELOG_SUM_F64 = 2, WEDM_ELOG_SUM_I32 = 3 };
enum wedm_elog_flag { WEDM_ELOG_COUNT = 1, WEDM_ELOG_SCATTER = 2, WEDM_ELOG_COMMIT = 4 };
typedef struct wedm_elog_plane {
    const void* src;     /* [n_rows][src_stride] of elem_bytes */
    void* dst;           /* [n_rows][capacity]: LAST of elem_bytes, SUM of 8 bytes */
    void* acc;           /* SUM: [n_rows][num_envs] of 8 bytes; LAST: not read */
    int64_t src_stride;  /* >= num_envs, in elements */
    int32_t n_rows;      /* >= 1 */
    int32_t elem_bytes;  /* LAST: 1, 4 or 8; SUM_F32 and SUM_I32: 4; SUM_F64: 8 */
    int32_t kind;        /* enum wedm_elog_kind */
    int32_t reserved;
} wedm_elog_plane;
typedef struct wedm_elog_desc {
    wedm_elog_plane plane[WEDM_ELOG_MAX_PLANES];
    const uint8_t* terminated;     /* [num_envs] */
    const uint8_t* truncated;      /* [num_envs] or NULL (zeros) */
    const uint8_t* mask;           /* [num_envs] or NULL: every environment is live */
    int64_t* env_out;              /* [capacity] */
    int64_t* stamp_out;            /* [capacity] */
    int64_t* head;                 /* [2]: records appended so far; records of the last call */
    int32_t* tile_counts;          /* [n_tiles_total] */
    int64_t capacity;              /* >= 1 */
    int64_t env_id_offset;
    int64_t stamp;
    int32_t n_planes;              /* in [1, WEDM_ELOG_MAX_PLANES]; the planes' rows together at most WEDM_ELOG_MAX_ROWS */
    int32_t num_envs;
    int32_t tile_offset;           /* global index of this batch's tile 0 */
    int32_t n_tiles_total;         /* tile_offset + ceil(num_envs / 256) <= n_tiles_total <= WEDM_NORM_MAX_TILES */
    int32_t flags;                 /* enum wedm_elog_flag */
    int32_t reserved;
} wedm_elog_desc;

/* At most three launches on `stream` (COUNT, SCATTER, COMMIT: one each), none of which waits for another block: no spin, no
 * cooperative launch, no atomic of any kind.  Stateless like wedm_gae: no wedm_ctx, the current device, caller-owned memory.
 * `desc` is HOST memory, read before the call returns; everything it names is device memory.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined; num_envs < 1;
 * capacity < 1; tile_offset < 0, n_tiles_total outside [1, WEDM_NORM_MAX_TILES] or the batch's tiles reaching past it;
 * n_planes outside [1, WEDM_ELOG_MAX_PLANES]; a plane with n_rows < 1, a kind that is not defined, an elem_bytes that its
 * kind does not take (a SUM plane of 1 byte among them), or a stride below num_envs; more than WEDM_ELOG_MAX_ROWS rows in
 * all; a needed pointer NULL or not aligned to its element (terminated and tile_counts always; head for SCATTER and COMMIT;
 * env_out, stamp_out and every plane's src and dst for SCATTER, and acc of every SUM plane); an output block (first to last
 * byte that the call may write: dst, acc, env_out, stamp_out, head, tile_counts) overlapping an input block (src,
 * terminated, truncated, mask).                                                                                          */
int32_t wedm_episode_log(const wedm_elog_desc* desc, void* stream);

/* ------------------------------------------------- the shaped reward: ten weighted terms of one control step, one call
 * One call per control step, after the step's launch: every environment's reward as a weighted sum of ten TERMS read from
 * the state blocks as the launch left them, and (optionally) the ten weighted terms themselves.
 *
 * THE ACCUMULATORS, NOT THE PUBLICATIONS.  A launch of one control interval (1000 us) BEGINS with the control sample: that
 * sample publishes the *_ACC rows of the pulse and signal blocks into the *_LAST rows and restarts them, so when the launch
 * ends the *_LAST rows (and observation columns 8 ...) describe the interval BEFORE this action, and what this action caused
 * lies in the *_ACC rows: after the second of two such launches SPARK_ACC holds this launch's sparks and SPARK_LAST the
 * previous launch's; SAMPLES_ACC is 999 and SAMPLES_LAST 1001.  The terms therefore read *_ACC.  The control sample itself
 * belongs to the previous publication, so a launch of one control interval contributes the 999 samples after its control step;
 * an environment that ended inside the launch contributes what it had when it froze.
 *
 * TERMS.  x_k of environment e, in this order (enum wedm_reward_term):
 *   0 PROGRESS     f64[WEDM_F_WORKPIECE_POS][e] - p0,  p0 = (restart != NULL && restart[e] != 0) ? pos_restart : pos_before[e]
 *   1 STEP         1.0
 *   2 WIRE_BREAK   i8[WEDM_B_WIRE_BROKEN][e] != 0 ? 1.0 : 0.0
 *   3 TARGET       i8[WEDM_B_TARGET_REACHED][e] != 0 ? 1.0 : 0.0
 *   4 SPARKS       (double) pulse[WEDM_P_SPARK_ACC][e]
 *   5 SHORTS       (double) pulse[WEDM_P_SHORT_ACC][e]
 *   6 SHORT_STEPS  (double) pulse[WEDM_P_SHORT_STEPS_ACC][e]
 *   7 ENERGY       sig[WEDM_SG_ENERGY_ACC][e]
 *   8 GAP_BELOW    (sig[WEDM_SG_SAMPLES_ACC][e] > 0 && gap_floor > sig[WEDM_SG_GAP_MIN_ACC][e])
 *                      ? gap_floor - sig[WEDM_SG_GAP_MIN_ACC][e] : 0.0
 *   9 TMAX_ABOVE   (sig[WEDM_SG_SAMPLES_ACC][e] > 0 && sig[WEDM_SG_TMAX_PEAK_ACC][e] > tmax_ceiling)
 *                      ? sig[WEDM_SG_TMAX_PEAK_ACC][e] - tmax_ceiling : 0.0
 *   The two hinge terms guard on SAMPLES_ACC > 0 because the identities of GAP_MIN_ACC and TMAX_PEAK_ACC are +inf and -inf;
 *   a NaN source fails both comparisons and gives 0.0.  `restart` names the environments that the launch itself restarted
 *   (the in-kernel autoreset): their progress counts from pos_restart, the position a reset leaves.
 * PER ENVIRONMENT e of [0, num_envs), live(e) = mask == NULL || mask[e] != 0:
 *   not live:  reward_out[e] = +0.0f and terms_out[k][e] = +0.0 for every k (a frozen environment earns nothing).
 *   live:      for k ascending  t_k = (weight[k] == 0.0) ? +0.0 : weight[k] * x_k   -- the product rounded to float64, nothing
 *              fused; with a zero weight x_k is NOT READ and its block may be NULL, so 0 * inf cannot occur;
 *              r = +0.0, then r = r + t_k for the k with a nonzero weight, in ascending k, each sum rounded to float64;
 *              reward_out[e] = (float) r, the single rounding to float32;  terms_out[k][e] = t_k where terms_out != NULL.
 *   A NaN is stored as 0x7FF8000000000000 in terms_out and as 0x7FC00000 in reward_out (r is summed from the t_k as they are).
 *   Never written: columns [num_envs, stride) of any block, any input.
 * BLOCKS.  f64 [WEDM_F64_COUNT][stride], i8 [WEDM_I8_COUNT][stride], pulse [WEDM_PULSE_COUNT][stride] and sig
 *   [WEDM_SIG_COUNT][stride] are an environment's state blocks (one stride, in elements); only the rows named above are read,
 *   and only those of terms whose weight is not zero: f64 and pos_before for PROGRESS, i8 for WIRE_BREAK / TARGET, pulse
 *   for SPARKS / SHORTS / SHORT_STEPS, sig for ENERGY / GAP_BELOW / TMAX_ABOVE.  A shard passes its blocks advanced by
 *   its first environment: the call is elementwise.                                                                      */
enum wedm_reward_term {
    WEDM_RW_PROGRESS = 0, WEDM_RW_STEP, WEDM_RW_WIRE_BREAK, WEDM_RW_TARGET, WEDM_RW_SPARKS, WEDM_RW_SHORTS, WEDM_RW_SHORT_STEPS,
    WEDM_RW_ENERGY, WEDM_RW_GAP_BELOW, WEDM_RW_TMAX_ABOVE, WEDM_RW_COUNT
};
typedef struct wedm_reward_desc {
    const double* f64;             /* [WEDM_F64_COUNT][stride] or NULL (weight[PROGRESS] == 0) */
    const int8_t* i8;              /* [WEDM_I8_COUNT][stride] or NULL (weights of WIRE_BREAK and TARGET zero) */
    const int32_t* pulse;          /* [WEDM_PULSE_COUNT][stride] or NULL (weights of SPARKS, SHORTS, SHORT_STEPS zero) */
    const double* sig;             /* [WEDM_SIG_COUNT][stride] or NULL (weights of ENERGY, GAP_BELOW, TMAX_ABOVE zero) */
    const double* pos_before;      /* [num_envs]: the workpiece position before the launch; NULL as f64 */
    const uint8_t* restart;        /* [num_envs] or NULL: nobody was restarted by the launch */
    const uint8_t* mask;           /* [num_envs] or NULL: every environment is live */
    float* reward_out;             /* [num_envs] */
    double* terms_out;             /* [WEDM_RW_COUNT][terms_stride] or NULL */
    int64_t stride;                /* >= num_envs, in elements: the four state blocks' */
    int64_t terms_stride;          /* >= num_envs where terms_out != NULL */
    double weight[WEDM_RW_COUNT];  /* finite; 0.0: the term is off */
    double pos_restart;            /* finite */
    double gap_floor;              /* finite [um] */
    double tmax_ceiling;           /* finite */
    int32_t num_envs;
    int32_t reserved;
} wedm_reward_desc;

/* One launch on `stream`: one lane per environment, no LDS, no atomic.  Stateless like wedm_episode_log: no wedm_ctx, the
 * current device, caller-owned memory.  `desc` is HOST memory, read before the call returns; everything it names is device
 * memory.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; num_envs < 1; stride < num_envs; terms_stride <
 * num_envs with terms_out given; a weight, pos_restart, gap_floor or tmax_ceiling that is not finite; a block that a nonzero
 * weight needs being NULL; reward_out NULL; a pointer not aligned to its element (f64, sig, pos_before, terms_out: 8; pulse,
 * reward_out: 4; i8, restart, mask: any address); an output block (reward_out, terms_out: first to last byte that the call
 * may write) overlapping an input block (the rows that the call may read, pos_before, restart, mask) or the other output.  */
int32_t wedm_reward(const wedm_reward_desc* desc, void* stream);

/* ------------------------------------------------- the sensor model: noise, calibration error and latency, one call
 * One call per control step (and per reset), between the environment's observation and everything downstream: C_out
 * measured CHANNELS, each of one SOURCE column out of the C_in rows of up to two source planes (the environment's observation
 * block and the wire-profile rows, as wedm_normalize takes them), delayed by a whole number of calls, scaled and shifted by
 * a calibration error that is fixed for the episode, disturbed by fresh Gaussian noise, quantised to the ADC's step and
 * saturated at its range.  The output is struct-of-arrays, out[C_out][out_stride]: wedm_normalize reads it as its plane 0.
 *
 * THE CHANNEL TABLE lies in device memory and the host does not read it: float64 chan[WEDM_SENSOR_FIELDS][C_out] (enum
 * wedm_sensor_field: SIGMA, GAIN_SPREAD, OFFSET_SPREAD, LSB, LO, HI) and int32 route[WEDM_SENSOR_ROUTES][C_out] (SOURCE,
 * MAX_DELAY).  Before either forms an address the kernel clamps SOURCE into [0, C_in) and MAX_DELAY into [0, L - 1]; the
 * float64 settings are used as they are (the Python class validates them before it uploads them).
 * STATE, the caller's memory, carried from call to call: ring[L][C_in][ring_stride] float32, the last L samples of every
 * source column (NULL and never touched when L == 1), and int32 pos[num_envs], age[num_envs]: the ring slot of the newest
 * sample and the number of samples the episode has behind it, at most L - 1.
 *
 * PER ENVIRONMENT e of [0, num_envs) with mask == NULL || mask[e] != 0 (for any other e nothing is read and nothing is
 * written: its output, ring, pos and age stay), g = (env_id_offset + e) mod 2^32, k = episode ? (uint64) episode[e] : 0,
 * key = {seed & 0xffffffff, seed >> 32}; all arithmetic float64, every operation rounded on its own, nothing fused:
 *  1. first == NULL || first[e] != 0:  age = 0, pos = 0  (the old values are not used: uninitialised state is harmless);
 *     otherwise  age = min(clamp(age_old, 0, L - 1) + 1, L - 1),  pos = (clamp(pos_old, 0, L - 1) + 1) mod L  (the clamps
 *     change nothing of a state this call wrote; they keep a foreign one from overflowing).
 *  2. L > 1:  ring[pos][s][e] = src[s][e] for every source column s (the bits are copied).
 *  3. for every channel c, s = clamp(SOURCE_c), md = clamp(MAX_DELAY_c):
 *     calibration words, only if GAIN_SPREAD_c != 0 || OFFSET_SPREAD_c != 0 || md != 0:
 *         W  = Philox4x32-10(key, counter {k lo, k hi, g, WEDM_SENSOR_STREAM0 + 0x100000 + c})
 *         ua = ((double) W.x + 0.5) * 2^-32,  ub = ((double) W.y + 0.5) * 2^-32,
 *         d  = (uint32) (((uint64) W.z * (uint64) (md + 1)) >> 32)                  (d = 0 without the words)
 *       -- gain error, offset and delay are a function of (seed, g, k, c): fixed for the episode.
 *     sample:  d_eff = min(d, age) (a delay never reaches into the episode before);
 *         x = d_eff == 0 ? src[s][e] : ring[(pos + L - d_eff) mod L][s][e];   y = (double) x
 *     if GAIN_SPREAD_c != 0 || OFFSET_SPREAD_c != 0:
 *         gain = 1.0 + GAIN_SPREAD_c * (2.0 * ua - 1.0);  off = OFFSET_SPREAD_c * (2.0 * ub - 1.0);  y = (y * gain) + off
 *     if SIGMA_c != 0:   y = y + SIGMA_c * n,  n the step kernels' polar method (Marsaglia on 53-bit pairs, the first of 64
 *         attempts j inside the unit circle, else 0.0) on the counters {t lo, t hi, g, WEDM_SENSOR_STREAM0 + 64 c + j}
 *       -- fresh for every call: a function of (seed, g, t, c).
 *     if LSB_c > 0:      y = LSB_c * rint(y / LSB_c), round half to even
 *     if y < LO_c: y = LO_c.   if y > HI_c: y = HI_c.   (a NaN falls through both comparisons)
 *     out[c][e] = (float) y, one rounding; a NaN is stored as 0x7FC00000 (the sign of a NaN made by an operation differs
 *     between x86 and gfx950).
 *   A channel with the settings 0, 0, 0, 0, -inf, +inf and MAX_DELAY 0 is therefore a copy of the source's bits, -0.0,
 *   subnormals and infinities included (a NaN in its canonical form): that is how clean columns pass through.
 * STREAMS.  WEDM_SENSOR_STREAM0 = 0xA0000000.  The noise of channel c uses WEDM_SENSOR_STREAM0 + 64 c + j, j < 64, c <= 158:
 *   64 * 159 = 10 176 streams, [0xA0000000, 0xA00027C0); the calibration words use WEDM_SENSOR_STREAM0 + 0x100000 + c,
 *   [0xA0100000, 0xA010009F).  The two ranges stay clear of each other and of the physics' streams 0 .. 64, of
 *   wedm_draw_episode's 0x80000000 + q, of the head's from 0xC0000000 and of the minibatch index's 0xE0000000.
 * Never written: columns [num_envs, stride) of any block, the ring slots other than pos, any input.  A shard passes every
 * per-environment pointer advanced by its first environment and env_id_offset moved with it: the call is elementwise.   */
#define WEDM_SENSOR_MAX_DELAY 7          /* L <= WEDM_SENSOR_MAX_DELAY + 1 */
#define WEDM_SENSOR_STREAM0 0xA0000000u
enum wedm_sensor_field {
    WEDM_SN_SIGMA = 0, WEDM_SN_GAIN_SPREAD, WEDM_SN_OFFSET_SPREAD, WEDM_SN_LSB, WEDM_SN_LO, WEDM_SN_HI, WEDM_SENSOR_FIELDS
};
enum wedm_sensor_route { WEDM_SN_SOURCE = 0, WEDM_SN_MAX_DELAY, WEDM_SENSOR_ROUTES };
typedef struct wedm_sensor_desc {
    wedm_norm_plane plane[2];      /* the sources: C_in = plane[0].n_rows + plane[1].n_rows, in [1, WEDM_NORM_MAX_COLUMNS - 1] */
    const double* chan;            /* [WEDM_SENSOR_FIELDS][n_out], device memory */
    const int32_t* route;          /* [WEDM_SENSOR_ROUTES][n_out], device memory */
    const uint8_t* first;          /* [num_envs] or NULL: every environment starts an episode */
    const uint8_t* mask;           /* [num_envs] or NULL: every environment takes part */
    const int64_t* episode;        /* [num_envs] or NULL: episode number 0 */
    float* out;                    /* [n_out][out_stride] */
    float* ring;                   /* [ring_len][C_in][ring_stride]; not read and not written when ring_len == 1 */
    int32_t* pos;                  /* [num_envs] */
    int32_t* age;                  /* [num_envs] */
    int64_t out_stride;            /* >= num_envs, in elements */
    int64_t ring_stride;           /* >= num_envs where ring_len > 1 */
    uint64_t seed;
    uint64_t t;                    /* the caller's call number */
    uint32_t env_id_offset;        /* global id of environment 0 */
    int32_t num_envs;
    int32_t n_out;                 /* C_out, in [1, WEDM_NORM_MAX_COLUMNS - 1] */
    int32_t ring_len;              /* L, in [1, WEDM_SENSOR_MAX_DELAY + 1] */
    int32_t flags;                 /* none is defined: 0 */
    int32_t reserved;
} wedm_sensor_desc;

/* One launch on `stream`: one lane per environment, the channel table through uniform loads, no LDS, no atomic.  Stateless
 * like wedm_reward: no wedm_ctx, the current device, caller-owned memory.  `desc` is HOST memory, read before the call
 * returns; everything it names is device memory.
 * WEDM_ERR_BAD_ARG (text: wedm_last_error(NULL)), nothing launched: desc NULL; flag bits that are not defined; num_envs < 1;
 * a negative n_rows or C_in outside [1, WEDM_NORM_MAX_COLUMNS - 1]; n_out outside the same range; ring_len outside
 * [1, WEDM_SENSOR_MAX_DELAY + 1]; ring NULL with ring_len > 1; a stride (of a plane that has rows, out_stride, ring_stride
 * with ring_len > 1) below num_envs; a needed block NULL or not aligned to its element (chan: 8; the planes' rows, route,
 * out, ring, pos, age: 4; episode: 8; first, mask: any address); out, ring, pos or age (first to last byte that the call may
 * touch) overlapping each other or an input (the planes' rows, chan, route, first, mask, episode).                       */
int32_t wedm_sensor(const wedm_sensor_desc* desc, void* stream);

/* TEST HOOK: evaluates one of the device math primitives the physics relies on,
 * element-wise on device arrays, so tests can compare them bit for bit with the CPU.
 * kind: 0 exp, 1 log, 2 correctly-rounded cube, 3 sqrt, 4 Python floor-division
 * a // b, 5 a / b, 6 the four Philox step uniforms (u0 + 2 u1 + 4 u2 + 8 u3) at (time=a, env=b),
 * 7 Philox polar normal at (time=a, env=b), 8 the spark's cell offset int(a // b) as the kernels
 * compute it (one division + a fused remainder where a >= 0 and b > 0).  Key 0x9abcdef012345678,
 * episode 3.                                                                               */
int32_t wedm_debug_math(int32_t kind, const double* a, const double* b, double* out, int32_t n, void* stream);

/* TEST HOOK: fills the LDS of every compute unit of the current device with `value`.  The step kernels stage only the
 * cells of a wire that exist; rows of their LDS image past a wire's end are never written, and a result that depended
 * on one would go unnoticed as long as the previous kernel happened to leave plausible temperatures there.  The GPU
 * tests poison the LDS (1e30) before every test.                                                                  */
int32_t wedm_debug_poison_lds(float value, void* stream);

/* TEST HOOKS: which instantiation of a step kernel a launch ran.  The library compiles every step kernel in many
 * instantiations -- (kernel number of wedm_set_kernel, lanes per environment, a set of form bits) -- and wedm_step picks one
 * per launch from the handle's settings, the table geometry and the batch size.  wedm_last_kernel()'s string names the
 * family and the bindings only; these three name the instantiation itself, so that a test can hold every one of them to
 * the oracle.  Host code only: none of them launches anything.
 *
 * wedm_debug_registry: entry `index` (0-based) of the list of compiled instantiations -> *kernel (1..12), *lanes (0 for a
 *   family without a lane count), *forms (the form bits).  index == -1: the number of entries -> *kernel (lanes and forms
 *   may be NULL).  Any other index outside the list, or a NULL output: WEDM_ERR_BAD_ARG.  Needs no context and no device.
 * wedm_debug_last_form: the entry the last wedm_step of `ctx` launched.  WEDM_ERR_BAD_ARG before the first launch.
 * wedm_debug_form_name: the name of form bit `bit` (0 = "TRACE", 1 = "F64", ...) as the library's messages spell it;
 *   "" for a bit number past the last form (or below 0).  A static string.                                            */
int32_t wedm_debug_registry(int32_t index, int32_t* kernel, int32_t* lanes, uint32_t* forms);
int32_t wedm_debug_last_form(wedm_ctx* ctx, int32_t* kernel, int32_t* lanes, uint32_t* forms);
const char* wedm_debug_form_name(int32_t bit);

#ifdef __cplusplus
}
#endif
#endif /* WEDM_HIP_H */
