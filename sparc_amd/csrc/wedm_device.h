// wedm_device.h — per-lane physics of one Wire-EDM microsecond on gfx950 (CDNA4).
//
// One lane owns one environment's scalar state in registers (float64, exactly the
// reference's Python-float arithmetic) and walks its wire temperature (float32)
// through an accessor (global memory or LDS).  The five reference modules
// (ignition -> material -> dielectric -> wire -> mechanics, wire_edm.py:123-132)
// are fused: everything before the stencil produces six float32 coefficients, the
// stencil makes ONE pass over the wire, everything after consumes max(T).
//
// Bit-exactness rules (compile with -ffp-contract=off -fno-fast-math):
//   * float64 expressions keep CPython's left-to-right order, no FMA contraction;
//   * `x**2` is x*x, `x**3` a correctly rounded cube (two explicit fma's), exp/log
//     are the table-free IEEE-basic-ops versions of wedm_portable.h — the same expression trees
//     the CPU oracle evaluates in its PORTABLE math mode;
//   * the stencil is float32 op-for-op as the reference evaluates wire.py:58-123
//     under NumPy-2 scalar promotion (every Python float operand cast to float32).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wedm_hip.h"
#include "wedm_env_rows.h"
#include "wedm_portable.h"  // bits2d ... spark_cell_offset, Philox and its variates

namespace wedm {

// ---------------------------------------------------------------- kernel forms
// A form is a compile-time variant of a step kernel family: every wedm_step_* kernel is a template over a set F of these
// bits (<int L, uint32_t F>, or <uint32_t F> where the family has no lane count) and static_asserts the bits its family
// accepts; which (family, lanes, forms) exist is the registry of wedm_kernels.hip.  Code that costs the other launches by
// its mere presence lives in a form of its own.  (Here rather than in wedm_common.h: scalar_prelude and quiet_prelude_t
// below take the forms of their caller.)
enum : uint32_t {
    F_TRACE = 1u << 0,      // the signal-trace point (wedm_bind_trace)
    F_F64 = 1u << 1,        // the float64-typed stencil (stencil_mode 1)
    F_REPLAY = 1u << 2,     // injected variates (wedm_bind_rng_replay)
    F_PULSE = 1u << 3,      // pulse statistics (wedm_bind_pulse_stats)
    F_ENVP = 1u << 4,       // per-environment physics rows (wedm_bind_env_params)
    F_MAT = 1u << 5,        // per-environment wire material (wedm_bind_wire_material)
    F_FROZEN_OK = 1u << 6,  // tile code that tolerates frozen lanes
    F_N1 = 1u << 7,         // stage-major code for one-change tiles (fused kernel)
    F_EXTRA = 1u << 8,      // code for one-change boundary tiles and 1- / 2-cell tails (packed and served kernels)
    F_CUT = 1u << 9,        // wires whose length is not a multiple of 8 (wide register kernel)
    F_ONE = 1u << 10,       // one microsecond per launch, no loop (stream kernel)
    F_CMAX104 = 1u << 11,   // chunks of up to 104 cells in registers, else 64 (stream kernel)
    F_MINB2 = 1u << 12,     // two blocks per CU, else one (float64 wide register kernel)
    F_SIG = 1u << 13,       // signal statistics (wedm_bind_signal_stats)
};

// ------------------------------------------------------------- per-lane state
struct Env {
    double wp, x, v, prev_a;
    double debris, rho, flow, last_gap, last_rho, wire_last_flow;
    double V, I, y, last_crater, cavity;
    double tdelta, tvolt, on, off, tpos, unwind;
    double ipk;  // peak current of the latched mode (ignition.py:98-113); derived, not stored
    double vacc; // running voltage sum since the last control step (row WEDM_F_VOLT_ACC)
    float h_base, h_zone, tmax;
    int32_t time, tss, tsov, tsi, tse, dur, rnd_rem, deb_rem, tcrit, mode, episode, sparks;
    uint32_t key0, key1;
    int32_t state;
    int32_t is_short, broken, reached, done, ctrl, err;
};

// What an ORDINARY microsecond reads.  Passed by value (kernarg -> SGPRs).  Everything
// else stays in the device copy of wedm_params ("cold") and is fetched through an
// opaque pointer inside the rare branch that needs it, so it never occupies SGPRs in
// the substep loop (the full struct is ~1 KB: by value it spilled >150 SGPRs to VGPR
// lanes and cost ~500 v_readlane per step).
struct Hot {
    double hard_short_gap, base_critical_density, gap_coefficient, max_critical_density, sigmoid_steepness;
    double ignition_a, ignition_b, ignition_c, ln2;
    double default_target_voltage, default_on_time, default_off_time, spark_voltage_factor;
    double debris_removal_per_us;
    double dt_s, damping_coeff, stiffness_coeff, omega_n, max_acceleration, max_jerk_dt, max_speed;
    float spool, tref, alpha, tdiel, tcrit, tbreak;
    int32_t servo_interval, dt_us, control_mode, disable_ignition, has_random_short, per_env_geometry;
    uint32_t env_id_offset;
    int32_t n_seg;  // uniform geometry only
    // what a terminating step writes into the lane's `done` (= "frozen") register: 1, or 0 with
    // wedm_params.keep_stepping_terminated (nothing is ever frozen then; store_env derives the DONE row from the flags)
    int32_t done_value;
};

// Pin the float64 every-step constants in VGPRs (same value in every lane).  gfx9 VALU
// instructions read at most ONE scalar operand, so an f64 op on two kernel constants needs a
// v_mov of one of them anyway, and the ~45 SGPRs they occupy are what pushes the substep loop
// into v_readlane / v_writelane SGPR spills.  Only for kernels with VGPRs to spare.
__device__ __forceinline__ void pin_hot_in_vgprs(Hot& h) {
#define WEDM_PIN(x) asm volatile("" : "+v"(h.x))
    WEDM_PIN(hard_short_gap); WEDM_PIN(base_critical_density); WEDM_PIN(gap_coefficient);
    WEDM_PIN(max_critical_density); WEDM_PIN(sigmoid_steepness);
    WEDM_PIN(ignition_a); WEDM_PIN(ignition_b); WEDM_PIN(ignition_c); WEDM_PIN(ln2);
    WEDM_PIN(default_target_voltage); WEDM_PIN(default_on_time); WEDM_PIN(default_off_time);
    WEDM_PIN(spark_voltage_factor); WEDM_PIN(debris_removal_per_us);
    WEDM_PIN(dt_s); WEDM_PIN(damping_coeff); WEDM_PIN(stiffness_coeff); WEDM_PIN(omega_n);
    WEDM_PIN(max_acceleration); WEDM_PIN(max_jerk_dt); WEDM_PIN(max_speed);
#undef WEDM_PIN
}

// per-environment physics rows (wedm_bind_env_params, enum wedm_envp_field): the pointer travels at the END of the kernel
// arguments and is read through the kernel-argument segment (kernarg_envp, wedm_common.h) by the ENVP instantiations only.
// The rows that the kernels read as `Hot` fields are copied into the lane's `Hot` once per launch (envp_apply); the two that
// live in the cold parameters (plasma efficiency, base convection) are read at their point of use, in the style of
// WEDM_COLD_GEOM_F64.
__device__ __forceinline__ const double* kernarg_envp();
#define WEDM_ENVP_ROW(rows, row, stride) ((rows)[(int64_t)(row) * (stride) + e])

// The ENVP instantiations' copy of `Hot`: environment e's rows (wedm_envp_field) replace the uniform values, bit for bit
// (`tdiel` is rounded to float32 as wedm_step rounds the uniform value).  Called once per launch by every lane, before the
// kernel pins its constants in VGPRs; `e` must be a real environment (the rows hold `stride` columns).
__device__ __forceinline__ void envp_apply(Hot& h, int64_t stride, int64_t e) {
    const double* const r = kernarg_envp();
    h.base_critical_density = WEDM_ENVP_ROW(r, WEDM_EP_BASE_CRITICAL_DENSITY, stride);
    h.gap_coefficient = WEDM_ENVP_ROW(r, WEDM_EP_GAP_COEFFICIENT, stride);
    h.max_critical_density = WEDM_ENVP_ROW(r, WEDM_EP_MAX_CRITICAL_DENSITY, stride);
    h.hard_short_gap = WEDM_ENVP_ROW(r, WEDM_EP_HARD_SHORT_GAP, stride);
    h.sigmoid_steepness = WEDM_ENVP_ROW(r, WEDM_EP_SIGMOID_STEEPNESS, stride);
    h.spark_voltage_factor = WEDM_ENVP_ROW(r, WEDM_EP_SPARK_VOLTAGE_FACTOR, stride);
    h.debris_removal_per_us = WEDM_ENVP_ROW(r, WEDM_EP_DEBRIS_REMOVAL_PER_US, stride);
    h.tdiel = (float)WEDM_ENVP_ROW(r, WEDM_EP_DIELECTRIC_TEMPERATURE, stride);
    h.damping_coeff = WEDM_ENVP_ROW(r, WEDM_EP_DAMPING_COEFF, stride);
    h.stiffness_coeff = WEDM_ENVP_ROW(r, WEDM_EP_STIFFNESS_COEFF, stride);
    h.omega_n = WEDM_ENVP_ROW(r, WEDM_EP_OMEGA_N, stride);
    h.max_acceleration = WEDM_ENVP_ROW(r, WEDM_EP_MAX_ACCELERATION, stride);
    h.max_jerk_dt = WEDM_ENVP_ROW(r, WEDM_EP_MAX_JERK_DT, stride);
    h.max_speed = WEDM_ENVP_ROW(r, WEDM_EP_MAX_SPEED, stride);
}

// per-environment wire material (wedm_bind_wire_material, enum wedm_wmat_field): the pointer travels at the END of the
// kernel arguments, after the ENVP pointer, and is read through the kernel-argument segment (kernarg_wmat, wedm_common.h)
// by the MAT instantiations only.  The three rows the kernels read as `Hot` fields are copied into the lane's `Hot` once
// per launch (wmat_apply); the three that live in the cold parameters (rho_elec, rho_c, and alpha_rho of the float64
// stencil) are read at their point of use, in the style of WEDM_COLD_GEOM_F64.  The material's conductivity and heat
// capacity come with the geometry rows (WEDM_G_K_COND, WEDM_G_TUF), which the any-geometry kernels read per environment.
__device__ __forceinline__ const double* kernarg_wmat();
#define WEDM_WMAT_ROW(rows, row, stride) ((rows)[(int64_t)(row) * (stride) + e])

// The MAT instantiations' copy of `Hot`: environment e's material rows replace the uniform values, rounded to float32
// exactly as wedm_step rounds the uniform ones.  Called once per launch by every lane, after envp_apply and before the
// kernel pins its constants in VGPRs; `e` must be a real environment (the rows hold `stride` columns).
__device__ __forceinline__ void wmat_apply(Hot& h, int64_t stride, int64_t e) {
    const double* const r = kernarg_wmat();
    h.alpha = (float)WEDM_WMAT_ROW(r, WEDM_WM_ALPHA_RHO, stride);
    h.tcrit = (float)WEDM_WMAT_ROW(r, WEDM_WM_CRITICAL_TEMPERATURE, stride);
    h.tbreak = (float)WEDM_WMAT_ROW(r, WEDM_WM_BREAKING_TEMPERATURE, stride);
}

__device__ __forceinline__ void pin_mechanics_in_vgprs(Hot& h) {  // the epilogue's constants only
#define WEDM_PIN(x) asm volatile("" : "+v"(h.x))
    WEDM_PIN(dt_s); WEDM_PIN(damping_coeff); WEDM_PIN(stiffness_coeff); WEDM_PIN(omega_n);
    WEDM_PIN(max_acceleration); WEDM_PIN(max_jerk_dt); WEDM_PIN(max_speed);
#undef WEDM_PIN
}

__device__ __forceinline__ void pin_quiet_in_vgprs(Hot& h) {  // the quiet prelude's constants
#define WEDM_PIN(x) asm volatile("" : "+v"(h.x))
    WEDM_PIN(base_critical_density); WEDM_PIN(gap_coefficient); WEDM_PIN(max_critical_density);
    WEDM_PIN(sigmoid_steepness); WEDM_PIN(ignition_a); WEDM_PIN(ignition_b); WEDM_PIN(ignition_c); WEDM_PIN(ln2);
#undef WEDM_PIN
}

// per-lane geometry the every-step path needs (uniform values or the env's rows)
struct Geom {
    double cavity_coeff;
    float k, tuf;
    int32_t n_seg, az_start, az_end, cb, ct;
    double k64, tuf64, a64;  // stencil_mode 1 only: k_cond, temp_update_factor, A as float64
};

// per-lane coefficients that survive across substeps (recomputed only when their
// inputs change): wire.py:304-312 advection, wire.py:349-374 convection
struct Persist {
    float adv, conv_base, conv_zone;
    int32_t adv_on;
    double adv64;  // stencil_mode 1 only
};

// float32 per-step coefficients the scalar prelude hands to the stencil pass
struct Coef {
    float jf;  // joule_factor (wire.py:98)
    float q;   // plasma heat (wire.py:298)
    int32_t joule_on, pidx;
    double jf64, q64;  // stencil_mode 1 only: the same two before their rounding to float32
};

struct Tables {  // device copies of wedm_params' per-mode tables
    const double* mode_current;
    const double* crater_mean;
    const double* crater_std;
    const double* crater_depth;
    const int32_t* crater_valid;
};

struct Cold {  // everything reachable only through rare branches
    const wedm_params* p;
    wedm_geom_ptrs g;
    wedm_action_ptrs a;
    wedm_state_ptrs s;
    Tables tb;
    const double* replay;   // wedm_bind_rng_replay: [step][WEDM_REPLAY_SLOTS][stride], or NULL
    int64_t replay_steps;
    // host-visible word (pinned, mapped): a wave of a kernel instantiation WITHOUT the frozen-lane tile code that finds a
    // terminated environment at its start sets it; wedm_step reads it (plain host read, no synchronisation) and launches
    // the FROZEN_OK instantiation from then on.  Only speed depends on it, never a result.
    int32_t* frozen_seen;
};

// The kernels never touch their by-value `Cold` argument directly: they read it THROUGH the
// kernel-argument segment (constant address space -> s_load at the point of use), with the
// segment pointer laundered at every use so that no load is hoisted out of the rare branch it
// sits in.  By value, the ~40 SGPRs of pointers competed with the every-step constants and the
// substep loop carried 200-370 v_readlane / v_writelane SGPR-spill instructions.
#define WEDM_AS4 __attribute__((address_space(4)))
typedef const WEDM_AS4 Cold* ColdPtr;
struct ColdRef {
    ColdPtr base;
    __device__ __forceinline__ ColdPtr get() const {
        ColdPtr p = base;
        asm volatile("" : "+s"(p));
        return p;
    }
    __device__ __forceinline__ ColdPtr operator->() const { return get(); }
};

// Hide a pointer from loop-invariant code motion: loads through the result cannot be
// hoisted out of the (rare) branch they sit in, so they cost SGPRs only there.
typedef const wedm_params* ParamsPtr;
template <class T>
__device__ __forceinline__ const T* opaque(const T* p) {
    asm volatile("" : "+s"(p));
    return p;
}
// The same, but the result points into the CONSTANT address space (wedm_params is written by the host between
// launches only), so a uniform load through it is an `s_load` (scalar cache, its own counter) instead of the
// `flat_load` the laundered generic pointer gets.  For the few reads at kernel entry / exit: a flat load there is
// queued behind the single-microsecond kernel's stream of wire rows and returns only after all of them.  NOT for the
// rare branches of the microsecond loop: there the scalar results cost SGPRs and v_movs into the float64 VALU
// operands, and measured 4-5 % slower on every fused workload than the vector loads.
template <class T>
__device__ __forceinline__ const WEDM_AS4 T* opaque_const(const T* p) {
    asm volatile("" : "+s"(p));
    return (const WEDM_AS4 T*)(unsigned long long)p;
}

// launch-level switches live in the device copy of wedm_params: read where they are used (kernel entry / exit)
#define WEDM_AUTORESET(cold) (opaque((cold)->p)->autoreset != 0)
#define WEDM_REWARD_ON(cold) (opaque((cold)->p)->reward_mode != 0 && (cold)->s.reward != nullptr)
// (the single-microsecond stream kernel's flavour: scalar loads, see opaque_const)
#define WEDM_AUTORESET_SCALAR(cold) (opaque_const((cold)->p)->autoreset != 0)
#define WEDM_REWARD_ON_SCALAR(cold) (opaque_const((cold)->p)->reward_mode != 0 && (cold)->s.reward != nullptr)

#define WEDM_ROW(ptr, row) ((ptr) + (int64_t)(row) * stride + e)

// cold geometry scalars: the env's row when geometry is per environment, else the uniform value
#define WEDM_COLD_GEOM_F64(cold, hot, row, field) \
    ((hot).per_env_geometry ? (cold)->g.f64[(int64_t)(row) * (cold)->s.stride + e] : opaque((cold)->p)->field)
#define WEDM_COLD_GEOM_I32(cold, hot, row, field) \
    ((hot).per_env_geometry ? (cold)->g.i32[(int64_t)(row) * (cold)->s.stride + e] : opaque((cold)->p)->field)

// ignition.py:98-113 with the module's initial cache (ignition.py:79-81): mode None (0, before the
// first latch) hits the fresh cache and yields 60 A whatever `default_current_mode` is; that
// parameter only serves modes outside currents.json.
// After a reset with reset_semantics 1 (the reference's own: the module object lives on) the cache may hold a mode of the
// previous episode: None then misses it and resolves through `default_current_mode`.  That None is encoded as mode -1
// (written by the reset from flag WEDM_B_MODE_CACHED), so no step ever reads the flag.
__device__ __forceinline__ double peak_current(const ColdRef cold, int32_t mode, int64_t e) {
    (void)e;
    if (mode == 0) return 60.0;
    return (mode >= 1 && mode <= WEDM_MAX_MODE) ? cold->tb.mode_current[mode] : opaque(cold->p)->default_current;
}

// ---- the register state and its rows: load_env ... env_i8_row expand the lists of wedm_env_rows.h, one statement per line and
// in the lists' order.  WEDM_LOAD_ROWS / WEDM_ZERO_ROWS / WEDM_STORE_ROWS(set): the lines with a tag in the set, all three blocks.
#define WEDM_STATE_BLOCKS(CONST)                                       \
    const ColdPtr c = cold.get(); const int64_t stride = c->s.stride; \
    const struct { CONST double* f64; CONST int32_t* i32; CONST int8_t* i8; } s{c->s.f64, c->s.i32, c->s.i8};
#define WEDM_LD_F(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) v.m = (decltype(v.m))*WEDM_ROW(s.f64, row);
#define WEDM_LD_I(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) v.m = (decltype(v.m))*WEDM_ROW(s.i32, row);
#define WEDM_LD_B(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) v.m = (decltype(v.m))*WEDM_ROW(s.i8, row);
#define WEDM_LOAD_ROWS(set) WEDM_ENV_F64(WEDM_LD_F, set) WEDM_ENV_I32(WEDM_LD_I, set) WEDM_ENV_I8(WEDM_LD_B, WEDM_LD_B, set)
#define WEDM_ZERO(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) v.m = 0;
#define WEDM_ZERO_ROWS(set) WEDM_ENV_F64(WEDM_ZERO, set) WEDM_ENV_I32(WEDM_ZERO, set) WEDM_ENV_I8(WEDM_ZERO, WEDM_ZERO, set)
#define WEDM_ST_F(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) *WEDM_ROW(s.f64, row) = (double)v.m;
#define WEDM_ST_I(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) *WEDM_ROW(s.i32, row) = (int32_t)v.m;
#define WEDM_ST_B(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) *WEDM_ROW(s.i8, row) = (int8_t)v.m;
#define WEDM_ST_DONE(set, m, row, stage, role, owner) if constexpr (WEDM_HAS(set, stage, role, owner)) *WEDM_ROW(s.i8, row) = (int8_t)done_row(cold, v);
#define WEDM_STORE_ROWS(set) WEDM_ENV_F64(WEDM_ST_F, set) WEDM_ENV_I32(WEDM_ST_I, set) WEDM_ENV_I8(WEDM_ST_B, WEDM_ST_DONE, set)

__device__ __forceinline__ void load_env(const ColdRef cold, int64_t e, Env& v) {
    WEDM_STATE_BLOCKS(const)
    WEDM_LOAD_ROWS(ROW_ALL)
    v.ipk = 0.0;
}

// The high word of `state.time` (row WEDM_I_TIME_HI; the reference counts in unbounded Python ints, wire_edm.py:135).
// The microsecond loop only carries the low word; a launch advances an environment by less than 2^32 us, so the low
// word wrapped inside this launch exactly when it ended below where it started.  Called by the writer lane BEFORE the
// TIME row is stored: the row still holds the launch's starting value (reinit_env stores the reset value there).
// `span` = n_substeps * dt_us: a low word that ended at or above it cannot have wrapped -- the rows are read only
// behind that (almost never taken) test.
__device__ __forceinline__ void store_time_hi(const ColdRef cold, int64_t e, const Env& v, uint32_t span) {
    if ((uint32_t)v.time < span) {
        const ColdPtr c = cold.get();
        const int64_t stride = c->s.stride;
        int32_t* const i32 = c->s.i32;
        const uint32_t t0 = (uint32_t)*WEDM_ROW(i32, WEDM_I_TIME);
        if ((uint32_t)v.time < t0) *WEDM_ROW(i32, WEDM_I_TIME_HI) += 1;
    }
}

// Row WEDM_B_DONE: the lane's frozen flag, or -- with keep_stepping_terminated, where nothing freezes -- `terminated` of
// the last step as the reference's step() returns it: both of its causes are sticky flags (wire_edm.py:129-130,172-179).
__device__ __forceinline__ int32_t done_row(const ColdRef cold, const Env& v) {
    return opaque(cold->p)->keep_stepping_terminated ? (v.broken | v.reached) : v.done;
}

__device__ __forceinline__ void store_env(const ColdRef cold, int64_t e, const Env& v) {
    WEDM_STATE_BLOCKS()
    WEDM_STORE_ROWS(ROW_STORED)
}

// ---- single-microsecond launches (wedm_step_split2): the state crosses HBM once per microsecond, so
// only the rows a microsecond READS are loaded and only the rows it can have CHANGED are stored.
// Which rows every step assigns before any use (write-only), always or by a launch-level switch: the `role` column of wedm_env_rows.h.
// h64: when given, the two convection coefficients are handed back as loaded (float64) and v.h_base / v.h_zone are left for
// the caller to convert LATER: the conversion is the first use of loaded data, and placed here it made the compiler wait
// for the state rows (a whole memory round trip) before the single-microsecond kernel could request its wire rows.
__device__ __forceinline__ void load_env_inputs(const ColdRef cold, int64_t e, Env& v, bool ignition_on, double* h64 = nullptr,
                                                bool keep_stepping = false) {
    WEDM_STATE_BLOCKS(const)
    WEDM_ENV_F64_DOUBLES(WEDM_LD_F, ROW_IN) WEDM_ENV_F64_SUMS(WEDM_LD_F, ROW_IN)
    static_assert((0u WEDM_ENV_F64_FLOATS(WEDM_ROW_BIT, ROW_IN)) == ((1u << WEDM_F_H_BASE) | (1u << WEDM_F_H_ZONE)),
                  "load_env_inputs() loads the unconditional inputs among the float members by hand (the h64 hand-back)");
    if (h64) { h64[0] = *WEDM_ROW(s.f64, WEDM_F_H_BASE); h64[1] = *WEDM_ROW(s.f64, WEDM_F_H_ZONE); v.h_base = 0.0f; v.h_zone = 0.0f; }
    else { v.h_base = (float)*WEDM_ROW(s.f64, WEDM_F_H_BASE); v.h_zone = (float)*WEDM_ROW(s.f64, WEDM_F_H_ZONE); }
    WEDM_ENV_I32(WEDM_LD_I, ROW_IN) WEDM_ENV_I8(WEDM_LD_B, WEDM_LD_B, ROW_IN)
    // every other member is assigned by the step before any use and starts from zero: current and the short flag ...
    WEDM_ZERO_ROWS(ROW_IN_FORCED)
    if (!ignition_on) { WEDM_LOAD_ROWS(ROW_IN_FORCED) }  // ... unless the caller forces the spark (single_spark_animation.py)
    WEDM_ZERO_ROWS(ROW_OUT | ROW_IN_KEEPSTEP)
    // keep_stepping_terminated: a broken wire's temperature monitor stands still (wire.py:260-261), so the maximum is an input
    if (keep_stepping) { WEDM_LOAD_ROWS(ROW_IN_KEEPSTEP) }  // (wave-uniform switch; the default mode never loads the row)
    v.ipk = 0.0;
}

// ---- the same inputs with HALF the load instructions (stream kernel, an even number of lanes per environment): the
// vector-memory front end of a CU handles one load instruction in ~16-18 cycles whatever it fetches, all 8 waves of the CU
// queue their requests at the same moment, and ~45 of a wave's ~67 loads are state rows that both lanes of an
// environment fetch redundantly.  Here the even lane of a pair loads row A and the odd lane row B IN ONE INSTRUCTION, and
// the two swap through DPP once the data are there (quad_perm [1,0,3,2]: no LDS, no wait counter).
__device__ __forceinline__ int32_t swap_with_neighbour(int32_t x) { return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false); }
__device__ __forceinline__ double swap_with_neighbour(double x) {
    const uint64_t u = d2bits(x);
    const uint32_t lo = (uint32_t)swap_with_neighbour((int32_t)(uint32_t)u), hi = (uint32_t)swap_with_neighbour((int32_t)(uint32_t)(u >> 32));
    return bits2d(((uint64_t)hi << 32) | lo);
}

#define WEDM_PAIR_F64(X) X(0, WEDM_F_WORKPIECE_POS, WEDM_F_WIRE_POS) X(1, WEDM_F_WIRE_VEL, WEDM_F_PREV_ACCEL) \
    X(2, WEDM_F_DEBRIS_VOLUME, WEDM_F_DEBRIS_DENSITY) X(3, WEDM_F_FLOW, WEDM_F_LAST_GAP) X(4, WEDM_F_LAST_DENSITY, WEDM_F_WIRE_LAST_FLOW) \
    X(5, WEDM_F_VOLTAGE, WEDM_F_SPARK_Y) X(6, WEDM_F_TARGET_DELTA, WEDM_F_TARGET_VOLTAGE) X(7, WEDM_F_ON_TIME, WEDM_F_OFF_TIME) \
    X(8, WEDM_F_TARGET_POS, WEDM_F_UNWIND_VEL) X(9, WEDM_F_VOLT_ACC, WEDM_F_H_BASE) X(10, WEDM_F_H_ZONE, WEDM_F_TMAX)
#define WEDM_PAIR_I32(X) X(0, WEDM_I_TIME, WEDM_I_SINCE_SERVO) X(1, WEDM_I_SINCE_OPEN_V, WEDM_I_SINCE_IGNITION) \
    X(2, WEDM_I_SINCE_SPARK_END, WEDM_I_SPARK_DUR) X(3, WEDM_I_RANDOM_SHORT_REM, WEDM_I_DEBRIS_SHORT_REM) \
    X(4, WEDM_I_TIME_CRITICAL, WEDM_I_CURRENT_MODE) X(5, WEDM_I_EPISODE, WEDM_I_KEY_LO) X(6, WEDM_I_KEY_HI, WEDM_I_SPARK_COUNT)
#define WEDM_PAIR_I8(X) X(0, WEDM_B_SPARK_STATE, WEDM_B_WIRE_BROKEN) X(1, WEDM_B_TARGET_REACHED, WEDM_B_DONE) X(2, WEDM_B_ERROR, WEDM_B_ERROR)
// (every pair is one load instruction, so the pairs are chosen by hand; what they must cover follows from the `role` column:
// the inputs, and TMAX, which fills the odd slot and is an input under keep_stepping.  ERROR pairs with itself.)
#define WEDM_PAIR_ONE(k, A, B) +1
#define WEDM_PAIR_BITS(k, A, B) | (1u << (A)) | (1u << (B))
constexpr int PAIRS_F64 = 0 WEDM_PAIR_F64(WEDM_PAIR_ONE), PAIRS_I32 = 0 WEDM_PAIR_I32(WEDM_PAIR_ONE), PAIRS_I8 = 0 WEDM_PAIR_I8(WEDM_PAIR_ONE);
static_assert((0u WEDM_PAIR_F64(WEDM_PAIR_BITS)) == WEDM_F64_ROWS(ROW_IN | ROW_IN_KEEPSTEP) && (0u WEDM_PAIR_I32(WEDM_PAIR_BITS)) == WEDM_I32_ROWS(ROW_IN | ROW_IN_KEEPSTEP) &&
              (0u WEDM_PAIR_I8(WEDM_PAIR_BITS)) == WEDM_I8_ROWS(ROW_IN | ROW_IN_KEEPSTEP) && WEDM_F64_ROWS(ROW_IN_FORCED) == 1u << WEDM_F_CURRENT &&
              WEDM_I32_ROWS(ROW_IN_FORCED) == 0 && WEDM_I8_ROWS(ROW_IN_FORCED) == 1u << WEDM_B_IS_SHORT,
              "the paired loader must load exactly the rows load_env_inputs() loads: the pairs (WEDM_PAIR_*) the roles IN and IN_KEEPSTEP of "
              "wedm_env_rows.h, PairRaw::cur and PairRaw::shrt the role IN_FORCED");
struct PairRaw { double f[PAIRS_F64]; int32_t i[PAIRS_I32]; int32_t b[PAIRS_I8]; double cur; int32_t shrt; };  // a lane's own row of every pair, as loaded

// requests: 21 loads (+ 2 when the caller forces the spark) instead of 40
#define WEDM_PAIR_LD_F(k, A, B) r.f[k] = s.f64[(int64_t)(odd ? (int)(B) : (int)(A)) * stride + e];
#define WEDM_PAIR_LD_I(k, A, B) r.i[k] = s.i32[(int64_t)(odd ? (int)(B) : (int)(A)) * stride + e];
#define WEDM_PAIR_LD_B(k, A, B) r.b[k] = s.i8[(int64_t)(odd ? (int)(B) : (int)(A)) * stride + e];
__device__ __forceinline__ void load_env_inputs_paired_issue(const ColdRef cold, int64_t e, bool odd, bool ignition_on, PairRaw& r) {
    WEDM_STATE_BLOCKS(const)
    WEDM_PAIR_F64(WEDM_PAIR_LD_F) WEDM_PAIR_I32(WEDM_PAIR_LD_I) WEDM_PAIR_I8(WEDM_PAIR_LD_B)
    r.cur = 0.0; r.shrt = 0;
    if (!ignition_on) {  // the caller forces the spark (single_spark_animation.py): current and the short flag are inputs then
        r.cur = *WEDM_ROW(s.f64, WEDM_F_CURRENT);
        r.shrt = *WEDM_ROW(s.i8, WEDM_B_IS_SHORT);
    }
}

// the wait for those loads, where the caller wants it (see env_loaded_here)
__device__ __forceinline__ void pair_raw_loaded_here(PairRaw& r) {
#pragma unroll
    for (int k = 0; k < PAIRS_F64; ++k) asm volatile("" : "+v"(r.f[k]));
#pragma unroll
    for (int k = 0; k < PAIRS_I32; ++k) asm volatile("" : "+v"(r.i[k]));
#pragma unroll
    for (int k = 0; k < PAIRS_I8; ++k) asm volatile("" : "+v"(r.b[k]));
    asm volatile("" : "+v"(r.cur), "+v"(r.shrt));
}

// the swap: every lane ends up with both rows of every pair (what load_env_inputs would have loaded)
__device__ __forceinline__ void load_env_inputs_paired_finish(const PairRaw& r, bool odd, Env& v, bool keep_stepping, double* h64) {
    double fa[PAIRS_F64], fb[PAIRS_F64];
    int32_t ia[PAIRS_I32], ib[PAIRS_I32], ba[PAIRS_I8], bb[PAIRS_I8];
#pragma unroll
    for (int k = 0; k < PAIRS_F64; ++k) { const double o = swap_with_neighbour(r.f[k]); fa[k] = odd ? o : r.f[k]; fb[k] = odd ? r.f[k] : o; }
#pragma unroll
    for (int k = 0; k < PAIRS_I32; ++k) { const int32_t o = swap_with_neighbour(r.i[k]); ia[k] = odd ? o : r.i[k]; ib[k] = odd ? r.i[k] : o; }
#pragma unroll
    for (int k = 0; k < PAIRS_I8; ++k) { const int32_t o = swap_with_neighbour(r.b[k]); ba[k] = odd ? o : r.b[k]; bb[k] = odd ? r.b[k] : o; }
    v.wp = fa[0]; v.x = fb[0]; v.v = fa[1]; v.prev_a = fb[1]; v.debris = fa[2]; v.rho = fb[2]; v.flow = fa[3]; v.last_gap = fb[3];
    v.last_rho = fa[4]; v.wire_last_flow = fb[4]; v.V = fa[5]; v.y = fb[5]; v.tdelta = fa[6]; v.tvolt = fb[6]; v.on = fa[7]; v.off = fb[7];
    v.tpos = fa[8]; v.unwind = fb[8]; v.vacc = fa[9];
    h64[0] = fb[9]; h64[1] = fa[10]; v.h_base = 0.0f; v.h_zone = 0.0f;
    v.tmax = keep_stepping ? (float)fb[10] : 0.0f;   // (an input only where a broken wire is stepped on: load_env_inputs)
    v.time = ia[0]; v.tss = ib[0]; v.tsov = ia[1]; v.tsi = ib[1]; v.tse = ia[2]; v.dur = ib[2]; v.rnd_rem = ia[3]; v.deb_rem = ib[3];
    v.tcrit = ia[4]; v.mode = ib[4]; v.episode = ia[5]; v.key0 = (uint32_t)ib[5]; v.key1 = (uint32_t)ia[6]; v.sparks = ib[6];
    v.state = ba[0]; v.broken = bb[0]; v.reached = ba[1]; v.done = bb[1]; v.err = ba[2];
    v.I = r.cur; v.is_short = r.shrt;
    v.last_crater = 0.0; v.cavity = 0.0; v.ctrl = 0;
    v.ipk = 0.0;
}

// Rows that are final once the scalar prelude has run (stored while the wire is being walked).
// `quiet_only`: every step of the launch took quiet_prelude_t for the whole wave, which never assigns the
// second group (workpiece position, dielectric / convection caches, latched action, short timers,
// spark count, error flag): those rows are left alone.
__device__ __forceinline__ void store_env_after_prelude(const ColdRef cold, int64_t e, const Env& v, bool quiet_only) {
    WEDM_STATE_BLOCKS()
    WEDM_STORE_ROWS(ROW_PRE_QUIET)
    if (quiet_only) return;
    WEDM_STORE_ROWS(ROW_PRE_GENERAL)
}

// Rows the scalar epilogue assigns (mechanics, clocks, temperature monitor, termination, voltage sum).
__device__ __forceinline__ void store_env_after_epilogue(const ColdRef cold, int64_t e, const Env& v) {
    WEDM_STATE_BLOCKS()
    // (block by block as everywhere, but the monitor before the running sums: the order these stores have always had)
    WEDM_ENV_F64_DOUBLES(WEDM_ST_F, ROW_EPILOGUE) WEDM_ENV_F64_FLOATS(WEDM_ST_F, ROW_EPILOGUE) WEDM_ENV_F64_SUMS(WEDM_ST_F, ROW_EPILOGUE)
    WEDM_ENV_I32(WEDM_ST_I, ROW_EPILOGUE) WEDM_ENV_I8(WEDM_ST_B, WEDM_ST_DONE, ROW_EPILOGUE)
}

// Make the compiler treat every loaded state register as USED here: it inserts the wait for the state
// loads at this point (and afterwards knows that none of them is pending).  Needed where vector-memory
// operations the compiler cannot count follow (the LDS-DMA loop of wedm_step_stream): a later first use of a
// state register would otherwise be a conservative `s_waitcnt vmcnt(0)` behind them.
// (Every member by hand, not from the lists: where one statement ends and the next begins decides which loads each wait covers.)
__device__ __forceinline__ void env_loaded_here(Env& v) {
    asm volatile("" : "+v"(v.wp), "+v"(v.x), "+v"(v.v), "+v"(v.prev_a), "+v"(v.debris), "+v"(v.rho), "+v"(v.flow),
                      "+v"(v.last_gap), "+v"(v.last_rho), "+v"(v.wire_last_flow), "+v"(v.V), "+v"(v.I), "+v"(v.y),
                      "+v"(v.last_crater), "+v"(v.cavity));
    asm volatile("" : "+v"(v.tdelta), "+v"(v.tvolt), "+v"(v.on), "+v"(v.off), "+v"(v.tpos), "+v"(v.unwind), "+v"(v.vacc),
                      "+v"(v.h_base), "+v"(v.h_zone), "+v"(v.tmax), "+v"(v.time), "+v"(v.tss), "+v"(v.tsov), "+v"(v.tsi),
                      "+v"(v.tse));
    asm volatile("" : "+v"(v.dur), "+v"(v.rnd_rem), "+v"(v.deb_rem), "+v"(v.tcrit), "+v"(v.mode), "+v"(v.episode),
                      "+v"(v.sparks), "+v"(v.key0), "+v"(v.key1), "+v"(v.state), "+v"(v.is_short), "+v"(v.broken),
                      "+v"(v.reached), "+v"(v.done), "+v"(v.ctrl), "+v"(v.err));
}

// ----------------------------------------------------------------- signal trace
// Row r of each state block as the registers hold it (the value store_env would write; 0 for a row no register holds).
// (`keep_stepping`: wedm_params.keep_stepping_terminated -- row DONE is then `terminated` of the step, see done_row())
#define WEDM_CASE(a, m, row, stage, role, owner) case row: return v.m;
#define WEDM_CASE_DONE(a, m, row, stage, role, owner) case row: return keep_stepping ? (v.broken | v.reached) : v.done;
__device__ __forceinline__ double env_f64_row(const Env& v, int row) { switch (row) { WEDM_ENV_F64(WEDM_CASE, ~) } return 0.0; }
__device__ __forceinline__ int32_t env_i32_row(const Env& v, int row) { switch (row) { WEDM_ENV_I32(WEDM_CASE, ~) } return 0; }
__device__ __forceinline__ int32_t env_i8_row(const Env& v, int row, bool keep_stepping) { switch (row) { WEDM_ENV_I8(WEDM_CASE, WEDM_CASE_DONE, ~) } return 0; }

// Column of environment e in the trace buffers, or -1 when it is not traced.
__device__ __forceinline__ int64_t trace_column(const wedm_trace_desc& tr, int64_t e) {
    const int64_t col = e - tr.env_lo;
    return (col >= 0 && col < tr.env_count) ? col : -1;
}

// The selected scalar rows of one environment into ring slot `slot` (one lane per environment).
__device__ __forceinline__ void trace_scalars(const wedm_trace_desc& tr, int64_t col, const Env& v, int slot, bool keep_stepping) {
    const int64_t cnt = tr.env_count;
    const uint32_t mf = tr.f64_mask, mi = tr.i32_mask, mb = tr.i8_mask;
    // loop over the SET bits (wave-uniform): the cost follows the number of traced rows, not the 45
    // rows that exist (one scalar branch per row tested cost ~13 % with a single traced row)
    if (mf) {
        double* dst = tr.f64 + (int64_t)slot * __builtin_popcount(mf) * cnt + col;
        for (uint32_t m = mf; m; m &= m - 1u) { *dst = env_f64_row(v, __builtin_ctz(m)); dst += cnt; }
    }
    if (mi) {
        int32_t* dst = tr.i32 + (int64_t)slot * __builtin_popcount(mi) * cnt + col;
        for (uint32_t m = mi; m; m &= m - 1u) { *dst = env_i32_row(v, __builtin_ctz(m)); dst += cnt; }
    }
    if (mb) {
        int8_t* dst = tr.i8 + (int64_t)slot * __builtin_popcount(mb) * cnt + col;
        for (uint32_t m = mb; m; m &= m - 1u) { *dst = (int8_t)env_i8_row(v, __builtin_ctz(m), keep_stepping); dst += cnt; }
    }
}

__device__ __forceinline__ void load_geom(const Hot& hot, const ColdRef cold, int64_t e, Geom& g) {
    const ColdPtr c = cold.get();
    const int64_t stride = c->s.stride;
    if (hot.per_env_geometry) {
        const struct { const double* f64; const int32_t* i32; } gp{c->g.f64, c->g.i32};
        g.cavity_coeff = *WEDM_ROW(gp.f64, WEDM_G_CAVITY_COEFF);
        g.k = (float)*WEDM_ROW(gp.f64, WEDM_G_K_COND); g.tuf = (float)*WEDM_ROW(gp.f64, WEDM_G_TUF);
        g.n_seg = *WEDM_ROW(gp.i32, WEDM_GI_N_SEG);
        g.az_start = *WEDM_ROW(gp.i32, WEDM_GI_AZ_START); g.az_end = *WEDM_ROW(gp.i32, WEDM_GI_AZ_END);
        g.cb = *WEDM_ROW(gp.i32, WEDM_GI_CONTACT_BOTTOM); g.ct = *WEDM_ROW(gp.i32, WEDM_GI_CONTACT_TOP);
        g.k64 = *WEDM_ROW(gp.f64, WEDM_G_K_COND); g.tuf64 = *WEDM_ROW(gp.f64, WEDM_G_TUF);
        g.a64 = *WEDM_ROW(gp.f64, WEDM_G_A_SURF);
    } else {
        const wedm_params* p = c->p;
        g.cavity_coeff = p->cavity_coeff;
        g.k = (float)p->k_cond; g.tuf = (float)p->tuf;
        g.n_seg = p->n_seg; g.az_start = p->az_start; g.az_end = p->az_end;
        g.cb = p->contact_bottom; g.ct = p->contact_top;
        g.k64 = p->k_cond; g.tuf64 = p->tuf; g.a64 = p->a_surf;
    }
}

// The cold parameter block as scalar_prelude reads it: through the laundered GENERIC pointer (vector `flat_load`s: what
// the fused kernels measured fastest, see opaque_const) or, SCOLD, through the constant address space (scalar loads).
// The single-microsecond stream kernel needs the second: vector loads return in order, and its general prelude runs
// while the lane's whole wire is still in flight -- a flat load issued there comes back only after every wire word.
template <bool SCOLD> struct ColdParams;
template <> struct ColdParams<false> {
    typedef const wedm_params* type;
    static __device__ __forceinline__ type get(const wedm_params* p) { return opaque(p); }
};
template <> struct ColdParams<true> {
    typedef const WEDM_AS4 wedm_params* type;
    static __device__ __forceinline__ type get(const wedm_params* p) { return opaque_const(p); }
};

// Entry `lane` of the per-mode crater tables in lane `lane` (the stream kernel requests them with its very first loads,
// like the peak-current table): a lookup is then a cross-lane read instead of a vector load queued behind the wire.
struct LaneTables { double mean, sd, depth; int32_t valid; };

// wire.py:349-374: h_eff * A products the stencil uses (float32 x float32, wire.py:109)
template <bool SCOLD = false>
__device__ __forceinline__ void refresh_convection(const Hot& hot, const ColdRef cold, int64_t e, const Env& s,
                                                   Persist& ps) {
    const float A = (float)(hot.per_env_geometry ? cold->g.f64[(int64_t)WEDM_G_A_SURF * cold->s.stride + e]
                                                 : ColdParams<SCOLD>::get(cold->p)->a_surf);
    ps.conv_base = s.h_base * A;
    ps.conv_zone = s.h_zone * A;
}

// once per launch: coefficients whose inputs no module changes (wire.py:304-312)
// SCALAR_LOADS (the single-microsecond stream kernel): the uniform constants through the constant address space
// MAT: rho_c comes from the environment's wire-material row (wedm_bind_wire_material)
template <bool SCALAR_LOADS = false, bool MAT = false>
__device__ __forceinline__ void init_persist(const Hot& hot, const ColdRef cold, int64_t e, const Env& s, Persist& ps) {
    double adv = 0.0;
    if (__builtin_fabs(s.unwind) > 1e-6) {
        if (SCALAR_LOADS) {
            const auto pc = opaque_const(cold->p);
            const double s_area = hot.per_env_geometry ? cold->g.f64[(int64_t)WEDM_G_S_AREA * cold->s.stride + e] : pc->s_area;
            const double rho_c = MAT ? WEDM_WMAT_ROW(kernarg_wmat(), WEDM_WM_RHO_C, cold->s.stride) : pc->rho_c;
            adv = rho_c * __builtin_fabs(s.unwind) * s_area;
        } else {
            const double s_area = WEDM_COLD_GEOM_F64(cold, hot, WEDM_G_S_AREA, s_area);
            const double rho_c = MAT ? WEDM_WMAT_ROW(kernarg_wmat(), WEDM_WM_RHO_C, cold->s.stride) : cold->p->rho_c;
            adv = rho_c * __builtin_fabs(s.unwind) * s_area;
        }
    }
    ps.adv_on = __builtin_fabs(adv) > 1e-9;  // wire.py:115
    ps.adv = ps.adv_on ? (float)adv : 0.0f;
    ps.adv64 = ps.adv_on ? adv : 0.0;
    if (SCALAR_LOADS) {  // refresh_convection()
        const float A = (float)(hot.per_env_geometry ? cold->g.f64[(int64_t)WEDM_G_A_SURF * cold->s.stride + e]
                                                     : opaque_const(cold->p)->a_surf);
        ps.conv_base = s.h_base * A;
        ps.conv_zone = s.h_zone * A;
    } else {
        refresh_convection(hot, cold, e, s, ps);
    }
}

// --------------------------------------------------- scalar prelude (modules 1-4a)
// wire_edm.py:117-121 latch, ignition.py:175-319, material.py:79-174,
// dielectric.py:82-163, wire.py:271-312.  Returns the per-step stencil coefficients.
// Running get_crater_statistics (material.py:207-227), kept in HBM.  No-return atomics: the
// wave does not wait for memory (a load-modify-store here stalled the wave for two HBM round
// trips at almost every third microsecond, since some lane of a wave nearly always sparks:
// -5 % on the 400-segment workload).  One lane per environment updates, in spark order, so the
// sums are the same sequence of IEEE additions as the oracle's.
__device__ __forceinline__ void crater_stats_update(double* st, int64_t sd, double vol) {
    (void)__hip_atomic_fetch_add(st + WEDM_S_CRATER_SUM * sd, vol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(st + WEDM_S_CRATER_SUMSQ * sd, vol * vol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_min(st + WEDM_S_CRATER_MIN * sd, vol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(st + WEDM_S_CRATER_MAX * sd, vol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `writer`: the one lane of an environment's L lanes that updates per-environment global memory
// beyond the state blocks (the running statistics).
struct QuietTry {  // what a failed quiet_prelude_t hands on: the step's Philox words, if it drew them (wave-uniform flag)
    W4 w;
    bool have_w;
};

// F: the calling kernel's forms (the bits below are read, the others ignored).
// F_REPLAY: the variates come from the caller's table (wedm_bind_rng_replay) instead of Philox — the reference's own
// draws, so that a native-seed run of the reference can be followed on the device (validation mode, global kernel).
// F_ENVP: plasma efficiency and base convection come from the environment's rows (wedm_bind_env_params) where they are
// used; the caller has put the rows of the `Hot` fields into `p` (envp_apply).
// F_MAT: the electrical resistivity of the Joule factor comes from the environment's wire-material row
// (wedm_bind_wire_material); the caller has put the material's `Hot` fields into `p` (wmat_apply).
// SCOLD / lt: the single-microsecond stream kernel's flavour -- cold parameters by scalar loads, crater tables from the
// lanes' registers (ColdParams, LaneTables): no vector load on the path a fresh spark takes.
template <uint32_t F = 0, bool SCOLD = false>
__device__ __forceinline__ Coef scalar_prelude(const Hot& p, const ColdRef cold, const Geom& g, int64_t e,
                                               uint32_t gid, Env& s, Persist& ps, bool writer,
                                               const QuietTry& qt = QuietTry{W4{0u, 0u, 0u, 0u}, false},
                                               const LaneTables* lt = nullptr, const LaneTables* lt1 = nullptr) {
    constexpr bool REPLAY = (F & F_REPLAY) != 0, ENVP = (F & F_ENVP) != 0, MAT = (F & F_MAT) != 0;
    double rv[WEDM_REPLAY_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // The cold parameter block and the pointer block, fetched ONCE per call (laundered: nothing read through them can
    // be hoisted out of the microsecond loop).  Every rare branch below used to launder its own copy: two dependent
    // scalar loads (kernel-argument segment, then the field) and a wait at each of ~15 sites of a fresh-spark step.
    const ColdPtr cc0 = cold.get();
    const typename ColdParams<SCOLD>::type c0 = ColdParams<SCOLD>::get(cc0->p);
    // the uniform constants of the rare branches, requested in one batch (scalar loads: one wait at the first use)
    const double seg = c0->segment_len, eff = c0->plasma_efficiency, rho_elec = c0->rho_elec, jg_u = c0->joule_geom;
    const double h_u = c0->workpiece_height, kerf_u = c0->kerf_base;
    const double ref_gap = c0->reference_gap, obstruction = c0->debris_obstruction_coeff;
    const int zs_u = c0->zone_start;
    if (REPLAY) {
        const ColdPtr c = cc0;
        int64_t step = (int64_t)s.time / p.dt_us;
        if (step >= c->replay_steps) { s.err = 1; step = c->replay_steps - 1; }
        const double* rp = c->replay + step * (int64_t)WEDM_REPLAY_SLOTS * c->s.stride + e;
#pragma unroll
        for (int q = 0; q < WEDM_REPLAY_SLOTS; ++q) rv[q] = rp[(int64_t)q * c->s.stride];
    }
    // ---- control-step latch (wire_edm.py:117-121,162-170)
    s.ctrl = s.tss >= p.servo_interval;
    if (s.ctrl) {
        const ColdPtr c = cc0;
        s.tdelta = c->a.servo[e];
        s.tvolt = c->a.target_voltage[e];
        s.mode = c->a.current_mode[e];
        s.on = c->a.on_time[e];
        s.off = c->a.off_time[e];
        s.tss = 0;
        s.ipk = peak_current(cold, s.mode, e);
    }
    const uint32_t t = (uint32_t)s.time, ep = (uint32_t)s.episode;

#ifdef WEDM_ABL_NO_IGN
    if (false) {
#else
    if (!p.disable_ignition) {
#endif
        // ---- short-circuit detection (ignition.py:197-245), written branch-free: in a
        // wave the lanes are in different generator states, so every per-lane `if` would be
        // executed by the whole wave anyway; selects avoid the exec-mask bookkeeping.  Real
        // branches remain only around rare, heavy work (exp, Philox, cold parameters).
        const bool timer_r = s.rnd_rem > 0;                 // random-short timer runs (checked first)
        const bool timer_d = !timer_r && (s.deb_rem > 0);   // debris-short timer runs
        const bool timers = timer_r || timer_d;
        const double d0 = s.wp - s.x;                       // unclamped gap (ignition.py:353)
        const double gap = d0 > 0.0 ? d0 : 0.0;
        const bool hard = gap < p.hard_short_gap;           // ignition.py:127-128
        double crit = p.base_critical_density + p.gap_coefficient * gap;
        crit = crit < p.max_critical_density ? crit : p.max_critical_density;
        const double ex = -p.sigmoid_steepness * (s.rho - crit);
        // every uniform is >= 2^-33 and 1/(1+e^ex) < 2^-33 for ex > 24: the roll cannot succeed,
        // so the exponential need not be evaluated there (same decision, exactly)
        double p_d = (hard || ex < -500) ? 1.0 : 0.0;
        // (a native NumPy uniform can be arbitrarily small: with injected variates the whole branch of ignition.py:136-146)
        if (!timers && !hard && ex <= (REPLAY ? 500.0 : 24.0) && ex >= -500) p_d = 1.0 / (1.0 + portable_exp(ex));
        double p_r = 0.0;
        if (p.has_random_short) {  // ignition.py:221-230; max_probability == 0 by default
            const auto c = c0;
            if (gap >= c->random_short_max_gap) p_r = 0.0;
            else if (gap <= c->random_short_min_gap) p_r = c->random_short_max_probability;
            else
                p_r = (1.0 - (gap - c->random_short_min_gap) / (c->random_short_max_gap - c->random_short_min_gap)) *
                      c->random_short_max_probability;
        }
        const bool idle = s.state == 0;
        W4 w{0u, 0u, 0u, 0u};
#ifndef WEDM_ABL_NO_PHILOX
        // (the words are a pure function of key, time, episode and environment: when the quiet attempt of this
        // step has already drawn them for the whole wave they are taken over instead of being computed again)
        if (qt.have_w) w = qt.w;
        else if (!timers && (p_d > 0.0 || p_r > 0.0 || idle)) w = philox4(s.key0, s.key1, t, ep, gid, 0u);
#else
        w = W4{t * 2654435761u + gid, 1u, 0xffffffffu - (t ^ gid) * 40503u, 7u};
#endif
        // p_d and p_r are exactly 0 in the ordinary gap regime: the rolls cannot succeed and the
        // integer -> double conversions are skipped for the whole wave
        bool new_d = false, new_r = false;
        if (__any(!timers && (p_d > 0.0 || p_r > 0.0))) {
            new_d = !timers && ((REPLAY ? rv[WEDM_RS_DEBRIS_ROLL] : u32_to_unit(w.x)) < p_d);
            new_r = !timers && !new_d && ((REPLAY ? rv[WEDM_RS_RANDOM_ROLL] : u32_to_unit(w.y)) < p_r);
        }
        if (new_d || new_r) {  // rare: a short begins (durations are cold parameters)
            const auto c = c0;
            if (new_d) s.deb_rem = c->debris_short_duration;
            else s.rnd_rem = c->random_short_duration;
        }
        s.rnd_rem = timer_r ? s.rnd_rem - 1 : s.rnd_rem;
        s.deb_rem = timer_d ? s.deb_rem - 1 : s.deb_rem;
        const bool shrt = timers || new_d || new_r;
        s.is_short = shrt ? 1 : 0;

        // `x or default` getters (ignition.py:329-343)
        const double Vt = s.tvolt != 0.0 ? s.tvolt : p.default_target_voltage;
        const double on = s.on != 0.0 ? s.on : p.default_on_time;
        const double off = s.off != 0.0 ? s.off : p.default_off_time;
        const double Vs = Vt * p.spark_voltage_factor;
        const double Ipk = s.ipk;

        // ---- spark state machine (ignition.py:186-195, 247-319) as selects
        const bool spk = s.state == 1, pls = s.state == -1, rst = s.state == -2;
        const double lam = p.ln2 / (p.ignition_a * (d0 * d0) + p.ignition_b * d0 + p.ignition_c);
        const bool ign = idle && !shrt && ((REPLAY ? rv[WEDM_RS_IGNITION_ROLL] : u32_to_unit(w.z)) < lam);   // _should_ignite
        const bool to_pulse = idle && shrt;                           // short during idle -> pulse
        const int32_t dur1 = s.dur + 1;
        const double ddur = (double)dur1;
        const bool end_on = (spk || pls) && (ddur >= on);             // spark / pulse finished
        const bool end_rest = rst && (ddur >= on + off);              // rest finished
        const bool burning = (ign || to_pulse) || ((spk || pls) && !end_on);
        double V = shrt ? 0.0 : s.V;                                  // ignition.py:182-183
        V = (idle && !shrt) ? (ign ? Vs : Vt) : V;
        V = (spk && !shrt) ? (end_on ? 0.0 : Vs) : V;
        V = (rst && !shrt) ? (end_rest ? Vt : 0.0) : V;
        s.V = V;
        s.I = burning ? Ipk : 0.0;
        // `_get_peak_current` is called exactly where `burning` holds; with a latched mode it fills the module's current
        // cache (ignition.py:98-113).  The first such call after a mode was latched falls on an ignition, a short pulse
        // or the latch step itself, and every one of those runs this general prelude: flag WEDM_B_MODE_CACHED.
        if (writer && burning && s.mode > 0 && (ign || to_pulse || s.ctrl))
            cc0->s.i8[(int64_t)WEDM_B_MODE_CACHED * cc0->s.stride + e] = 1;
        if (ign) {  // rare: spark location, Generator.uniform(0, h)
            const double h = p.per_env_geometry ? cc0->g.f64[(int64_t)WEDM_G_HEIGHT * cc0->s.stride + e] : h_u;
            s.y = REPLAY ? rv[WEDM_RS_SPARK_Y] : 0.0 + (h - 0.0) * u32_to_unit(w.w);
        }
        s.y = (to_pulse || end_rest) ? __builtin_nan("") : s.y;
        s.dur = idle ? ((ign || to_pulse) ? 0 : s.dur) : (end_rest ? 0 : dur1);
        s.state = ign ? 1 : to_pulse ? -1 : end_on ? -2 : end_rest ? 0 : s.state;
    }  // !disable_ignition
    const bool fresh = (s.state == 1) && (s.dur == 0);  // material.py:83, dielectric.py:95

    // `lt` / `lt1` (stream kernel): the crater-table entries of this lane's mode AS IT WAS BEFORE THIS STEP and of mode I1,
    // looked up by the caller across lanes; a step that latches a new mode reads the tables in memory
    const bool use_lt = lt != nullptr && !__any(s.ctrl != 0);

    // ---- material removal (material.py:79-174)
    if (fresh) {
        const ColdPtr cc = cc0;
        const Tables tb{cc->tb.mode_current, cc->tb.crater_mean, cc->tb.crater_std, cc->tb.crater_depth, cc->tb.crater_valid};
        int m = s.mode <= 0 ? 1 : s.mode;  // None (0, or -1: see peak_current) -> "I1" (material.py:104-105)
        const bool in_range = m >= 1 && m <= WEDM_MAX_MODE;
        if (!in_range) m = 1;
        // everything this branch reads from memory is requested here, before the crater normal (~230 instructions
        // with no memory access) is computed: one latency instead of a chain of them
        const int32_t valid = use_lt ? lt->valid : tb.crater_valid[m];
        double mean = use_lt ? lt->mean : tb.crater_mean[m], sd = use_lt ? lt->sd : tb.crater_std[m],
               depth = use_lt ? lt->depth : tb.crater_depth[m];
        const double kerf_base = p.per_env_geometry ? cc0->g.f64[(int64_t)WEDM_G_KERF_BASE * cc0->s.stride + e] : kerf_u;
        const double h = p.per_env_geometry ? cc0->g.f64[(int64_t)WEDM_G_HEIGHT * cc0->s.stride + e] : h_u;
        double* const clog = cc->s.crater_log;
        const int64_t clog_cap = cc->s.crater_log_capacity, sstride = cc->s.stride;
        double* const stats = cc->s.stats;
        if (!in_range || !valid) {  // unknown mode (the reference raises ValueError, material.py:108-113)
            s.err = 1;
            if (use_lt) { mean = lt1->mean; sd = lt1->sd; depth = lt1->depth; }
            else { mean = tb.crater_mean[1]; sd = tb.crater_std[1]; depth = tb.crater_depth[1]; }
        }
        double vol;
        if (REPLAY) {
            vol = rv[WEDM_RS_CRATER_UM3];
        } else {
            const double z = philox_std_normal(s.key0, s.key1, t, ep, gid);
            vol = mean + sd * z;
        }
        if (!(vol > 0)) vol = 0;
        if (writer && clog && clog_cap > 0)  // crater_volumes_um3.append (material.py:133)
            clog[((int64_t)s.sparks % clog_cap) * sstride + e] = vol;
        s.sparks += 1;
        if (writer && stats) crater_stats_update(stats + e, sstride, vol);
        double crater = vol / 1e9;
        s.last_crater = crater;
        if (crater > 0) {
            double kerf = kerf_base + depth / 1000.0;
            double dx = 0.0;
            if (kerf > 0 && h > 0) dx = crater / (kerf * h) * 1000.0;
            s.wp += dx;
        }
    } else {
        s.last_crater = 0.0;
    }

    // ---- dielectric / debris (dielectric.py:82-163)
#ifndef WEDM_ABL_NO_DIEL
    {
        double d = s.wp - s.x;
        double gap_um = d > 0.001 ? d : 0.001;
        s.cavity = g.cavity_coeff * (gap_um * 0.001);
        if (fresh && s.last_crater > 0) s.debris += s.last_crater;
        if (s.cavity > 0) {
            double q = s.debris / s.cavity;
            s.rho = q < 1.0 ? q : 1.0;
        } else {
            s.rho = 0.0;
        }
        if (__builtin_fabs(gap_um - s.last_gap) > 0.01 || __builtin_fabs(s.rho - s.last_rho) > 0.001) {
            double cube = cube_cr(gap_um / ref_gap);
            double gap_factor = cube < 1.0 ? cube : 1.0;
            double kd = obstruction * s.rho;
            double df;
            if (kd < 2.0) df = kd < 0.5 ? (1 - 0.5 * kd) / (1 + 0.5 * kd) : portable_exp(-kd);
            else df = portable_exp(-obstruction * s.rho);
            s.flow = gap_factor * df;
            s.last_gap = gap_um;
            s.last_rho = s.rho;
        }
        if (s.flow > 0.001 && s.debris > 0.001) {
            double nv = s.debris - p.debris_removal_per_us * s.flow;
            s.debris = nv > 0.0 ? nv : 0.0;
        }
    }
#endif

    // ---- wire prelude (wire.py:271-312, 349-374)
    Coef cf;
    {
        const double I = s.I, I2 = I * I;
        // (`!s.broken`: with keep_stepping_terminated a broken wire's module returns before it looks at its convection cache,
        // wire.py:260-261; elsewhere a broken wire never gets here)
        if (!s.broken && __builtin_fabs(s.flow - s.wire_last_flow) > 0.01) {
            const auto c = c0;
            double ve = c->convection_velocity_factor * s.unwind;
            ve = ve > -0.9 ? ve : -0.9;
            const double base_convection = ENVP ? WEDM_ENVP_ROW(kernarg_envp(), WEDM_EP_BASE_CONVECTION, cc0->s.stride)
                                                : c->base_convection;
            double hb = base_convection * (1.0 + ve);
            double fl = 0.1 * base_convection;
            hb = fl > hb ? fl : hb;
            double he = hb * (1.0 + c->convection_flow_enhancement * s.flow);
            s.h_base = (float)hb;
            s.h_zone = (float)he;
            s.wire_last_flow = s.flow;
            refresh_convection<SCOLD>(p, cold, e, s, ps);
        }
        cf.pidx = -1;
        cf.q = 0.0f;
        cf.q64 = 0.0;
        if (s.state == 1 && s.y == s.y) {
            const int zone_start = p.per_env_geometry ? cc0->g.i32[(int64_t)WEDM_GI_ZONE_START * cc0->s.stride + e] : zs_u;
            int idx = seg != 0 ? zone_start + spark_cell_offset(s.y, seg) : zone_start;
            if (idx >= 0 && idx < g.n_seg) {
                cf.pidx = idx;
                cf.q64 = (ENVP ? WEDM_ENVP_ROW(kernarg_envp(), WEDM_EP_PLASMA_EFFICIENCY, cc0->s.stride) : eff) * s.V * I;
                cf.q = (float)cf.q64;
            }
        }
        cf.joule_on = I2 > 1e-6;
        cf.jf = 0.0f;
        cf.jf64 = 0.0;
        if (cf.joule_on) {
            const double joule_geom = p.per_env_geometry ? cc0->g.f64[(int64_t)WEDM_G_JOULE_GEOM * cc0->s.stride + e] : jg_u;
            cf.jf64 = joule_geom * I2 * (MAT ? WEDM_WMAT_ROW(kernarg_wmat(), WEDM_WM_RHO_ELEC, cc0->s.stride) : rho_elec);
            cf.jf = (float)cf.jf64;
        }
    }
    return cf;
}

// ------------------------------------------------- scalar work split over the two lanes of one environment
// Where two neighbouring lanes (2 i, 2 i + 1) hold the SAME environment (wedm_step_regs<2>), code that runs one
// instruction sequence on two independent operand sets need not run both sets in both lanes: the even lane ("A") takes
// one set, the odd lane ("B") the other, and they hand each other the result through the quad permute [1,0,3,2] of
// swap_with_neighbour.  Every operation is the same integer / IEEE operation on the same operands; only the lane that
// executes it changes, so the results are bit for bit what both lanes would have computed.
// The exchanges must run with a lane's partner active.  The two lanes of an environment hold identical scalar state
// and therefore take the same branches, so a lane's partner is active whenever the lane is; the callers below also keep
// the exchanges in wave-uniform control flow.  Used only by the two-lane register kernel.
__device__ __forceinline__ bool pair_lane_b() { return (threadIdx.x & 1u) != 0u; }
// the even lane's value in both lanes / the odd lane's value in both lanes: quad permutes [0,0,2,2] and [1,1,3,3]
// (a quad permute reads no lane outside the quad, so the result needs no `old` value: mov_dpp leaves it undefined and
// saves the move that update_dpp(0, ..) spends on it)
__device__ __forceinline__ uint32_t pair_from_a(uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int32_t)x, 0xA0, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t pair_from_b(uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int32_t)x, 0xF5, 0xF, 0xF, true); }
__device__ __forceinline__ double pair_from_a(double x) {
    const uint64_t u = d2bits(x);
    return bits2d(((uint64_t)pair_from_a((uint32_t)(u >> 32)) << 32) | pair_from_a((uint32_t)u));
}
__device__ __forceinline__ double pair_from_b(double x) {
    const uint64_t u = d2bits(x);
    return bits2d(((uint64_t)pair_from_b((uint32_t)(u >> 32)) << 32) | pair_from_b((uint32_t)u));
}

// Philox4x32-10 of philox4(), one multiplication chain per lane.  A round of philox4 is
//     p0 = M0 c0, p1 = M1 c2;  c0' = hi(p1) ^ c1 ^ k0, c1' = lo(p1), c2' = hi(p0) ^ c3 ^ k1, c3' = lo(p0):
// lane A holds (X, lo) = (c0, c3), multiplies by M0 and owns key k0; lane B holds (c2, c1), multiplies by M1 and owns k1.
// Both run   m = mul X;  t = hi(m) ^ lo;  lo = lo(m);  X = partner(t) ^ k;  k += weyl
// -- one 64-bit multiply and two xors (the partner's t as the DPP operand of the second) instead of two and four.
// After the tenth round A holds (c0, c3) and B holds (c2, c1).
// One running key per lane, advanced by an add per round (ten round keys of a launch kept in registers, what the compiler
// does for philox4 in a microsecond loop, measured 10 % slower here: DESIGN.md section 4.4).
struct PhiloxHalf { uint32_t X, lo; };
__device__ __forceinline__ PhiloxHalf philox4_pair(bool lane_b, uint32_t key0, uint32_t key1, uint32_t time, uint32_t episode,
                                                   uint32_t gid, uint32_t stream) {
    // (the lane's choice among launch constants -- key, episode, environment -- made opaque per call: hoisted out of a
    // microsecond loop the selected values are registers the loop does not have, and come back as scratch loads)
    uint32_t odd = lane_b ? 1u : 0u;
    asm volatile("" : "+v"(odd));
    lane_b = odd != 0u;
    const uint32_t mul = lane_b ? 0xCD9E8D57u : 0xD2511F53u, weyl = lane_b ? 0xBB67AE85u : 0x9E3779B9u;
    uint32_t X = lane_b ? gid : time, lo = lane_b ? episode : stream, k = lane_b ? key1 : key0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t m = (uint64_t)mul * X;
        const uint32_t t = (uint32_t)(m >> 32) ^ lo;
        lo = (uint32_t)m;
        X = (uint32_t)swap_with_neighbour((int32_t)t) ^ k;
        k += weyl;
    }
    return PhiloxHalf{X, lo};
}
// the four words of philox4() in both lanes (off the hot line: the general prelude's rolls)
__device__ __forceinline__ W4 philox4_pair_words(PhiloxHalf h) {
    return W4{pair_from_a(h.X), pair_from_b(h.lo), pair_from_b(h.X), pair_from_a(h.lo)};
}

// ------------------------------------------------- quiet-step fast path (wave-uniform)
// In an ordinary microsecond nothing discrete happens to an environment: no short timer runs,
// the generator idles or rests, the action is not latched, the gap is far from a hard short, the
// debris sigmoid cannot fire (exponent > 24), the flow / convection caches stay valid and the
// ignition roll fails.  For such a step scalar_prelude() reduces to the straight line below
// (every assignment is what the general code computes under exactly these conditions).  The
// fast path is taken only if EVERY live lane of the wave qualifies and none ignites; nothing is
// written before that is known, so otherwise the general path runs on untouched state.
// Returns true when the step was handled (the stencil coefficients are then {0, 0, off, none}).
// DENSE (the instantiation for densely sparking batches, chosen per launch from the spark density of the previous ones):
// the same straight line also carries a spark that ignited in an EARLIER microsecond and keeps burning or ends now
// (ignition.py:270-287 with no short: duration + 1, voltage = spark voltage or 0, current = peak or 0, state 1 -> -2
// when the ON time is over) and hands its plasma / Joule coefficients to the stencil (wire.py:284-301) — for such a
// lane scalar_prelude() computes exactly these assignments.  Only an igniting lane (fresh spark: crater, debris, cache
// refresh), a short, or a control-step latch still sends the wave through the general path.  Bit-identical; it costs
// registers, so batches that spark rarely run the instantiation without it.
// F: the calling kernel's forms.  F_ENVP: the plasma efficiency comes from the environment's row (wedm_bind_env_params),
// as in scalar_prelude.  F_MAT: the electrical resistivity comes from the environment's wire-material row
// (wedm_bind_wire_material), as in scalar_prelude.
// PAIR: the caller's lanes 2 i and 2 i + 1 hold the same environment (wedm_step_regs<2>).  The step's Philox words are
// then computed half in each lane (philox4_pair), and the line's two float64 quotients -- debris / cavity and
// ln 2 / (a d0^2 + b d0 + c), independent of each other -- by ONE division sequence: the even lane divides the first
// pair of operands, the odd lane the second, and each takes the other's quotient by DPP.  For that the ignition
// denominator is formed before the first ballot (it has no side effect; when no lane idles its quotient is unused).
template <bool DENSE, uint32_t F = 0, bool PAIR = false>
__device__ __forceinline__ bool quiet_prelude_t(const Hot& p, const ColdRef cold, const Geom& g, int64_t e, uint32_t gid,
                                                Env& s, QuietTry& qt, Coef& cf) {
    constexpr bool ENVP = (F & F_ENVP) != 0, MAT = (F & F_MAT) != 0;
    qt.have_w = false;
    if (p.disable_ignition || p.has_random_short) return false;
    const bool live = !s.done;
    const double d0 = s.wp - s.x;                       // unclamped gap (>= hard_short_gap > 0.001 below)
    const bool idle = s.state == 0, rest = s.state == -2;
    const bool spk = DENSE && s.state == 1;             // ignited in an earlier microsecond
    double crit = p.base_critical_density + p.gap_coefficient * d0;
    crit = crit < p.max_critical_density ? crit : p.max_critical_density;
    const double ex = -p.sigmoid_steepness * (s.rho - crit);
    bool q = (s.tss < p.servo_interval) && (s.rnd_rem == 0) && (s.deb_rem == 0) && (idle || rest || spk) &&
             (d0 >= p.hard_short_gap) && (ex > 24.0);
    // dielectric (dielectric.py:87-139): this step's density and the cache test
    const double cavity = g.cavity_coeff * (d0 * 0.001);
    double rho = 0.0;
    double lam_pair = 0.0;
    if (PAIR) {
        const bool lane_b = pair_lane_b();
        const double den = p.ignition_a * (d0 * d0) + p.ignition_b * d0 + p.ignition_c;
        const double quot = (lane_b ? p.ln2 : s.debris) / (lane_b ? den : cavity);
        const double qq = pair_from_a(quot);
        lam_pair = pair_from_b(quot);
        if (cavity > 0) rho = qq < 1.0 ? qq : 1.0;
    } else if (cavity > 0) {
        const double qq = s.debris / cavity;
        rho = qq < 1.0 ? qq : 1.0;
    }
    q = q && !(__builtin_fabs(d0 - s.last_gap) > 0.01 || __builtin_fabs(rho - s.last_rho) > 0.001) &&
        !(__builtin_fabs(s.flow - s.wire_last_flow) > 0.01) && (d0 > 0.001);
    if (!__all(q || !live)) return false;
    // ignition roll of the idle lanes (ignition.py:321-327)
    bool ign = false;
    PhiloxHalf wh{0u, 0u};
    if (__any(idle && live)) {
        if (PAIR) {
            wh = philox4_pair(pair_lane_b(), s.key0, s.key1, (uint32_t)s.time, (uint32_t)s.episode, gid, 0u);
            ign = idle && live && (u32_to_unit(pair_from_b(wh.X)) < lam_pair);   // w.z is the odd lane's X
        } else {
            const double lam = p.ln2 / (p.ignition_a * (d0 * d0) + p.ignition_b * d0 + p.ignition_c);
            const W4 w = philox4(s.key0, s.key1, (uint32_t)s.time, (uint32_t)s.episode, gid, 0u);
            ign = idle && live && (u32_to_unit(w.z) < lam);
            qt.w = w;      // every lane of the wave computed its words: the general path need not repeat them
        }
        qt.have_w = true;
    }
    if (__any(ign)) {
        // (the general path wants all four words: exchanged here, off the quiet line, still with every lane active)
        if (PAIR) qt.w = philox4_pair_words(wh);
        return false;
    }
    bool burning = false;
    if (live) {
        const double Vt = s.tvolt != 0.0 ? s.tvolt : p.default_target_voltage;
        const double on = s.on != 0.0 ? s.on : p.default_on_time;
        const double off = s.off != 0.0 ? s.off : p.default_off_time;
        const int32_t dur1 = s.dur + 1;
        const bool end_rest = rest && ((double)dur1 >= on + off);
        const bool end_on = spk && ((double)dur1 >= on);
        burning = spk && !end_on;
        s.ctrl = 0;
        s.is_short = 0;
        double V = idle ? Vt : (end_rest ? Vt : 0.0);
        if (DENSE) V = spk ? (end_on ? 0.0 : Vt * p.spark_voltage_factor) : V;
        s.V = V;
        s.I = burning ? s.ipk : 0.0;
        s.y = end_rest ? __builtin_nan("") : s.y;
        s.dur = idle ? s.dur : (end_rest ? 0 : dur1);
        s.state = end_rest ? 0 : (end_on ? -2 : s.state);
        s.last_crater = 0.0;
        s.cavity = cavity;
        s.rho = rho;
        if (s.flow > 0.001 && s.debris > 0.001) {
            const double nv = s.debris - p.debris_removal_per_us * s.flow;
            s.debris = nv > 0.0 ? nv : 0.0;
        }
    }
    if (DENSE && __any(burning)) {  // wire.py:284-301, 96-100 for the lanes that keep burning
        // the five cold constants of this block in one batch of scalar loads (one wait instead of four chains of two)
        const ColdPtr cc0 = cold.get();
        const ParamsPtr c = opaque(cc0->p);
        const double seg = c->segment_len, eff = c->plasma_efficiency, rho_elec = c->rho_elec;
        const int zone_start = (p.per_env_geometry && burning) ? cc0->g.i32[(int64_t)WEDM_GI_ZONE_START * cc0->s.stride + e] : c->zone_start;
        const double joule_geom = (p.per_env_geometry && burning) ? cc0->g.f64[(int64_t)WEDM_G_JOULE_GEOM * cc0->s.stride + e] : c->joule_geom;
        if (burning && s.y == s.y) {
            const int idx = seg != 0 ? zone_start + spark_cell_offset(s.y, seg) : zone_start;
            if (idx >= 0 && idx < g.n_seg) {
                cf.pidx = idx;
                cf.q64 = (ENVP ? WEDM_ENVP_ROW(kernarg_envp(), WEDM_EP_PLASMA_EFFICIENCY, cc0->s.stride) : eff) * s.V * s.I;
                cf.q = (float)cf.q64;
            }
        }
        if (burning) {
            const double I2 = s.I * s.I;
            cf.joule_on = I2 > 1e-6;
            if (cf.joule_on) {
                cf.jf64 = joule_geom * I2 * (MAT ? WEDM_WMAT_ROW(kernarg_wmat(), WEDM_WM_RHO_ELEC, cc0->s.stride) : rho_elec);
                cf.jf = (float)cf.jf64;
            }
        }
    }
    return true;
}

// a - 2*b exactly as the reference rounds it: 2*b is exact in binary floating point, so
// `a - (2*b)` rounds once, which is what one fused multiply-add fma(-2, b, a) computes.  The only
// FMA in the stencil: everywhere else a product is rounded before it is added (wire.py:91-120).
__device__ __forceinline__ float sub_twice(float a, float b) { return __builtin_fmaf(-2.0f, b, a); }
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v sub_twice(f2v a, f2v b) {
    const f2v m2 = {-2.0f, -2.0f};
    return __builtin_elementwise_fma(m2, b, a);
}

// one cell of wire.py:58-123, float32 op for op; tm1/tc/tp1 are OLD temperatures
__device__ __forceinline__ float stencil_cell(int i, int n_seg, float tm1, float tc, float tp1, const Geom& g,
                                              const Coef& c, const Persist& ps, float tref, float alpha,
                                              float tdiel) {
    float d;
    if (i < n_seg - 1) {
        float a = sub_twice(tm1, tc);  // T[i-1] - 2*T[i]
        d = g.k * (a + tp1);
    } else {
        d = g.k * (tm1 - tc);
    }
    if (c.joule_on && i >= g.cb && i <= g.ct) {
        float rho_T = 1.0f + alpha * (tc - tref);
        d = d + c.jf * rho_T;
    }
    if (i == c.pidx) d = d + c.q;
    bool in_zone = (i >= g.az_start) && (i < g.az_end);
    float conv = in_zone ? ps.conv_zone : ps.conv_base;
    d = d - conv * (tc - tdiel);
    if (ps.adv_on) d = d + ps.adv * (tm1 - tc);
    return tc + d * g.tuf;
}

// The same cell as Numba types wire.py:58-123 (`@njit`: float32 array elements promoted to float64 in
// every expression, the result rounded where it is stored into the float32 `dT_dt[i]` / `T[i]`; without
// fastmath re-association) — wedm_params.stencil_mode 1.  h_base / h_zone are the float32 `h_eff_zone`
// entries (wire.py:205), everything else float64 constants.
struct StencilF64 {  // the float64 constants of that typing (read from the cold parameters by the F64 instantiations)
    double tref, alpha, tdiel;
};
__device__ __forceinline__ float stencil_cell_f64(int i, int n_seg, float tm1, float tc, float tp1, const Geom& g,
                                                  const Coef& c, const Persist& ps, const StencilF64& h, float h_base,
                                                  float h_zone) {
    const double m = (double)tm1, t = (double)tc;
    float d;
    if (i < n_seg - 1) d = (float)(g.k64 * (m - 2.0 * t + (double)tp1));
    else d = (float)(g.k64 * (m - t));
    if (c.joule_on && i >= g.cb && i <= g.ct) {
        const double rho_T = 1.0 + h.alpha * (t - h.tref);
        d = (float)((double)d + c.jf64 * rho_T);
    }
    if (i == c.pidx) d = (float)((double)d + c.q64);
    const bool in_zone = (i >= g.az_start) && (i < g.az_end);
    const double conv = (double)(in_zone ? h_zone : h_base) * g.a64;
    d = (float)((double)d - conv * (t - h.tdiel));
    if (ps.adv_on) d = (float)((double)d + ps.adv64 * (m - t));
    return (float)(t + (double)d * g.tuf64);
}

// An INTERIOR cell (1 <= i <= n - 2) in that typing, coefficients handed in (the fused kernel's tile code, stencil_mode 1):
// the same sequence of float64 expressions and float32 roundings as stencil_cell_f64, with the Joule and advection terms
// always applied -- their coefficient is 0.0 where the reference skips them, and (float)((double)d + 0.0 * x) == d.
__device__ __forceinline__ float interior_cell_f64(float tm1, float tc, float tp1, double k64, double tuf64, double conv64,
                                                   double tdiel64, double adv64, double jfe64, double alpha64, double tref64) {
    const double m = (double)tm1, t = (double)tc;
    float d = (float)(k64 * (m - 2.0 * t + (double)tp1));
    const double rho_T = 1.0 + alpha64 * (t - tref64);
    d = (float)((double)d + jfe64 * rho_T);
    d = (float)((double)d - conv64 * (t - tdiel64));
    d = (float)((double)d + adv64 * (m - t));
    return (float)(t + (double)d * tuf64);
}

// ------------------------------------------- scalar epilogue (modules 4b, 5, env)
// wire.py:376-388, wire_edm.py:129-146,172-179, mechanics.py:79-114
// Two halves.  The MONITOR is everything that reads the step's maximum temperature (wire.py:376-388: time above the critical
// temperature, the break test); the MOTION is what follows a step whose wire did not break (the driver's voltage sum,
// mechanics, clocks, termination) and reads nothing the monitor writes except `broken`.  scalar_epilogue() is the two in the
// reference's order; a kernel whose scalar physics runs ahead of its stencil (wedm_step_served) calls the motion half first
// where it can PROVE that the step cannot break the wire, and the monitor half when the maximum arrives.
__device__ __forceinline__ void epilogue_voltage_sum(Env& s) {
    // the driver appends state.voltage after EVERY step(), the early-return one included
    // (experiments/run_simulation.py:256-264): running sum in step order
#ifndef WEDM_ABL_NO_VACC
    s.vacc = s.vacc + s.V;
#endif
}

// wire.py:376-388 (`_check_wire_breaking`); returns with s.broken set when the wire broke in this step
__device__ __forceinline__ void epilogue_monitor(const Hot& p, Env& s, float tmax) {
    int32_t tcrit = tmax > p.tcrit ? s.tcrit + 1 : 0;
    // keep_stepping_terminated only (elsewhere a broken wire is frozen and never gets here): the wire module returns at
    // once on a broken wire (wire.py:260-261) -- no stencil (the caller's walk left this lane's wire alone and its `tmax`
    // is meaningless), no temperature monitor
    if (__any(s.broken != 0)) {
        tmax = s.broken ? s.tmax : tmax;
        tcrit = s.broken ? s.tcrit : tcrit;
    }
    s.tmax = tmax;
    s.tcrit = tcrit;
    if (tmax > p.tbreak) s.broken = 1;
}

// mechanics.py:79-114, wire_edm.py:135-146,172-179 for a step whose wire is not broken
__device__ __forceinline__ void epilogue_motion(const Hot& p, Env& s) {
#ifndef WEDM_ABL_NO_MECH
    {
        double x = s.x, v = s.v, a_nom;
        if (p.control_mode == 0) {
            double x_error = x - (x + s.tdelta);
            a_nom = p.damping_coeff * v + p.stiffness_coeff * x_error;
        } else {
            a_nom = -p.omega_n * (v - s.tdelta);
        }
        if (a_nom > p.max_acceleration) a_nom = p.max_acceleration;
        else if (a_nom < -p.max_acceleration) a_nom = -p.max_acceleration;
        double da = a_nom - s.prev_a;
        if (da > p.max_jerk_dt) da = p.max_jerk_dt;
        else if (da < -p.max_jerk_dt) da = -p.max_jerk_dt;
        double a = s.prev_a + da;
        s.prev_a = a;
        v += a * p.dt_s;
        if (v > p.max_speed) v = p.max_speed;
        else if (v < -p.max_speed) v = -p.max_speed;
        x += v * p.dt_s;
        s.v = v;
        s.x = x;
    }
#endif
    s.time = (int32_t)((uint32_t)s.time + (uint32_t)p.dt_us);  // low word of the 64-bit clock: wraps (store_time_hi)
    s.tss += p.dt_us;
    s.tsov = (int32_t)((uint32_t)s.tsov + (uint32_t)p.dt_us);  // never reset by the reference either: in step with `time`
    if (s.state == 1) { s.tsi += p.dt_us; s.tse = 0; }
    else { s.tse += p.dt_us; s.tsi = 0; }
    if (s.x > s.wp + 100) { s.broken = 1; s.done = p.done_value; }
    else if (s.wp >= s.tpos) { s.reached = 1; s.done = p.done_value; }
}

__device__ __forceinline__ void scalar_epilogue(const Hot& p, Env& s, float tmax) {
    epilogue_voltage_sum(s);
    epilogue_monitor(p, s, tmax);
    if (s.broken) {  // early return before mechanics and clocks
        s.done = p.done_value;
        return;
    }
    epilogue_motion(p, s);
}

// The wire of a lane whose wire is broken stays as it is: around its walk a kernel ORs `broken` into the lane's frozen
// flag (`freeze_wire`) and afterwards takes it out again (`unfreeze_wire`).  Without keep_stepping_terminated both are
// no-ops (a broken wire is frozen anyway: done_value 1); with it they make the walk skip exactly the lanes whose wire
// module would return at once (wire.py:260-261) while prelude and epilogue go on running.
// Lanes past the end of the batch carry done = WEDM_DEAD_LANE (bit 1), which neither of the two ever clears: such a lane
// never runs physics and never stores, in either mode.
#define WEDM_DEAD_LANE 2
__device__ __forceinline__ void freeze_wire(Env& s) { s.done |= s.broken; }
__device__ __forceinline__ void unfreeze_wire(const Hot& p, Env& s) { s.done &= (p.done_value ? ~0 : WEDM_DEAD_LANE); }

__device__ __forceinline__ void write_obs(const ColdRef cold, int64_t e, const Env& s) {
    const ColdPtr c = cold.get();
    float* obs = c->s.obs;
    if (!obs || c->p->obs_dim < 8) return;
    const int64_t stride = c->s.stride;
    float* o = obs + e;
    o[0 * stride] = (float)(s.wp - s.x);
    o[1 * stride] = (float)s.v;
    o[2 * stride] = (float)s.V;
    o[3 * stride] = (float)s.I;
    o[4 * stride] = (float)s.state;
    o[5 * stride] = (float)s.rho;
    o[6 * stride] = (float)s.flow;
    o[7 * stride] = s.tmax;
}

// Control step (wire_edm.py:117-121): the observation, the interval's voltage sum (row
// WEDM_F_VOLT_SUM: this step included, plus the previous control step's sample the accumulator was
// restarted from) and the restart of the accumulator.  Every lane of an environment restarts its
// replica; only `writer` touches memory.
__device__ __forceinline__ void control_step_outputs(const ColdRef cold, int64_t e, Env& s, bool writer) {
    if (writer) {
        write_obs(cold, e, s);
        const ColdPtr c = cold.get();
        c->s.f64[(int64_t)WEDM_F_VOLT_SUM * c->s.stride + e] = s.vacc;
    }
    s.vacc = s.V;
}

// ------------------------------------------------- pulse statistics (wedm_bind_pulse_stats, enum wedm_pulse_field)
// The block's pointer travels at the END of the kernel arguments (existing kernels keep their argument layout) and is read
// through the kernel-argument segment at the point of use, like `Cold`: it costs SGPRs only inside the rare branch.
typedef int32_t* const WEDM_AS4* PulseSlot;
struct PulseRef {
    PulseSlot slot;
    __device__ __forceinline__ int32_t* get() const {
        PulseSlot p = slot;
        asm volatile("" : "+s"(p));
        return *p;
    }
};

// what the reference driver's summary looks at in one sample (experiments/run_simulation.py:604-627): 0 = no pulse
// (I <= 0.1 A), 1 = a spark pulse (I > 0.1 A, no short), 2 = a short pulse (I > 0.1 A during a short)
__device__ __forceinline__ int32_t pulse_kind(const Env& s) { return s.I > 0.1 ? (s.is_short ? 2 : 1) : 0; }

// The tally of one sample, called by every kernel's PULSE instantiation right before control_step_outputs() for a step the
// environment ran; `prev` = pulse_kind() of the previous sample (taken before the step's prelude).  A rising edge and a
// short-circuit sample are rare per environment: the writer lane increments the accumulator row in memory with a
// fire-and-forget atomic (no register carries a count through the microsecond loop, nothing waits), as crater_stats_update()
// does at a fresh spark.  At a control step the accumulators are swapped out for zero (atomics to the same address from
// one lane are performed in program order) and published, with the observation's columns 8-10 where obs_dim >= 11.
template <bool PULSE>
__device__ __forceinline__ void pulse_tally(const PulseRef pulse, const ColdRef cold, int64_t e, const Env& s, int32_t prev,
                                            bool writer) {
    if (!PULSE) return;
    const int32_t kind = pulse_kind(s);
    const bool edge = kind != 0 && kind != prev;
    if (writer && (edge || s.is_short || s.ctrl)) {
        int32_t* const rows = pulse.get();
        const ColdPtr c = cold.get();
        const int64_t stride = c->s.stride;
        if (edge)
            (void)__hip_atomic_fetch_add(WEDM_ROW(rows, kind == 1 ? WEDM_P_SPARK_ACC : WEDM_P_SHORT_ACC), 1, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        if (s.is_short)
            (void)__hip_atomic_fetch_add(WEDM_ROW(rows, WEDM_P_SHORT_STEPS_ACC), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s.ctrl) {
            float* const obs = c->s.obs;
            const bool to_obs = obs && opaque(c->p)->obs_dim >= 11;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int32_t n = __hip_atomic_exchange(WEDM_ROW(rows, WEDM_P_SPARK_ACC + q), 0, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
                *WEDM_ROW(rows, WEDM_P_SPARK_LAST + q) = n;
                if (to_obs) obs[(int64_t)(8 + q) * stride + e] = (float)n;
            }
        }
    }
}

// reinit_env()'s part for the pulse block (the in-launch autoreset): all six rows to zero, by the writer lane
template <bool PULSE>
__device__ __forceinline__ void pulse_reinit(const PulseRef pulse, const ColdRef cold, int64_t e, bool writer) {
    if (!PULSE || !writer) return;
    int32_t* const rows = pulse.get();
    const int64_t stride = cold->s.stride;
#pragma unroll
    for (int q = 0; q < WEDM_PULSE_COUNT; ++q) __hip_atomic_store(WEDM_ROW(rows, q), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------- signal statistics (wedm_bind_signal_stats, enum wedm_sig_field)
// The block's pointer travels at the END of the kernel arguments, after the wire-material pointer, and is read through the
// kernel-argument segment at the point of use (kernarg_sig, wedm_common.h), like the pulse block's.
typedef double* const WEDM_AS4* SigSlot;
struct SigRef {
    SigSlot slot;
    __device__ __forceinline__ double* get() const {
        SigSlot p = slot;
        asm volatile("" : "+s"(p));
        return *p;
    }
};

// The six accumulators of one environment (rows WEDM_SG_*_ACC).  Unlike a pulse edge, every sample updates every one of
// them, so they do not live in memory during a launch: the SIG instantiations load them when they open the environment
// (sig_load), carry them in registers through the microsecond loop and store them when the launch closes (sig_store).
// Every lane of an environment carries a replica; only the writer lane touches memory.  Without F_SIG the struct is never
// read or written and costs nothing.
struct Sig { double n, cur, en, gap, gmin, tpk; };

__device__ __forceinline__ void sig_identities(Sig& g) {
    g.n = 0.0; g.cur = 0.0; g.en = 0.0; g.gap = 0.0; g.gmin = __builtin_inf(); g.tpk = -__builtin_inf();
}

// the accumulator rows of environment e (`live`: not a lane past the batch, whose replica is never stored)
template <bool SIG>
__device__ __forceinline__ void sig_load(const SigRef sig, const ColdRef cold, int64_t e, bool live, Sig& g) {
    if (!SIG) return;
    sig_identities(g);
    if (!live) return;
    const double* const rows = sig.get();
    const int64_t stride = cold->s.stride;
    g.n = *WEDM_ROW(rows, WEDM_SG_SAMPLES_ACC); g.cur = *WEDM_ROW(rows, WEDM_SG_CURRENT_ACC);
    g.en = *WEDM_ROW(rows, WEDM_SG_ENERGY_ACC); g.gap = *WEDM_ROW(rows, WEDM_SG_GAP_ACC);
    g.gmin = *WEDM_ROW(rows, WEDM_SG_GAP_MIN_ACC); g.tpk = *WEDM_ROW(rows, WEDM_SG_TMAX_PEAK_ACC);
}

// the launch's close: the accumulators back into their rows, in the lane for which `store` holds
template <bool SIG>
__device__ __forceinline__ void sig_store(const SigRef sig, const ColdRef cold, int64_t e, bool store, const Sig& g) {
    if (!SIG || !store) return;
    double* const rows = sig.get();
    const int64_t stride = cold->s.stride;
    *WEDM_ROW(rows, WEDM_SG_SAMPLES_ACC) = g.n; *WEDM_ROW(rows, WEDM_SG_CURRENT_ACC) = g.cur;
    *WEDM_ROW(rows, WEDM_SG_ENERGY_ACC) = g.en; *WEDM_ROW(rows, WEDM_SG_GAP_ACC) = g.gap;
    *WEDM_ROW(rows, WEDM_SG_GAP_MIN_ACC) = g.gmin; *WEDM_ROW(rows, WEDM_SG_TMAX_PEAK_ACC) = g.tpk;
}

// The tally of one sample, called where pulse_tally is: right before control_step_outputs() for a step the environment ran.
// The energy term is the product V * I rounded to float64 and then added: the build's -ffp-contract=off (part of the
// numerics contract) keeps the compiler from fusing the two into one fma, which would round once.  At a control step the
// writer lane publishes the accumulators (this sample included) into the *_LAST rows and, as float32, into the observation
// columns base .. base + 4 (base 11 in a PULSE form, whose block owns columns 8-10, else 8) where obs_dim holds them; every
// lane restarts its replica from the identities.  Plain vector stores: nothing else writes these rows during a launch.
template <bool SIG, bool PULSE>
__device__ __forceinline__ void sig_tally(const SigRef sig, const ColdRef cold, int64_t e, const Env& s, bool writer, Sig& g) {
    if (!SIG) return;
    const double gap = s.wp - s.x, tm = (double)s.tmax;
    const double vi = s.V * s.I;
    g.n += 1.0;
    g.cur += s.I;
    g.en += vi;
    g.gap += gap;
    g.gmin = gap < g.gmin ? gap : g.gmin;
    g.tpk = tm > g.tpk ? tm : g.tpk;
    if (s.ctrl) {
        if (writer) {
            double* const rows = sig.get();
            const ColdPtr c = cold.get();
            const int64_t stride = c->s.stride;
            *WEDM_ROW(rows, WEDM_SG_SAMPLES_LAST) = g.n; *WEDM_ROW(rows, WEDM_SG_CURRENT_LAST) = g.cur;
            *WEDM_ROW(rows, WEDM_SG_ENERGY_LAST) = g.en; *WEDM_ROW(rows, WEDM_SG_GAP_LAST) = g.gap;
            *WEDM_ROW(rows, WEDM_SG_GAP_MIN_LAST) = g.gmin; *WEDM_ROW(rows, WEDM_SG_TMAX_PEAK_LAST) = g.tpk;
            constexpr int base = PULSE ? 11 : 8;
            float* const obs = c->s.obs;
            if (obs && opaque(c->p)->obs_dim >= base + 5) {
                float* const o = obs + e;
                o[(int64_t)(base + 0) * stride] = (float)g.cur;
                o[(int64_t)(base + 1) * stride] = (float)g.en;
                o[(int64_t)(base + 2) * stride] = (float)g.gap;
                o[(int64_t)(base + 3) * stride] = (float)g.gmin;
                o[(int64_t)(base + 4) * stride] = (float)g.tpk;
            }
        }
        sig_identities(g);
    }
}

// reinit_env()'s part for the signal block (the in-launch autoreset): the replica to the identities (the close stores it
// into the *_ACC rows), the *_LAST rows to zero by the writer lane
template <bool SIG>
__device__ __forceinline__ void sig_reinit(const SigRef sig, const ColdRef cold, int64_t e, bool writer, Sig& g) {
    if (!SIG) return;
    sig_identities(g);
    if (!writer) return;
    double* const rows = sig.get();
    const int64_t stride = cold->s.stride;
#pragma unroll
    for (int q = WEDM_SG_SAMPLES_LAST; q < WEDM_SIG_COUNT; ++q) *WEDM_ROW(rows, q) = 0.0;
}

// wedm_params.autoreset: what wedm_reset_kernel(mask = DONE, reseed = 0) writes for one environment,
// applied to the registers at the start of a launch (next-step autoreset).  `writer` also clears the
// per-environment memory outside the register state (statistics, observation) and stores the rows
// store_env() never writes.  The caller sets the environment's wire to the spool temperature.
__device__ __forceinline__ void reinit_env(const ColdRef cold, int64_t e, Env& s, bool writer) {
    const ColdPtr c = cold.get();
    const ParamsPtr p = opaque(c->p);
    const int32_t episode = s.episode + 1;
    const uint32_t k0 = s.key0, k1 = s.key1;
    const float spool = (float)p->spool_T;
    // reset_semantics 1: the reference's reset() builds a new EDMState only (wire_edm.py:106-114); what its module objects
    // hold lives on: short timers, debris volume, flow / density / convection caches, `prev_accel`, the crater list
    const bool keep_modules = p->reset_semantics != 0;
    s.wp = p->initial_gap; s.x = 0.0; s.v = 0.0;
    s.rho = 0.0; s.V = 0.0; s.I = 0.0; s.y = __builtin_nan(""); s.last_crater = 0.0; s.cavity = 0.0;
    s.tdelta = 0.0; s.tvolt = 0.0; s.on = 0.0; s.off = 0.0; s.tpos = p->target_cutting_distance; s.unwind = 0.2;
    s.vacc = 0.0;
    s.tmax = spool;
    s.time = 0; s.tss = 0; s.tsov = 0; s.tsi = 0; s.tse = 0; s.dur = 0; s.tcrit = 0;
    // state.current_mode = None: 0, or -1 where the module's surviving current cache names a mode (peak_current)
    s.mode = (keep_modules && c->s.i8[(int64_t)WEDM_B_MODE_CACHED * c->s.stride + e]) ? -1 : 0;
    s.episode = episode; s.key0 = k0; s.key1 = k1;
    s.state = 0; s.is_short = 0; s.broken = 0; s.reached = 0; s.done = 0; s.ctrl = 0; s.err = 0;
    if (!keep_modules) {  // the members whose line in wedm_env_rows.h says MODULE (wedm_reset_kernel takes its masks from that column)
        s.prev_a = 0.0; s.debris = 0.0; s.flow = 0.0; s.last_gap = -1.0; s.last_rho = -1.0; s.wire_last_flow = 0.0;
        s.h_base = 0.0f; s.h_zone = 0.0f; s.rnd_rem = 0; s.deb_rem = 0; s.sparks = 0;
    }
    if (writer) {
        const int64_t stride = c->s.stride;
        *WEDM_ROW(c->s.f64, WEDM_F_WORKPIECE_POS) = s.wp;   // the reward's "position at the start of the launch"
        *WEDM_ROW(c->s.f64, WEDM_F_TARGET_POS) = s.tpos;
        *WEDM_ROW(c->s.f64, WEDM_F_UNWIND_VEL) = s.unwind;
        *WEDM_ROW(c->s.f64, WEDM_F_VOLT_SUM) = 0.0;
        *WEDM_ROW(c->s.i32, WEDM_I_EPISODE) = episode;
        *WEDM_ROW(c->s.i32, WEDM_I_TIME) = 0;      // store_time_hi's "low word at the start of the launch"
        *WEDM_ROW(c->s.i32, WEDM_I_TIME_HI) = 0;
        if (!keep_modules) {
            *WEDM_ROW(c->s.i8, WEDM_B_MODE_CACHED) = 0;
            if (c->s.stats) {
                *WEDM_ROW(c->s.stats, WEDM_S_CRATER_SUM) = 0.0; *WEDM_ROW(c->s.stats, WEDM_S_CRATER_SUMSQ) = 0.0;
                *WEDM_ROW(c->s.stats, WEDM_S_CRATER_MIN) = __builtin_inf(); *WEDM_ROW(c->s.stats, WEDM_S_CRATER_MAX) = -__builtin_inf();
            }
        }
        if (c->s.obs)
            for (int q = 0; q < p->obs_dim; ++q) c->s.obs[(int64_t)q * stride + e] = 0.0f;
    }
}

// wedm_params.reward_mode 1, called by the writer lane right BEFORE store_env(): the workpiece-position
// row still holds the value the launch started from (reinit_env stored the reset value there).
__device__ __forceinline__ void write_reward(const ColdRef cold, int64_t e, const Env& s) {
    const ColdPtr c = cold.get();
    if (!c->s.reward) return;
    const double wp0 = c->s.f64[(int64_t)WEDM_F_WORKPIECE_POS * c->s.stride + e];
    const double pen = opaque(c->p)->reward_break_penalty;
    c->s.reward[e] = (float)(s.wp - wp0) - (float)pen * (s.broken ? 1.0f : 0.0f);
}

}  // namespace wedm
