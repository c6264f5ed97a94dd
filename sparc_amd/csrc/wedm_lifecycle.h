// wedm_lifecycle.h — what a step kernel does with an environment around its walk: the launch's `Hot`, opening the
// environment (load, next-step autoreset, the launch's derived values), the end of a microsecond, closing the launch, and
// the float64 typing's constants.
//
// Each of the opening, the end of a microsecond and the close is written ONCE, as text (the WEDM_ENV_* macros below) that a
// kernel expands in its own body: the compiler then sees the tokens it saw when every kernel carried them, and every
// kernel's code is what it was (profiles/r12/asm_parent_vs_lifecycle_text.txt).  Wrapped in functions, the same lines moved
// the register kernels' and the LDS kernels' allocation ("The launch lifecycle").  The text names the
// includer's `k`, `cold`, `e`, `live`, `s`, `ps` and its forms `F`; a form-dependent call takes F, so a family without the
// form expands a no-op, and a new bound block that touches a piece edits that piece and nothing else.
//
// Who expands what:
//   * the opening (WEDM_ENV_LOAD, WEDM_ENV_RESET, WEDM_ENV_START): wedm_step_regs, wedm_step_regs_wide, wedm_step_fused,
//     wedm_step_packed, wedm_step_lanes and wedm_step_lanes_pk.  A kernel puts its own statements between the pieces (the
//     register kernels load the wire, the LDS kernels take their column, the F_SIG forms load their accumulators).
//     wedm_step_lanes_pk and wedm_step_global form `reinit` themselves, in front of sig_load, and expand WEDM_ENV_RESET_UNDER
//     (formed behind it, the SIG forms' code moves).  wedm_step_global, which leaves early with a frozen lane, and the served
//     kernels' scalar wave, whose lanes past the batch need more members and whose launches never unfreeze, expand the reset
//     around their own load and start.  wedm_step_split opens under its first wave through env_open / env_start below, which
//     expand the text: expanded in place, that kernel's code moved.
//   * the end of a microsecond (WEDM_ENV_END_US / WEDM_ENV_STEP_DONE) and the close (WEDM_ENV_CLOSE): the two register
//     kernels in place; every other family through env_end_us / env_step_done / env_close, which expand the same text.
//   * launch_hot and stencil_f64_consts: the families with those forms (the register kernels read the uniform constants).
//   * wedm_step_stream keeps its own opening and close (scalar loads, state stores split around the epilogue, the reward
//     from a register).
//
// The helpers are __forceinline__ and take Env / Hot / Persist the way the other device helpers do (a real
// call with Env by reference puts the hot loop's state into memory).  `writer` is the one lane of an environment that
// touches memory.  A kernel without signal-statistics forms hands in a `Sig` that nothing reads.
//
// Included by wedm_common.h, after KArgs and the kernarg_* accessors.
#pragma once

// The launch's every-step constants: k.hot, or (F_ENVP / F_MAT) the lane's copy with environment e's rows, the material's
// applied after the physics rows.  A lane past the batch reads environment 0's rows (the rows hold `stride` columns).
template <uint32_t F>
__device__ __forceinline__ Hot launch_hot(const KArgs& k, const ColdRef cold, int64_t e, bool live) {
    Hot hv = k.hot;
    if (F & (F_ENVP | F_MAT)) {
        const int64_t er = live ? e : 0;
        if (F & F_ENVP) envp_apply(hv, cold->s.stride, er);
        if (F & F_MAT) wmat_apply(hv, cold->s.stride, er);
    }
    return hv;
}

// ---- the opening, in three pieces
// Environment e's state rows, or the values of a lane past the batch (which never runs physics and never stores).
#define WEDM_ENV_LOAD()                                                                                       \
    if (live) load_env(cold, e, s);                                                                           \
    else { s.done = WEDM_DEAD_LANE; s.unwind = 0.0; s.h_base = 0.0f; s.h_zone = 0.0f; }

// The next-step autoreset -- an environment found terminated is reset inside the launch; all lanes of an environment agree,
// the writer lane clears its memory, the bound blocks' rows included -- and then `wipe`: the includer sets its own image of
// the wire to the spool temperature (LDS column, global words; empty where it wipes afterwards, as the register kernels do
// under __any(reinit)).  `sg`: the lane's signal-statistics accumulators.
#define WEDM_ENV_RESET_UNDER(reinit, writer, sg, wipe)                                                        \
    if (reinit) {                                                                                             \
        reinit_env(cold, e, s, writer);                                                                       \
        pulse_reinit<(F & F_PULSE) != 0>(kernarg_pulse(), cold, e, writer);                                   \
        if constexpr ((F & F_SIG) != 0) sig_reinit<true>(kernarg_sig(), cold, e, writer, sg);                 \
        wipe;                                                                                                 \
    }
#define WEDM_ENV_RESET(writer, sg, wipe)                                                                      \
    const bool reinit = live && s.done && WEDM_AUTORESET(cold);                                               \
    WEDM_ENV_RESET_UNDER(reinit, writer, sg, wipe)

// What a launch derives once from the opened state: the peak current of the latched mode and the coefficients no module
// changes.  (keep_stepping_terminated: the DONE row is `terminated` of the last step and freezes nothing, so it is taken
// out first.)  `frozen0` receives whether the environment is terminated and sits the launch out (a declaration, or a
// variable of the includer); `report`: what the includer tells the host about it (WEDM_REPORT_FROZEN, or nothing).
#define WEDM_ENV_START(frozen0, report)                                                                       \
    unfreeze_wire(k.hot, s);                                                                                  \
    frozen0 = s.done;                                                                                         \
    report;                                                                                                   \
    if (!s.done) {                                                                                            \
        s.ipk = peak_current(cold, s.mode, e);                                                                \
        init_persist<false, (F & F_MAT) != 0>(k.hot, cold, e, s, ps);                                         \
    }

// ---- the end of a microsecond
// What follows the walk of a microsecond the environment ran: the epilogue on the step's maximum temperature, the pulse
// tally against `prev_pulse` (pulse_kind() before the step's prelude; F_PULSE forms), the signal-statistics tally into the
// lane's accumulators `sg` (F_SIG forms) and, at a control step, the outputs.
#define WEDM_ENV_STEP_DONE(hv, tmax, prev_pulse, writer, sg)                                                  \
    scalar_epilogue(hv, s, tmax);                                                                             \
    pulse_tally<(F & F_PULSE) != 0>(kernarg_pulse(), cold, e, s, prev_pulse, writer);                         \
    if constexpr ((F & F_SIG) != 0) sig_tally<true, (F & F_PULSE) != 0>(kernarg_sig(), cold, e, s, writer, sg); \
    if (s.ctrl) control_step_outputs(cold, e, s, writer);
// The same in a kernel that froze broken wires around its walk (freeze_wire); `mark`: a phase stamp, or nothing
#define WEDM_ENV_END_US(hv, tmax, prev_pulse, writer, sg, mark)                                               \
    unfreeze_wire(hv, s);                                                                                     \
    mark;                                                                                                     \
    if (!s.done) { WEDM_ENV_STEP_DONE(hv, tmax, prev_pulse, writer, sg) }

// ---- the close, in the lane that stores (the environment's writer, not past the batch): the reward -- a frozen environment
// earns nothing, not the previous launch's reward --, the clock's high word and the state rows.  An F_SIG form stores its
// accumulators next to it (sig_store, wedm_device.h), under the same condition.
#define WEDM_ENV_CLOSE(frozen0)                                                                               \
    if (WEDM_REWARD_ON(cold)) {                                                                               \
        if (!frozen0) write_reward(cold, e, s);                                                               \
        else cold->s.reward[e] = 0.0f;                                                                        \
    }                                                                                                         \
    store_time_hi(cold, e, s, (uint32_t)k.n_substeps * (uint32_t)k.hot.dt_us);                                \
    store_env(cold, e, s);

// ---- the same text as helpers, for the families whose code does not depend on how it is wrapped
// The opening for wedm_step_split's first wave (see the head).  env_open returns whether the environment was reset, env_start
// `frozen0`.
template <uint32_t F>
__device__ __forceinline__ bool env_open(const ColdRef cold, int64_t e, bool live, bool writer, Env& s) {
    WEDM_ENV_LOAD()
    Sig none;  // (wedm_step_split has no F_SIG form: nothing reads it)
    WEDM_ENV_RESET(writer, none, )
    return reinit;
}
template <uint32_t F>
__device__ __forceinline__ bool env_start(const KArgs& k, const ColdRef cold, int64_t e, Env& s, Persist& ps) {
    WEDM_ENV_START(const bool frozen0, )
    return frozen0;
}

template <uint32_t F>
__device__ __forceinline__ void env_step_done(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                              bool writer, Sig& sg) {
    WEDM_ENV_STEP_DONE(hv, tmax, prev_pulse, writer, sg)
}
// (the families without F_SIG forms: no accumulators)
template <uint32_t F>
__device__ __forceinline__ void env_step_done(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                              bool writer) {
    static_assert(!(F & F_SIG), "an F_SIG form hands in its accumulators");
    Sig none;
    env_step_done<F>(hv, cold, e, s, tmax, prev_pulse, writer, none);
}

template <uint32_t F>
__device__ __forceinline__ void env_end_us(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                           bool writer, Sig& sg) {
    WEDM_ENV_END_US(hv, tmax, prev_pulse, writer, sg, )
}
template <uint32_t F>
__device__ __forceinline__ void env_end_us(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                           bool writer) {
    static_assert(!(F & F_SIG), "an F_SIG form hands in its accumulators");
    Sig none;
    env_end_us<F>(hv, cold, e, s, tmax, prev_pulse, writer, none);
}

__device__ __forceinline__ void env_close(const KArgs& k, const ColdRef cold, int64_t e, const Env& s, bool frozen0, bool store) {
    if (!store) return;
    WEDM_ENV_CLOSE(frozen0)
}

// The float64 constants of stencil_mode 1 for the forms F (zeros without F_F64): the uniform values of the parameter
// block, environment e's rows where the form binds them
template <uint32_t F>
__device__ __forceinline__ StencilF64 stencil_f64_consts(const ColdRef cold, int64_t e) {
    if (!(F & F_F64)) return StencilF64{0.0, 0.0, 0.0};
    const wedm_params* pp = cold->p;
    return StencilF64{pp->temp_ref,
                      (F & F_MAT) ? WEDM_WMAT_ROW(kernarg_wmat(), WEDM_WM_ALPHA_RHO, cold->s.stride) : pp->alpha_rho,
                      (F & F_ENVP) ? WEDM_ENVP_ROW(kernarg_envp(), WEDM_EP_DIELECTRIC_TEMPERATURE, cold->s.stride) : pp->dielectric_temperature};
}
