// wedm_lifecycle.h — what a step kernel does with an environment around its walk: the launch's `Hot`, opening the
// environment (load, next-step autoreset, the launch's derived values), the end of a microsecond, closing the launch, and
// the float64 typing's constants.
//
// Who calls what ("The launch lifecycle", has the measurements):
//   * the end of a microsecond (env_end_us / env_step_done), the close (env_close), launch_hot and stencil_f64_consts: every
//     family that runs the block except the register kernels.  A new form bit of one of these goes here, and into
//     wedm_step_regs / wedm_step_regs_wide, which keep all of their lifecycle as text (converted, the rows held but the
//     kernels timed 0.3 - 3 % slower).
//   * the opening (env_open, env_start): wedm_step_split only.  Every other family still carries the opening as its own
//     text, because wrapped in these helpers its register rows moved: a new form bit of the OPENING is a hand edit of each
//     of those kernels as well.
//   * wedm_step_stream keeps its own opening and close (scalar loads, state stores split around the epilogue, the reward
//     from a register).
//
// All of them are __forceinline__ and take Env / Hot / Persist the way the other device helpers do (a real
// call with Env by reference puts the hot loop's state into memory).  `writer` is the one lane of an environment that
// touches memory; F is the kernel's set of form bits.
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

// Opens environment e in this lane: its state rows, or the values of a lane past the batch (which never runs physics and
// never stores), then the next-step autoreset -- an environment found terminated is reset inside the launch; all lanes of
// an environment agree, the writer lane clears its memory, the pulse block's rows included.  Returns whether it was reset:
// the caller then sets its own image of the wire to the spool temperature (LDS column, registers, global words).
template <uint32_t F>
__device__ __forceinline__ bool env_open(const ColdRef cold, int64_t e, bool live, bool writer, Env& s) {
    if (live) load_env(cold, e, s);
    else { s.done = WEDM_DEAD_LANE; s.unwind = 0.0; s.h_base = 0.0f; s.h_zone = 0.0f; }
    const bool reinit = live && s.done && WEDM_AUTORESET(cold);
    if (reinit) {
        reinit_env(cold, e, s, writer);
        pulse_reinit<(F & F_PULSE) != 0>(kernarg_pulse(), cold, e, writer);
    }
    return reinit;
}

// What a launch derives once from the opened state: the peak current of the latched mode and the coefficients no module
// changes.  (keep_stepping_terminated: the DONE row is `terminated` of the last step and freezes nothing, so it is taken
// out first.)  Returns `frozen0`: the environment is terminated and sits the launch out.
template <uint32_t F>
__device__ __forceinline__ bool env_start(const Hot& hot, const ColdRef cold, int64_t e, Env& s, Persist& ps) {
    unfreeze_wire(hot, s);
    const bool frozen0 = s.done;
    if (!s.done) {
        s.ipk = peak_current(cold, s.mode, e);
        init_persist<false, (F & F_MAT) != 0>(hot, cold, e, s, ps);
    }
    return frozen0;
}

// What follows the walk of a microsecond the environment ran: the epilogue on the step's maximum temperature, the pulse
// tally against `prev_pulse` (pulse_kind() before the step's prelude; F_PULSE forms), the signal-statistics tally into the
// lane's accumulators `sg` (F_SIG forms) and, at a control step, the outputs.
template <uint32_t F>
__device__ __forceinline__ void env_step_done(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                              bool writer, Sig& sg) {
    scalar_epilogue(hv, s, tmax);
    pulse_tally<(F & F_PULSE) != 0>(kernarg_pulse(), cold, e, s, prev_pulse, writer);
    sig_tally<(F & F_SIG) != 0, (F & F_PULSE) != 0>(kernarg_sig(), cold, e, s, writer, sg);
    if (s.ctrl) control_step_outputs(cold, e, s, writer);
}
// (the families without F_SIG forms: no accumulators)
template <uint32_t F>
__device__ __forceinline__ void env_step_done(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                              bool writer) {
    static_assert(!(F & F_SIG), "an F_SIG form hands in its accumulators");
    Sig none;
    env_step_done<F>(hv, cold, e, s, tmax, prev_pulse, writer, none);
}

// The end of a microsecond in a kernel that froze broken wires around its walk (freeze_wire)
template <uint32_t F>
__device__ __forceinline__ void env_end_us(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                           bool writer, Sig& sg) {
    unfreeze_wire(hv, s);
    if (!s.done) env_step_done<F>(hv, cold, e, s, tmax, prev_pulse, writer, sg);
}
template <uint32_t F>
__device__ __forceinline__ void env_end_us(const Hot& hv, const ColdRef cold, int64_t e, Env& s, float tmax, int32_t prev_pulse,
                                           bool writer) {
    static_assert(!(F & F_SIG), "an F_SIG form hands in its accumulators");
    Sig none;
    env_end_us<F>(hv, cold, e, s, tmax, prev_pulse, writer, none);
}

// Closes the launch, in the lane for which `store` holds (the environment's writer, not past the batch): the reward -- a
// frozen environment earns nothing, not the previous launch's reward --, the clock's high word and the state rows.  An
// F_SIG form stores its accumulators next to it (sig_store, wedm_device.h), under the same `store`.
__device__ __forceinline__ void env_close(const KArgs& k, const ColdRef cold, int64_t e, const Env& s, bool frozen0, bool store) {
    if (!store) return;
    if (WEDM_REWARD_ON(cold)) {
        if (!frozen0) write_reward(cold, e, s);
        else cold->s.reward[e] = 0.0f;
    }
    store_time_hi(cold, e, s, (uint32_t)k.n_substeps * (uint32_t)k.hot.dt_us);
    store_env(cold, e, s);
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
