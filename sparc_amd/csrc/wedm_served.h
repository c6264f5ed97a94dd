// wedm_served.h — "served" kernels: the float64 scalar physics of a block's environments on a wave of its own.
//
// Included by wedm_kernels.hip behind wedm_common.h (KArgs, WalkTable, copy_wire, PackedSlot, tile_staged) and wedm_k_regs.h.
// Here: the mailbox, both sides of its protocol written once each (served_scalar_wave; the walkers' behind sv_wait), and
// wedm_step_served and wedm_step_regs_served.  The third kernel that runs it, wedm_step_lanes_served, is in wedm_lanes2.h.
// The walkers of wedm_step_served run the text of wedm_packed_walk.inc (wedm_step_packed's walk, column stride 192, the frozen
// flag from the mailbox) with this kernel's own tiles and tails; those of wedm_step_regs_served the text of wedm_regs_walk.inc.
//
// Why.  In every kernel with L >= 4 lanes per environment the scalar physics of a microsecond (wire_edm.py:116-157 without
// the stencil: ~340 wave-level instructions, most of them float64) is executed by every lane of the environment -- once per
// WAVE, i.e. per 64 / L environments: 43 of the 103 wave-instructions per env-step of wedm_step_packed<8> at 32 768 x 400, 85 of
// the 214 of wedm_step_lanes<8> (profiles/valu.json, round 3).  The reference runs that chain once per environment-step.  Here
// a block's last wave is the SCALAR wave: lane i of it owns environment i of the block (its whole Env in registers) and
// runs prelude and epilogue once per environment and microsecond; the other WW (three) waves are WALKER waves: they own the
// wire (in LDS, as in wedm_step_packed) and nothing else -- no Env, no float64 -- and get the six stencil coefficients of a
// microsecond through a mailbox in LDS.  Blocks of FOUR waves (3 walkers + 1 scalar, 24 environments at 8 lanes each), three
// of them per CU at a 168-register budget: a block of 4 + 1 waves is admitted only ONCE per CU at that budget although the
// occupancy API answers 2 (census by HW_ID, tools/stamps_served.py: the dispatcher wants room for ceil(5 / 4) = 2 waves on
// EVERY SIMD per block), and one such block per CU is as fast as wedm_step_packed and no faster.
//
// Protocol (LDS operations of one wave are processed in order; all waves of a block are resident together):
//   scalar wave, step k : prelude(k) -> cf[k & 1][env] (jf, q, plasma cell, flags, convection pair) -> cf_seq = k + 1
//   walker wave, step k : spin until cf_seq > k -> walk(k) -> tmax[k & 1][env] -> tm_seq[wave] = k + 1
//   scalar wave         : reads tmax(k) when tm_seq[every walker wave] > k
// The scalar wave runs ONE STEP AHEAD: the only thing the epilogue of step k needs from the walk is max(T) (wire.py:376-388:
// time above the critical temperature; the break test, after which the reference returns before mechanics and clocks).  Where
// the scalar wave can PROVE from max(T) of step k - 1 and the coefficients of step k that step k cannot break the wire, it runs
// the rest of the epilogue (mechanics, clocks, termination) and the prelude of step k + 1 while the walkers are still in step
// k, and applies the temperature monitor of step k when its maximum arrives.  The proof is a maximum principle of the explicit
// scheme: with every coefficient non-negative and tuf (2 k + conv + adv) <= 1,
//       max(T_new) <= M + tuf (jf (1 + alpha (M - T_ref)) + max(q, 0)),   M = max(max(T_old), T_dielectric)
// (each new cell is a convex combination of old cells and T_dielectric plus the two source terms; float32 rounding of the ~10
// operations of a cell is below 1e-2 K, the test keeps 1 K).  Where the bound does not stay below the breaking temperature,
// at control steps (the observation carries max(T)) and in the first step of a launch (max(T) of a wire the caller may have
// assigned is unknown) the scalar wave simply waits for the walkers, as an unserved kernel does every step.  Nothing is ever
// rolled back; a break in a step that was proven safe would set the environment's sticky ERROR flag (it cannot happen).
//
// Results are bit-identical to every other kernel: the same prelude / epilogue functions on the same values in the same order
// per environment, the same tile code on the same coefficients.
#pragma once

namespace wedm {

// flags word of a published coefficient set
enum { SV_JOULE = 1, SV_DONE = 2, SV_STOP = 4, SV_ADV = 8 };

template <int EPB>
struct ServedBox {   // lives in LDS behind the wire image
    uint32_t cf_seq;          // steps whose coefficients are published
    uint32_t tm_seq[4];       // per walker wave (at most four): steps whose maxima are published
    uint32_t pad_[3];
    float jf[2][EPB], q[2][EPB], conv_base[2][EPB], conv_zone[2][EPB];
    int32_t pidx[2][EPB], flags[2][EPB];
    float tmax[2][EPB];
    float adv[EPB];
};

// diagnostic build -DWEDM_STAMPS (tools/stamps_served.py): per wave {HW_ID, XCC_ID, start, end (100 MHz clock all XCDs
// share), shader-clock cycles spent spinning, shader-clock cycles in the loop, steps speculated, three phase sums}
#ifdef WEDM_STAMPS
struct SvStamps {
    unsigned long long wait_acc = 0, t0 = 0, t1 = 0, c0 = 0, c1 = 0, spec = 0, pa = 0, pb = 0, pc = 0, q0 = 0, q1 = 0, w0 = 0;
    uint32_t hwid = 0, xcc = 0;
};
#define WEDM_SV_CLOCK(var) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory")
#define WEDM_SV_WAIT_BEGIN() WEDM_SV_CLOCK(svs.w0)
#define WEDM_SV_WAIT_END() do { unsigned long long sv_w1_; WEDM_SV_CLOCK(sv_w1_); svs.wait_acc += sv_w1_ - svs.w0; } while (0)
#define WEDM_SV_PHASE(acc) do { __builtin_amdgcn_sched_barrier(0); WEDM_SV_CLOCK(svs.q1); svs.acc += svs.q1 - svs.q0; svs.q0 = svs.q1; __builtin_amdgcn_sched_barrier(0); } while (0)
#define WEDM_SV_PHASE_START() do { __builtin_amdgcn_sched_barrier(0); WEDM_SV_CLOCK(svs.q0); __builtin_amdgcn_sched_barrier(0); } while (0)
#define WEDM_SV_LOOP_START() WEDM_SV_CLOCK(svs.c0)
#define WEDM_SV_LOOP_END() WEDM_SV_CLOCK(svs.c1)
#define WEDM_SV_COUNT_SPEC() (++svs.spec)
__device__ __forceinline__ void sv_stamps_begin(SvStamps& svs) {
    asm volatile("s_getreg_b32 %0, hwreg(4)\n\ts_getreg_b32 %1, hwreg(20)" : "=s"(svs.hwid), "=s"(svs.xcc));
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(svs.t0)::"memory");
}
// `row`: this wave's 12 words of the stamp buffer (lane 0 writes), or null
__device__ __forceinline__ void sv_stamps_out(SvStamps& svs, unsigned long long* row) {
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(svs.t1)::"memory");
    if (row && (threadIdx.x & 63) == 0) {
        row[0] = svs.hwid; row[1] = svs.xcc; row[2] = svs.t0; row[3] = svs.t1; row[4] = svs.wait_acc; row[5] = svs.c1 - svs.c0;
        row[6] = svs.spec; row[7] = svs.pa; row[8] = svs.pb; row[9] = svs.pc;
    }
}
#else
struct SvStamps { };
#define WEDM_SV_WAIT_BEGIN() do { } while (0)
#define WEDM_SV_WAIT_END() do { } while (0)
#define WEDM_SV_PHASE(acc) do { } while (0)
#define WEDM_SV_PHASE_START() do { } while (0)
#define WEDM_SV_LOOP_START() do { } while (0)
#define WEDM_SV_LOOP_END() do { } while (0)
#define WEDM_SV_COUNT_SPEC() do { } while (0)
__device__ __forceinline__ void sv_stamps_begin(SvStamps&) { }
__device__ __forceinline__ void sv_stamps_out(SvStamps&, unsigned long long*) { }
#endif

__device__ __forceinline__ void sv_wait(const volatile uint32_t* p, uint32_t want) {
    // wave-uniform spin on an LDS word another wave of the block advances (monotone counters: signed distance)
    for (;;) {
        const uint32_t v = __builtin_amdgcn_readfirstlane(*p);
        if ((int32_t)(v - want) >= 0) break;
        __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
}

// the same with one word per lane (the scalar wave: every lane waits for the walker wave of ITS environment)
__device__ __forceinline__ void sv_wait_lanes(const volatile uint32_t* p, uint32_t want) {
    for (;;) {
        const uint32_t v = *p;
        if (__all((int32_t)(v - want) >= 0)) break;
        __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
}

}  // namespace wedm

// ------------------------------------------------------------------------------------- the walkers' side of the mailbox
// Written once for the walkers of the three kernels, which keep their WEDM_SV_WAIT_BEGIN / _END and WEDM_SV_PHASE marks
// around the pieces.  Functions where a function leaves every kernel's code as it was; text the kernel expands (as
// wedm_lifecycle.h's, naming the includer's `box`, `tid`, `it`, `slot`, `el`, `live`, `ps`, `s`, `hv`) where a function moved
// a wave's register allocation: profiles/r13/asm_parent_vs_served_walker.txt.
// Thread 0 of the block, before barrier (A): nothing is published yet.
#define WEDM_SV_BOX_INIT() \
    if (tid == 0) { box->cf_seq = 0u; box->tm_seq[0] = 0u; box->tm_seq[1] = 0u; box->tm_seq[2] = 0u; box->tm_seq[3] = 0u; }
// this wave's 12 words of the stamp buffer (WAVES per block, the scalar wave included), or null
template <int WAVES>
__device__ __forceinline__ unsigned long long* sv_stamp_row(const KArgs& k, int tid) {
    return k.dbg ? k.dbg + ((size_t)blockIdx.x * WAVES + (tid >> 6)) * 12 : nullptr;
}
// next-step autoreset: the environment's wire starts at the spool temperature (the scalar wave re-initialises the state)
__device__ __forceinline__ bool sv_walker_reinit(const ColdRef cold, int64_t stride, int64_t e, bool live) {
    return live && WEDM_AUTORESET(cold) && cold->s.i8[(int64_t)WEDM_B_DONE * stride + e] != 0;
}
// Step `it`: until its coefficients are published; then take those of environment slot `el`: the step's `cf`, the convection
// pair and adv_on of `ps`, and `frozen` (no store into this environment's wire: terminated, or past the batch).  SV_STOP:
// every environment of the block is terminated, the walker leaves its loop (block-wide: every lane reads it).
#define WEDM_SV_WAIT_COEF() sv_wait(&box->cf_seq, (uint32_t)it + 1u)
#define WEDM_SV_TAKE(cf, frozen)                                                                                  \
    const int32_t fl = box->flags[slot][el];                                                                      \
    if (fl & SV_STOP) break;                                                                                      \
    Coef cf{box->jf[slot][el], box->q[slot][el], (fl & SV_JOULE) ? 1 : 0, box->pidx[slot][el]};                   \
    ps.conv_base = box->conv_base[slot][el];                                                                      \
    ps.conv_zone = box->conv_zone[slot][el];                                                                      \
    ps.adv_on = (fl & SV_ADV) ? 1 : 0;                                                                            \
    const bool frozen = !live || (fl & SV_DONE);
// Give the environment's maximum of step `it` (`first`: the environment's first lane writes it).  The store order is the
// protocol's: the data word, then the compiler barrier, then the sequence word of this walker wave (by its first lane).
template <int EPB>
__device__ __forceinline__ void sv_give(volatile ServedBox<EPB>* box, int slot, int el, bool first, int tid, int wave, int it, float tmax) {
    if (first) box->tmax[slot][el] = tmax;
    asm volatile("" ::: "memory");
    if ((tid & 63) == 0) box->tm_seq[wave] = (uint32_t)it + 1u;
}
// The scalar wave applies the temperature monitor (wire.py:376-388) of a step it ran ahead of, when the maximum `tm` is
// there.  The step was proven not to break the wire: a break here is impossible, and loud (the sticky ERROR flag).
#define WEDM_SV_APPLY_MONITOR(tm)                                                                                 \
    s.tcrit = (tm) > hv.tcrit ? s.tcrit + 1 : 0;                                                                  \
    s.tmax = (tm);                                                                                                \
    if ((tm) > hv.tbreak) { s.err = 1; s.broken = 1; s.done = hv.done_value; }

#ifndef WEDM_SERVED_STAGE_W
#define WEDM_SERVED_STAGE_W 2  // pairs per stage of the packed walk
#endif
#ifndef WEDM_SERVED_WAVES_PER_EU
#define WEDM_SERVED_WAVES_PER_EU 3
#endif

// ------------------------------------------------------------------------------------------------ the scalar wave
// Lane `sl` owns environment e0 + sl of the block (EPB of them); the walker waves hold LPE lanes per environment, so the
// maxima of environment sl come from walker wave (sl * LPE) / 64.  Runs from the launch's first barrier to its last store.
template <int EPB, int LPE>
__device__ __forceinline__ void served_scalar_wave(const KArgs& k, const ColdRef cold, volatile ServedBox<EPB>* box, int64_t e0, int sl,
                                                   SvStamps& svs, unsigned long long* stamp_row) {
    const float spool = k.hot.spool, tref = k.hot.tref, alpha = k.hot.alpha, tdiel = k.hot.tdiel;
#ifdef WEDM_SV_NO_SCALAR  // (register-pressure probes of the two roles: tools/kernel_resources.py -DWEDM_SV_NO_...)
    return;
#endif
    __builtin_amdgcn_s_setprio(3);  // its chain is on the critical path of four walker waves
    Hot hv = k.hot;  // (no pinned constants: the scalar wave's 168 registers hold an Env and a prelude's temporaries, nothing to spare)
    const int64_t e = e0 + (sl < EPB ? sl : 0);
    const bool live = sl < EPB && e0 + sl < k.num_envs;
    Env s;
    Geom g;
    Persist ps{0.0f, 0.0f, 0.0f, 0};
    load_geom(k.hot, cold, live ? e : 0, g);
    if (live) load_env(cold, e, s);
    else { s.done = WEDM_DEAD_LANE; s.unwind = 0.0; s.h_base = 0.0f; s.h_zone = 0.0f; s.broken = 0; s.ctrl = 0; s.tmax = spool; s.tcrit = 0; }
    constexpr uint32_t F = 0;  // (the served kernels have no bound-block forms)
    Sig none;                  // (nothing reads it)
    WEDM_ENV_RESET(true, none, )
    const bool frozen0 = s.done;
    if (!s.done) {
        s.ipk = peak_current(cold, s.mode, e);
        init_persist(k.hot, cold, e, s, ps);
    }
    const uint32_t gid = k.hot.env_id_offset + (uint32_t)e;
    if (sl < EPB) box->adv[sl] = ps.adv;
    __syncthreads();  // (A) the walkers have staged the wire; the mailbox is initialised

    // the maximum principle needs non-negative coefficients and the explicit scheme inside its stability limit
    const float kf = g.k, tuf = g.tuf;
    bool pending = false;      // the previous step's temperature monitor is still to be applied (wave-uniform)
    bool pend_live = false;    // ... for this lane
    bool have_m = false;       // max(T) of the wire as it is now is known (wave-uniform): not in a launch's first step
    float M = spool;
    int it = 0;
    WEDM_SV_LOOP_START();
    for (; it < k.n_substeps; ++it) {
        const int slot = it & 1;
        if (__all(s.done != 0)) {  // every environment of the block is terminated: the walkers stop too
            if (sl < EPB) box->flags[slot][sl] = SV_STOP | SV_DONE;
            asm volatile("" ::: "memory");
            if (sl == 0) box->cf_seq = (uint32_t)it + 1u;
            break;
        }
        WEDM_SV_PHASE_START();
        Coef cf{0.0f, 0.0f, 0, -1};
        QuietTry qt;
#ifdef WEDM_SV_STUB_SCALAR  // (instruction-count probe: the scalar wave publishes a quiet step and computes nothing; results are garbage)
        const bool was_quiet = true;
        qt.have_w = false;
#else
        const bool was_quiet = quiet_prelude_t<kPackedDense>(hv, cold, g, e, gid, s, qt, cf);
#endif
        // (inlined: as a real function call the general prelude measured 9.8 ms against 8.3 ms at 32 768 x 400 -- the values
        // that live across the call are spilled around it in the hot loop too)
        if (__builtin_expect(!was_quiet && !s.done, 0)) cf = scalar_prelude(hv, cold, g, e, gid, s, ps, true, qt);
        const float jf_eff = (cf.joule_on && !s.done) ? cf.jf : 0.0f;
        if (sl < EPB) {
            box->jf[slot][sl] = cf.jf; box->q[slot][sl] = cf.q; box->pidx[slot][sl] = cf.pidx;
            box->conv_base[slot][sl] = ps.conv_base; box->conv_zone[slot][sl] = ps.conv_zone;
            box->flags[slot][sl] = (cf.joule_on ? SV_JOULE : 0) | (s.done ? SV_DONE : 0) | (ps.adv_on ? SV_ADV : 0);
        }
        asm volatile("" ::: "memory");
        if (sl == 0) box->cf_seq = (uint32_t)it + 1u;
        WEDM_SV_PHASE(pa);  // prelude and publication
        // ---- the previous step's temperature monitor, now that its maximum is there (the walkers had a prelude's time)
        if (pending) {
            { WEDM_SV_WAIT_BEGIN(); sv_wait_lanes(&box->tm_seq[(sl < EPB ? sl * LPE : 0) >> 6], (uint32_t)it); WEDM_SV_WAIT_END(); }
            const float tm = sl < EPB ? box->tmax[slot ^ 1][sl] : spool;
            if (pend_live) {
                WEDM_SV_APPLY_MONITOR(tm)
                M = tm;
            }
            pending = false;
            have_m = true;
        }
        WEDM_SV_PHASE(pb);  // wait for and apply the previous step's monitor
        // ---- can this step break the wire?
        // (the proof reads the uniform tbreak / alpha and the uniform kf / tuf: the served kernels take uniform geometry only,
        // so with a per-environment wire material bound -- which needs per-environment geometry -- they are never reached;
        // choose_kernel refuses them by name)
        const float Mb = fmaxf(M, tdiel);
        const float conv_max = fmaxf(ps.conv_base, ps.conv_zone);
        const bool scheme_ok = kf >= 0.0f && tuf > 0.0f && alpha >= 0.0f && ps.conv_base >= 0.0f && ps.conv_zone >= 0.0f &&
                               ps.adv >= 0.0f && jf_eff >= 0.0f && tuf * (2.0f * kf + conv_max + ps.adv) <= 1.0f;
        const float rise = tuf * (jf_eff * (1.0f + alpha * (Mb - tref)) + fmaxf(cf.q, 0.0f));
        const bool safe = s.done || (scheme_ok && !s.ctrl && Mb + rise + 1.0f < hv.tbreak);  // (a NaN anywhere: not safe)
        if (have_m && __all(safe)) {
            // proven: no lane's wire breaks in this step -> the rest of the epilogue now, the monitor when the maximum arrives
            pend_live = !s.done;
            WEDM_SV_COUNT_SPEC();
#ifndef WEDM_SV_STUB_SCALAR
            if (!s.done) {
                epilogue_voltage_sum(s);
                epilogue_motion(hv, s);
            }
#endif
            pending = true;
        } else {
            { WEDM_SV_WAIT_BEGIN(); sv_wait_lanes(&box->tm_seq[(sl < EPB ? sl * LPE : 0) >> 6], (uint32_t)it + 1u); WEDM_SV_WAIT_END(); }
            const float tm = sl < EPB ? box->tmax[slot][sl] : spool;
            if (!s.done) {
                env_step_done<0>(hv, cold, e, s, tm, 0, true);
                M = tm;
            }
            have_m = true;
        }
        WEDM_SV_PHASE(pc);  // the proof and the rest of the epilogue
    }
    if (pending) {  // the last step's monitor
        sv_wait_lanes(&box->tm_seq[(sl < EPB ? sl * LPE : 0) >> 6], (uint32_t)it);
        const float tm = sl < EPB ? box->tmax[(it - 1) & 1][sl] : spool;
        if (pend_live) {
            WEDM_SV_APPLY_MONITOR(tm)
        }
    }
    WEDM_SV_LOOP_END();
    sv_stamps_out(svs, stamp_row);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // (B) the walkers' last step is in LDS
    env_close(k, cold, e, s, frozen0, live);
}

// ============================================ served packed kernel: L lanes / env, 2 cells / op, scalar physics on a wave of its own
// Walk, LDS image and tile table are wedm_step_packed's (two virtual chunks per lane in float2 registers; the table built for
// 2 L chunks; one-change tiles and 1- / 2-cell tails with F_EXTRA).  A wave with a frozen (terminated) environment keeps
// the tile code, its lanes do not store (wedm_step_packed's F_FROZEN_OK, always on here).
// Not here (the launch plan keeps such launches on wedm_step_packed): a trace sample inside the launch, keep_stepping_terminated.
// This kernel's pieces of the walk, expanded by wedm_packed_walk.inc where it uses them (its head says what each has to do).
// Tail cells: ONE packed pair per tail position -- both virtual chunks together, the Joule term only where some lane of the
// wave carries current, exactly as the tiles do it -- instead of two scalar cells with the Joule term always.
#define WEDM_PACKED_WALK_TAILS_FROM_OLD()                                                                                      \
    f2 ttp[2] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}}; /* [q] = (chunk A, chunk B) */                                               \
    if (use_tail) {                                                                                                            \
        const float jfl = (cf.joule_on && !done) ? cf.jf : 0.0f;                                                               \
        const bool joule_tail = __any(jfl != 0.0f);                                                                            \
        _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                        \
            if (q < tail) {                                                                                                    \
                const int r = Cv - tail + q;                                                                                   \
                const uint32_t ba = tail_bits >> (4 * (2 * q)), bb = tail_bits >> (4 * (2 * q + 1));                           \
                const f2 tm = {col[(2 * (r - 1)) * CS], col[(2 * (r - 1) + 1) * CS]};                                          \
                const f2 tcc = {col[(2 * r) * CS], col[(2 * r + 1) * CS]};                                                     \
                const f2 tp = {col[(2 * (r + 1)) * CS], col[(2 * (r + 1) + 1) * CS]};                                          \
                const f2 conv = {(ba & 1u) ? ps.conv_zone : ps.conv_base, (bb & 1u) ? ps.conv_zone : ps.conv_base};            \
                const f2 jfe = {(ba & 2u) ? jfl : 0.0f, (bb & 2u) ? jfl : 0.0f};                                               \
                ttp[q] = joule_tail ? interior2<true>(tm, tcc, tp, g.k, g.tuf, conv, tdiel, ps.adv, jfe, alpha, tref)          \
                                    : interior2<false>(tm, tcc, tp, g.k, g.tuf, conv, tdiel, ps.adv, jfe, alpha, tref);        \
            }                                                                                                                  \
        }                                                                                                                      \
    }
#define WEDM_PACKED_WALK_TAIL_NEW(q, v) ((v) ? ttp[q].y : ttp[q].x)
#define WEDM_PACKED_WALK_DONE done
#define WEDM_PACKED_WALK_REGULAR_TILE(JOULE)                                 \
    _Pragma("unroll") for (int o = 0; o < 8; o += WEDM_SERVED_STAGE_W)       \
        tile_staged<f2, JOULE, false, WEDM_SERVED_STAGE_W>(old, tn, o, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref)
#define WEDM_PACKED_WALK_ONECHANGE_TILE() percell_tile(joule_wave, old, tn, split, conv_lo, conv_hi, jfe_lo, jfe_hi)

template <int L, uint32_t F>
__global__ void __launch_bounds__(256, WEDM_SERVED_WAVES_PER_EU) wedm_step_served(const KArgs k) {
    static_assert((F & ~F_EXTRA) == 0, "forms of wedm_step_served");
    constexpr bool EXTRA = (F & F_EXTRA) != 0;
    constexpr int WW = 3;         // walker waves; with the scalar wave, blocks of (WW + 1) * 64 = 256 threads
    constexpr int NT = WW * 64;   // walker threads = columns of the LDS image
    constexpr int EPB = NT / L;   // environments per block
    static_assert(EPB <= 64 && WW <= 4, "one lane of the scalar wave per environment of the block");
    typedef ServedBox<EPB> Box;
    const ColdRef cold = kernarg_cold();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    const WalkTable* __restrict__ wt = k.walk;  // built for 2L virtual chunks
    const int Cv = wt->C;
    const int R = 2 * Cv;  // data rows per lane; rows R and R+1 are the halo pair
    const int n = k.hot.n_seg;
    const int64_t stride = cold->s.stride;
    volatile Box* const box = (volatile Box*)(lds + (size_t)(R + 2) * NT);
    const float spool = k.hot.spool, tref = k.hot.tref, alpha = k.hot.alpha, tdiel = k.hot.tdiel;
    const bool scalar_wave = tid >= NT;
    SvStamps svs;
    sv_stamps_begin(svs);
    unsigned long long* const stamp_row = sv_stamp_row<WW + 1>(k, tid);

    WEDM_SV_BOX_INIT()

    if (scalar_wave) {
        served_scalar_wave<EPB, L>(k, cold, box, e0, tid - NT, svs, stamp_row);
        return;
    }

    // ---------------------------------------------------------------------------------------------------- the walker waves
#ifdef WEDM_SV_NO_WALK
    return;
#endif
    const int el = tid / L, c = tid % L;
    const int64_t e = e0 + el;
    const bool live = e < k.num_envs;
    const int wave = tid >> 6;
    // ---- stage
    const PackedSlot<NT> wire_slot{Cv};
    copy_wire<L, true, NT>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
    Geom g;
    load_geom(k.hot, cold, 0, g);  // uniform geometry
    float* col = lds + tid;
    const bool reinit = sv_walker_reinit(cold, stride, e, live);
    __syncthreads();  // (A)
    if (reinit) {
        for (int row = 0; row < R; ++row) col[row * NT] = spool;
    }
    Persist ps{box->adv[el], 0.0f, 0.0f, 0};

    const int baseA = 2 * c * Cv, baseB = baseA + Cv;  // first wire cell of each virtual chunk
    const int n_tiles = wt->n_tiles;
    constexpr int CS = NT;             // column stride of the LDS image: one column per walker thread
    constexpr bool FROZEN_OK = true;   // (wedm_step_packed's F_FROZEN_OK, always on here)
#define WEDM_PACKED_WALK_SETUP
#include "wedm_packed_walk.inc"
#undef WEDM_PACKED_WALK_SETUP

    WEDM_SV_LOOP_START();
    for (int it = 0; it < k.n_substeps; ++it) {
        const int slot = it & 1;
        { WEDM_SV_WAIT_BEGIN(); WEDM_SV_WAIT_COEF(); WEDM_SV_WAIT_END(); }
        WEDM_SV_PHASE_START();
        WEDM_SV_TAKE(cf, done)

        float tmax = spool;
        // a tile with one coefficient change at `split`: the pairs' coefficients are selected group by group, right before
        // the stage-major group that uses them (all eight up front are 32 registers the walker does not have)
        auto percell_tile = [&](bool joule_wave, const f2 (&old)[10], f2 (&tn)[8], int split, f2 conv_lo, f2 conv_hi, f2 jfe_lo, f2 jfe_hi) {
            constexpr int W = WEDM_SERVED_STAGE_W;
#pragma unroll
            for (int o = 0; o < 8; o += W) {
                f2 cv[8], jv[8];  // (only entries o .. o + W - 1 are set and read)
#pragma unroll
                for (int u = 0; u < W; ++u) {
                    cv[o + u] = (o + u) < split ? conv_lo : conv_hi;
                    jv[o + u] = (o + u) < split ? jfe_lo : jfe_hi;
                }
                if (joule_wave) tile_staged<f2, true, true, W>(old, tn, o, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
                else tile_staged<f2, false, true, W>(old, tn, o, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
            }
        };
        constexpr bool kWalkTiles = true;
#define WEDM_PACKED_WALK_MARK_TILES WEDM_SV_PHASE(pa)    // mailbox, halos, patched cells and tails from old values
#define WEDM_PACKED_WALK_MARK_PATCHES WEDM_SV_PHASE(pb)  // the tiles
#define WEDM_PACKED_WALK_US
#include "wedm_packed_walk.inc"
#undef WEDM_PACKED_WALK_US
#undef WEDM_PACKED_WALK_MARK_TILES
#undef WEDM_PACKED_WALK_MARK_PATCHES
        tmax = max_over_env_lanes<L>(tmax);
        sv_give(box, slot, el, c == 0, tid, wave, it, tmax);
        WEDM_SV_PHASE(pc);  // patches, reduction, publication
    }

    WEDM_SV_LOOP_END();
    sv_stamps_out(svs, stamp_row);
    __syncthreads();  // (B)
    copy_wire<L, false, NT>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
}
#undef WEDM_PACKED_WALK_TAILS_FROM_OLD
#undef WEDM_PACKED_WALK_TAIL_NEW
#undef WEDM_PACKED_WALK_DONE
#undef WEDM_PACKED_WALK_REGULAR_TILE
#undef WEDM_PACKED_WALK_ONECHANGE_TILE

// ============================================ served register kernel: the wire in the walkers' registers, no LDS image
// wedm_step_regs<2>'s walk (wedm_regs_walk.inc) on TWO walker waves of a block -- two lanes per environment, 32 packed
// pairs each --, the scalar physics of the block's 64 environments on a third wave, all 64 of its lanes busy.  Blocks of three
// waves, four to a CU at 168 registers: 256 environments per CU, 65 536 in ONE round.  LDS holds the mailbox only.
// By name only (kernel 12), measured at 65 536 x 128 (round 4): fused launches 1.666e10 env-steps/s against wedm_step_regs<2>'s
// 1.674e10 -- a sixth fewer instructions, given back by spills: the walk with 64 wire registers per lane wants 239 registers
// and spills 53 at the 168 that three waves per SIMD leave, the scalar wave 113 -- and launches of ONE microsecond 41.7 us
// against wedm_step_stream's 20.4 us (every state row loaded and stored, scratch traffic cold at every launch).
template <uint32_t F>
__global__ void __launch_bounds__(192, WEDM_SERVED_WAVES_PER_EU) wedm_step_regs_served(const KArgs k) {
    static_assert(F == 0, "wedm_step_regs_served has one form");
    constexpr int CELLS = 128, L = 2, H = CELLS / (2 * L), EPB = 64, NT = 128;
    static_assert(H % 8 == 0 && H / 8 <= 16, "whole tiles");
    constexpr int SW = WEDM_REGS_SW2;
    typedef ServedBox<EPB> Box;
    const ColdRef cold = kernarg_cold();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    volatile Box* const box = (volatile Box*)lds;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    SvStamps svs;
    sv_stamps_begin(svs);
    unsigned long long* const stamp_row = sv_stamp_row<3>(k, tid);
    WEDM_SV_BOX_INIT()
    if (tid >= NT) {
        served_scalar_wave<EPB, L>(k, cold, box, e0, tid - NT, svs, stamp_row);
        return;
    }

    // ---------------------------------------------------------------------------------------------------- the walker waves
    const int c = tid % L, el = tid / L, wave = tid >> 6;
    const int64_t e = e0 + el;
    const bool live = e < k.num_envs;
    const WalkTable* __restrict__ wt = k.walk;  // 2 L chunks of H cells
    const int n = k.hot.n_seg;
    const int64_t stride = cold->s.stride;
    const int base = c * 2 * H;  // this lane's first cell
    const float spool = k.hot.spool, tref = k.hot.tref, alpha = k.hot.alpha, tdiel = k.hot.tdiel;
    WEDM_REGS_LOAD_WIRE()  // (the wire first)
    Geom g;
    load_geom(k.hot, cold, 0, g);  // uniform geometry
    const bool reinit = sv_walker_reinit(cold, stride, e, live);
    WEDM_REGS_WIPE_WIRE()
    // tile flags of this lane's two chunks (bit t: the tile's first cell lies in the workpiece zone / between the contacts)
    const int n_tiles = wt->n_tiles;
    uint32_t zoneA = 0u, zoneB = 0u, jouleA = 0u, jouleB = 0u, joule_any = 0u;
    for (int t = 0; t < n_tiles; ++t) {
        const uint32_t lo = wt->zj[8 * t];
        zoneA |= ((lo >> (2 * c)) & 1u) << t;       zoneB |= ((lo >> (2 * c + 1)) & 1u) << t;
        jouleA |= ((lo >> (16 + 2 * c)) & 1u) << t; jouleB |= ((lo >> (17 + 2 * c)) & 1u) << t;
        joule_any |= ((lo >> 16) != 0u ? 1u : 0u) << t;
    }
    joule_any = __builtin_amdgcn_readfirstlane(joule_any);
    const uint32_t kind_n = __builtin_amdgcn_readfirstlane(wt->kind_n_mask);
    const uint32_t kind_ne = __builtin_amdgcn_readfirstlane(wt->kind_ne_mask), kind_nj = __builtin_amdgcn_readfirstlane(wt->kind_nj_mask);
    const int last_base = (2 * L - 1) * H;
    const uint32_t last_tile = (n > last_base) ? (1u << ((n - 1 - last_base) >> 3)) : 0u;
    const bool owns_last = c == L - 1;
    __syncthreads();  // (A) the mailbox is initialised, the scalar wave has published the advection coefficients
    Persist ps{box->adv[el], 0.0f, 0.0f, 0};
    f2 convp[H / 8];  // the convection coefficient pair (chunk A, chunk B) of every tile, from the published coefficients

    WEDM_SV_LOOP_START();
    for (int it = 0; it < k.n_substeps; ++it) {
        const int slot = it & 1;
        { WEDM_SV_WAIT_BEGIN(); WEDM_SV_WAIT_COEF(); WEDM_SV_WAIT_END(); }
        WEDM_SV_PHASE_START();
        WEDM_SV_TAKE(cf, frozen)
        const bool act = !frozen;
#pragma unroll
        for (int t = 0; t < H / 8; ++t)
            convp[t] = f2{((zoneA >> t) & 1u) ? ps.conv_zone : ps.conv_base, ((zoneB >> t) & 1u) ? ps.conv_zone : ps.conv_base};
        float tmax = spool;
        asm volatile("" : "+v"(zoneA), "+v"(zoneB), "+v"(jouleA), "+v"(jouleB));  // (see wedm_step_regs: the rare code's predicates stay where they are used)
        Geom gw = g;
        gw.n_seg = __builtin_amdgcn_readfirstlane(g.n_seg); gw.az_start = __builtin_amdgcn_readfirstlane(g.az_start);
        gw.az_end = __builtin_amdgcn_readfirstlane(g.az_end); gw.cb = __builtin_amdgcn_readfirstlane(g.cb);
        gw.ct = __builtin_amdgcn_readfirstlane(g.ct);
        asm volatile("" : "+s"(gw.n_seg), "+s"(gw.az_start), "+s"(gw.az_end), "+s"(gw.cb), "+s"(gw.ct));
        int nw = __builtin_amdgcn_readfirstlane(n);
        asm volatile("" : "+s"(nw));
        // halos, OLD values (every lane takes part in the exchange, frozen environments included)
        const float a_last = P[H - 1].x, b_first = P[0].y;
        const float give = c == 0 ? P[H - 1].y : P[0].x;
        const float got = __int_as_float(swap_with_neighbour(__float_as_int(give)));
        const float halo_l = c == 0 ? spool : got, halo_r = c == 0 ? got : 0.0f;
        WEDM_SV_PHASE(pa);
        constexpr bool kF64 = false;  // (float32 stencil only)
        const StencilF64 f64c{0.0, 0.0, 0.0};
        const float rw_h_base = 0.0f, rw_h_zone = 0.0f;
#define WEDM_REGS_WALK_TILE_FENCE 1
#include "wedm_regs_walk.inc"
#undef WEDM_REGS_WALK_TILE_FENCE
        WEDM_SV_PHASE(pb);
        tmax = fmax_gt(tmax, __int_as_float(swap_with_neighbour(__float_as_int(tmax))));
        sv_give(box, slot, el, c == 0, tid, wave, it, tmax);
        WEDM_SV_PHASE(pc);
    }
    WEDM_SV_LOOP_END();
    sv_stamps_out(svs, stamp_row);

    WEDM_REGS_STORE_WIRE()
    __syncthreads();  // (B)
}
