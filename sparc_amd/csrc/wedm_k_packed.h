// wedm_k_packed.h — wedm_step_packed<L>: the fused walk with two virtual chunks per lane advanced in float2 registers.
//
// Included by wedm_kernels.hip (one translation unit per WEDM_PART; see the bottom of that file).
// The walk itself -- the lane's tile flags, and per microsecond the halos, the tiles and the patches -- is the text of
// wedm_packed_walk.inc, shared with wedm_step_served; here are the kernel's frame (staging, lifecycle, the reduction over the
// environment's lanes, the trace point) and its own pieces of the walk: tile8_staged tiles and four scalar tail cells.
#pragma once

// ============================================ packed fused kernel, L lanes / env, 2 cells / op
// Same walk as wedm_step_fused, but every lane owns TWO virtual chunks A and B of Cv cells and
// advances them together in one float2 register pair, so each v_pk_add_f32 / v_pk_mul_f32 does
// two cells.  With only 1-2 waves per SIMD (the batch fixes the wave count) a wave is limited by
// its own in-order issue, one VALU per 4 cycles, while the SIMD pipe idles half the time: packing
// halves the instructions the wave has to issue.  Rows of A and B are interleaved in the lane's
// LDS column (row 2r = A[r], row 2r+1 = B[r]; rows 2Cv, 2Cv+1 hold the right halos), so a pair
// is one ds_read2st64_b32 / ds_write2st64_b32.  The walk table is the one built for 2L chunks.

template <bool JOULE>
__device__ __forceinline__ f2 interior2(f2 tm1, f2 tc, f2 tp1, float k, float tuf, f2 conv, float tdiel, float adv,
                                        f2 jfe, float alpha, float tref) {
    f2 a = sub_twice(tm1, tc);
    f2 d = k * (a + tp1);
    if (JOULE) {
        f2 rho_T = 1.0f + alpha * (tc - tref);
        d = d + jfe * rho_T;
    }
    d = d - conv * (tc - tdiel);
    d = d + adv * (tm1 - tc);
    return tc + d * tuf;
}

// This kernel's pieces of the walk, expanded by wedm_packed_walk.inc where it uses them (its head says what each has to do).
// Tail cells: four scalar cells, the Joule term always.
#define WEDM_PACKED_WALK_TAILS_FROM_OLD()                                                                                         \
    float tt[4] = {0.0f, 0.0f, 0.0f, 0.0f}; /* [2 q + v] */                                                                       \
    if (use_tail) {                                                                                                               \
        const float jfl = (cf.joule_on && !s.done) ? cf.jf : 0.0f;                                                                \
        _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                                           \
            if (q < tail) {                                                                                                       \
                const int r = Cv - tail + q;                                                                                      \
                _Pragma("unroll") for (int v = 0; v < 2; ++v) {                                                                   \
                    const uint32_t b = tail_bits >> (4 * (2 * q + v));                                                            \
                    /* rows 2 Cv and 2 Cv + 1 hold the halo pair: the right neighbour of a chunk's last cell */                   \
                    tt[2 * q + v] = interior_cell<true>(col[(2 * (r - 1) + v) * CS], col[(2 * r + v) * CS], col[(2 * (r + 1) + v) * CS], \
                                                        g.k, g.tuf, (b & 1u) ? ps.conv_zone : ps.conv_base, tdiel, ps.adv,        \
                                                        (b & 2u) ? jfl : 0.0f, alpha, tref);                                      \
                }                                                                                                                 \
            }                                                                                                                     \
        }                                                                                                                         \
    }
#define WEDM_PACKED_WALK_TAIL_NEW(q, v) tt[2 * (q) + (v)]
#define WEDM_PACKED_WALK_DONE s.done
#define WEDM_PACKED_WALK_REGULAR_TILE(JOULE) tile8_staged<f2, JOULE, false>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref)
// One-change tiles: all eight coefficient pairs up front.
#define WEDM_PACKED_WALK_ONECHANGE_TILE()                                                                     \
    f2 cv[8], jv[8];                                                                                          \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                           \
        cv[u] = u < split ? conv_lo : conv_hi;                                                                \
        jv[u] = u < split ? jfe_lo : jfe_hi;                                                                  \
    }                                                                                                         \
    if (joule_wave) tile8_staged<f2, true, true>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);    \
    else tile8_staged<f2, false, true>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref)

// Forms: F_TRACE, and
// F_FROZEN_OK: the form for handles with in-launch autoreset, i.e. batches in which environments terminate at
// different times and wait, frozen, for the next launch.  Without it a wave with a frozen lane walks every cell on the
// predicated path (~4 x slower: 3.65e9 instead of 1.36e10 env-steps/s on a batch that resets 17 % of its environments per
// launch); with it such a wave takes a second copy of the tile code in which the frozen lanes do not store.  A separate
// form, because the mere presence of that copy costs the other waves 2 % (6 % when folded into one copy).
// F_EXTRA: the form for tile tables that need them: one-change tiles on the stage-major code (see wedm_step_fused's
// F_N1) and a chunk's 1- or 2-cell tail computed with the patched cells (virtual chunks of 25 cells: 400 segments over 8 lanes).
template <int L, uint32_t F>
__global__ void __launch_bounds__(256, WEDM_PACKED_MIN_BLOCKS) wedm_step_packed(const KArgs k) {
    static_assert((F & ~(F_TRACE | F_FROZEN_OK | F_EXTRA)) == 0, "forms of wedm_step_packed");
    constexpr bool TRACE = (F & F_TRACE) != 0, FROZEN_OK = (F & F_FROZEN_OK) != 0, EXTRA = (F & F_EXTRA) != 0;
    constexpr bool kFrozenOk = FROZEN_OK;
    const ColdRef cold = kernarg_cold();
    Hot hv = k.hot;
    // the constants of the epilogue and of the quiet prelude: what fits in 256 VGPRs without a
    // spill (pinning all of them spills 10 VGPRs and is no faster); +11 % over none
    pin_mechanics_in_vgprs(hv);
    pin_quiet_in_vgprs(hv);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int EPB = 256 / L;
    const int tid = threadIdx.x;
    const int el = tid / L, c = tid % L;
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = e0 + el;
    const bool live = e < k.num_envs;
    const WalkTable* __restrict__ wt = k.walk;  // built for 2L virtual chunks
    const int Cv = wt->C;
    const int R = 2 * Cv;  // data rows per lane; rows R and R+1 are the halo pair
    const int n = k.hot.n_seg;
    const int64_t stride = cold->s.stride;

    // ---- stage: wire cell i -> virtual chunk vc = i / Cv, cell r = i % Cv -> lane vc/2, row 2r + vc%2
    const PackedSlot<256> wire_slot{Cv};
    copy_wire<L, true>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
    __syncthreads();

    Env s;
    Geom g;
    Persist ps{0.0f, 0.0f, 0.0f, 0};
    load_geom(k.hot, cold, live ? e : 0, g);
    WEDM_ENV_LOAD()
    float* col = lds + tid;
    Sig none;  // (no F_SIG forms: nothing reads it)
    WEDM_ENV_RESET(c == 0, none, for (int row = 0; row < R; ++row) col[row * 256] = k.hot.spool)
    WEDM_ENV_START(const bool frozen0, WEDM_REPORT_FROZEN(frozen0 && live))
    const uint32_t gid = k.hot.env_id_offset + (uint32_t)e;

    const int baseA = 2 * c * Cv, baseB = baseA + Cv;  // first wire cell of each virtual chunk
    const float spool = k.hot.spool, tref = k.hot.tref, alpha = k.hot.alpha, tdiel = k.hot.tdiel;
    const int n_tiles = wt->n_tiles;
    constexpr int CS = 256;  // column stride of the LDS image: one column per thread of the block
#define WEDM_PACKED_WALK_SETUP
#include "wedm_packed_walk.inc"
#undef WEDM_PACKED_WALK_SETUP

    WEDM_STAMP_DECL;
    const bool tracing = WEDM_TRACING(k);
    int trace_next = k.trace_next, trace_slot = k.trace_slot;
    (void)trace_next; (void)trace_slot;
    for (int it = 0; it < k.n_substeps; ++it) {
        if (__all(s.done) && !tracing) break;
        WEDM_STAMP(st0);
        Coef cf{0.0f, 0.0f, 0, -1};
        QuietTry qt;
        const bool was_quiet = quiet_prelude_t<kPackedDense>(hv, cold, g, e, gid, s, qt, cf);
        if (!was_quiet && !s.done) cf = scalar_prelude(hv, cold, g, e, gid, s, ps, c == 0, qt);
        freeze_wire(s);
        WEDM_STAMP(st1);
#ifdef WEDM_STAMPS
        if (was_quiet) { accN += st1 - st0; ++cntN; } else { accB += st1 - st0; ++cntB; }  // quiet / general prelude
#endif

        float tmax = spool;
#ifdef WEDM_ABL_NO_STENCIL
        constexpr bool kWalkTiles = false;
#define WEDM_PACKED_WALK_MARK_TILES asm volatile("" ::"v"(cf.jf), "v"(cf.q), "v"(cf.pidx), "v"(ps.conv_base), "v"(ps.conv_zone), "v"(tpl), "v"(tlast))
#else
        constexpr bool kWalkTiles = true;
#define WEDM_PACKED_WALK_MARK_TILES do { } while (0)
#endif
#define WEDM_PACKED_WALK_MARK_PATCHES WEDM_STAMP(st2)
#define WEDM_PACKED_WALK_US
#include "wedm_packed_walk.inc"
#undef WEDM_PACKED_WALK_US
#undef WEDM_PACKED_WALK_MARK_TILES
#undef WEDM_PACKED_WALK_MARK_PATCHES
#pragma unroll
        for (int m = 1; m < L; m <<= 1) tmax = fmax_gt(tmax, __shfl_xor(tmax, m));
        WEDM_STAMP(st3);
        env_end_us<F>(hv, cold, e, s, tmax, 0, c == 0);
        WEDM_TRACE_POINT(k, it, e, s, c == 0,
                         for (int r = 0; r < Cv; ++r) {
                             if (baseA + r < n) tT[(int64_t)(baseA + r) * tcnt] = col[(2 * r) * 256];
                             if (baseB + r < n) tT[(int64_t)(baseB + r) * tcnt] = col[(2 * r + 1) * 256];
                         });
        WEDM_STAMP(st4);
        WEDM_STAMP_ACC();
    }
    WEDM_STAMP_OUT();

    __syncthreads();
    copy_wire<L, false>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
    env_close(k, cold, e, s, frozen0, live && c == 0);
}
#undef WEDM_PACKED_WALK_TAILS_FROM_OLD
#undef WEDM_PACKED_WALK_TAIL_NEW
#undef WEDM_PACKED_WALK_DONE
#undef WEDM_PACKED_WALK_REGULAR_TILE
#undef WEDM_PACKED_WALK_ONECHANGE_TILE


