// wedm_k_fused.h — wedm_step_fused<L>: uniform geometry, L lanes per environment, wire chunks in LDS, wave-uniform tile table.
//
// Included by wedm_kernels.hip (one translation unit per WEDM_PART; see the bottom of that file).
// The walk itself -- per microsecond the halos, the patched cells, the tiles, the patches, the reduction over the environment's
// lanes and the trace point -- is the text of wedm_fused_walk.inc, shared with wedm_step_stream; here are the kernel's frame
// (staging, lifecycle, the lane's tile flags gathered from the walk table) and its own pieces of the walk: the stencil's two
// typings, the tail cells, the one-change tiles' test and the instrumentation.
#pragma once

// ===================================================== fused kernel, L lanes / env

// One interior cell (1 <= i <= n-2), float32 op for op as wire.py:91-120 evaluates it.
// The advection term is always applied: adv == 0 in lanes where the reference skips it
// (d + 0*(..) == d), which keeps the loop free of a per-lane branch.
template <bool JOULE>
__device__ __forceinline__ float interior_cell(float tm1, float tc, float tp1, float k, float tuf, float conv,
                                               float tdiel, float adv, float jfe, float alpha, float tref) {
    float a = sub_twice(tm1, tc);  // T[i-1] - 2*T[i], one rounding
    float d = k * (a + tp1);
    if (JOULE) {
        float rho_T = 1.0f + alpha * (tc - tref);
        d = d + jfe * rho_T;  // jfe == 0 in lanes outside the contacts: d + 0 == d
    }
    d = d - conv * (tc - tdiel);
    d = d + adv * (tm1 - tc);
    return tc + d * tuf;
}

// This kernel's pieces of the walk, expanded by wedm_fused_walk.inc where it uses them (its head says what each has to do).
#define WEDM_FUSED_WALK_CELLWISE all_slow
// one cell by the full predicated formula / one interior cell, in the stencil's typing: the kernel's lambdas cell_full / cell_interior
#define WEDM_FUSED_WALK_FULL_CELL(i, tm, tc, tp) cell_full(i, tm, tc, tp, cf, ps)
#define WEDM_FUSED_WALK_INTERIOR_CELL(tp, zone, contacts, conv, jfe)      \
    (F64 ? cell_interior(tm1, tc, tp, zone, contacts, cf, ps, jf_lane) \
         : interior_cell<true>(tm1, tc, tp, g.k, g.tuf, conv, tdiel, ps.adv, jfe, alpha, tref))
// Tail cells (see `tail` in the kernel): new values from OLD ones, before the walk; not on the predicated path, whose last
// tile covers them.  Written behind the walk; bits per tail cell: valid (the cell exists) and interior (it counts for the
// maximum and is not the wire's last cell, which the patch after it writes).
#define WEDM_FUSED_WALK_TAILS_FROM_OLD()                                                                                          \
    const bool use_tail = tail != 0 && !all_slow;                                                                                 \
    float tt0 = 0.0f, tt1 = 0.0f;                                                                                                 \
    if (use_tail) {                                                                                                               \
        const float jfl = (cf.joule_on && !s.done) ? cf.jf : 0.0f;                                                                \
        const int j0 = C - tail;                                                                                                  \
        const float a0 = col[(j0 - 1) * 256], b0 = col[j0 * 256], c0 = col[(j0 + 1) * 256]; /* row C holds the right halo */      \
        tt0 = interior_cell<true>(a0, b0, c0, g.k, g.tuf, (tail_bits & 1u) ? ps.conv_zone : ps.conv_base, tdiel, ps.adv,          \
                                  (tail_bits & 2u) ? jfl : 0.0f, alpha, tref);                                                    \
        if (tail == 2) {                                                                                                          \
            const float c1 = col[(j0 + 2) * 256];                                                                                 \
            tt1 = interior_cell<true>(b0, c0, c1, g.k, g.tuf, (tail_bits & 16u) ? ps.conv_zone : ps.conv_base, tdiel, ps.adv,     \
                                      (tail_bits & 32u) ? jfl : 0.0f, alpha, tref);                                               \
        }                                                                                                                         \
    }                                                                                                                             \
    const int n_walk = use_tail ? n_tiles - 1 : n_tiles
#define WEDM_FUSED_WALK_BEFORE_PATCHES()                                                                    \
    WEDM_STAMP(st2);                                                                                        \
    if (use_tail && !s.done) {                                                                              \
        if (tail_bits & 4u) { col[(C - tail) * 256] = tt0; tmax = fmax_gt(tmax, tt0); }                     \
        if (tail == 2 && (tail_bits & 64u)) { col[(C - 1) * 256] = tt1; tmax = fmax_gt(tmax, tt1); }        \
    }
#define WEDM_FUSED_WALK_IS_ONECHANGE(t) (N1 && (((kind_n1 & ~slow_now) >> (t)) & 1u))
#define WEDM_FUSED_WALK_TILE_B_OK true
// (nothing leaves the LDS column during the walk: copy_wire writes the block back after the last microsecond)
#define WEDM_FUSED_WALK_OUT_REGULAR() do { } while (0)
#define WEDM_FUSED_WALK_OUT_B_DECL do { } while (0)
#define WEDM_FUSED_WALK_OUT_B_CELL(u, v) do { } while (0)
#define WEDM_FUSED_WALK_OUT_B() do { } while (0)
#ifdef WEDM_ABL_NO_STENCIL
#define WEDM_FUSED_WALK_MARK_TILES asm volatile("" ::"v"(cf.jf), "v"(cf.q), "v"(cf.pidx), "v"(ps.conv_base), "v"(ps.conv_zone), "v"(tpl), "v"(tlast))
#else
#define WEDM_FUSED_WALK_MARK_TILES do { } while (0)
#endif
#ifdef WEDM_STAMPS_TILES
// (diagnostic buckets: regular tiles, boundary tiles, and -- in the third -- one-change tiles of the N1 instantiation together
// with the predicated fallback)
#define WEDM_FUSED_WALK_TILE_BEGIN \
    WEDM_STAMP(tk0);               \
    const int tkind = ((n_now >> t) & 1u) ? 0 : (WEDM_FUSED_WALK_IS_ONECHANGE(t) ? 2 : (!((slow_now >> t) & 1u) ? 1 : 2))
#define WEDM_FUSED_WALK_TILE_END \
    WEDM_STAMP(tk1);             \
    if (tkind == 0) { accN += tk1 - tk0; ++cntN; } else if (tkind == 1) { accB += tk1 - tk0; ++cntB; } else { accS += tk1 - tk0; ++cntS; }
#else
#define WEDM_FUSED_WALK_TILE_BEGIN do { } while (0)
#define WEDM_FUSED_WALK_TILE_END do { } while (0)
#endif
#define WEDM_FUSED_WALK_MARK_REDUCED WEDM_STAMP(st3)

// Forms: F_TRACE; F_FROZEN_OK: see wedm_step_packed.  F_N1: the form for tile tables with a one-change tile that is a
// boundary tile in every microsecond (4 096 x 400 over 16 lanes: the end of the workpiece zone falls inside tile 2 of 4):
// +4.7 % there; the extra code costs tables without such a tile 1-1.5 %, so they run the form without it.
// F_F64: wedm_params.stencil_mode 1 -- the stencil as Numba types wire.py:58-123 (float64 expressions rounded at each float32
// store), on the tile walk: every tile takes the boundary-tile code (per-cell coefficients, interior formula, end cells
// patched), which is exact for regular tiles too; no stage-major / packed form.  Only with F_FROZEN_OK, without F_N1.
template <int L, uint32_t F>
__global__ void __launch_bounds__(256, WEDM_FUSED_MIN_BLOCKS) wedm_step_fused(const KArgs k) {
    static_assert((F & ~(F_TRACE | F_FROZEN_OK | F_N1 | F_F64)) == 0, "forms of wedm_step_fused");
    constexpr bool TRACE = (F & F_TRACE) != 0, FROZEN_OK = (F & F_FROZEN_OK) != 0, N1 = (F & F_N1) != 0, F64 = (F & F_F64) != 0;
    constexpr bool kFrozenOk = FROZEN_OK;
#ifdef WEDM_ABL_NO_STENCIL
    constexpr bool kWalkTiles = false;
#else
    constexpr bool kWalkTiles = true;
#endif
    const ColdRef cold = kernarg_cold();
    Hot hv = k.hot;
    pin_hot_in_vgprs(hv);  // 178 -> 225 VGPRs, SGPR spill traffic in the loop 111 -> 37 instructions: +8 %
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int EPB = 256 / L;  // environments per block
    const int tid = threadIdx.x;
    const int el = tid / L, c = tid % L;
    const int64_t e0 = (int64_t)blockIdx.x * EPB;
    const int64_t e = e0 + el;
    const bool live = e < k.num_envs;
    const WalkTable* __restrict__ wt = k.walk;
    const int C = wt->C;
    const int n = k.hot.n_seg;
    const int64_t stride = cold->s.stride;

    // ---- stage the block's EPB wire columns: 16-byte words of the quad-interleaved block -> LDS
    // wire cell i -> chunk i / C, cell i % C -> LDS [cell][256 lanes], lane = environment slot * L + chunk
    const ChunkSlot wire_slot{C};
    copy_wire<L, true>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
    __syncthreads();

    Env s;
    Geom g;
    Persist ps{0.0f, 0.0f, 0.0f, 0};
    load_geom(k.hot, cold, live ? e : 0, g);
    WEDM_ENV_LOAD()
    float* col = lds + tid;
    Sig none;  // (no F_SIG forms: nothing reads it)
    WEDM_ENV_RESET(c == 0, none, for (int j = 0; j < C; ++j) col[j * 256] = k.hot.spool)
    WEDM_ENV_START(const bool frozen0, WEDM_REPORT_FROZEN(frozen0 && live))
    const uint32_t gid = k.hot.env_id_offset + (uint32_t)e;

    const int cbase = c * C;
    const float spool = k.hot.spool, tref = k.hot.tref, alpha = k.hot.alpha, tdiel = k.hot.tdiel;
    const StencilF64 f64c = stencil_f64_consts<F>(cold, e);
    // one cell by the full predicated formula / one interior cell with coefficients handed in, in the stencil's typing
    // (zone / contacts: whether the cell lies in the workpiece zone / between the contacts)
    auto cell_full = [&](int i, float tm, float tcc, float tp, const Coef& cf, const Persist& ps) -> float {
        if (F64) return stencil_cell_f64(i, n, tm, tcc, tp, g, cf, ps, f64c, s.h_base, s.h_zone);
        return stencil_cell(i, n, tm, tcc, tp, g, cf, ps, tref, alpha, tdiel);
    };
    auto cell_interior = [&](float tm, float tcc, float tp, bool zone, bool contacts, const Coef& cf, const Persist& ps,
                             float jf_lane) -> float {
        if (F64)
            return interior_cell_f64(tm, tcc, tp, g.k64, g.tuf64, (double)(zone ? s.h_zone : s.h_base) * g.a64, f64c.tdiel, ps.adv64,
                                     (contacts && cf.joule_on) ? cf.jf64 : 0.0, f64c.alpha, f64c.tref);
        return interior_cell<true>(tm, tcc, tp, g.k, g.tuf, zone ? ps.conv_zone : ps.conv_base, tdiel, ps.adv,
                                   contacts ? jf_lane : 0.0f, alpha, tref);
    };
    const int n_tiles = wt->n_tiles;
    // per-lane tile membership, gathered ONCE so that walking a tile reads nothing but LDS
    // (scalar loads share lgkmcnt with LDS and would drain the prefetch every tile):
    // bit t of zone_lo/joule_lo = flags of the tile's first cell, *_hi = flags of its last cell
    uint32_t zone_lo = 0u, joule_lo = 0u, zone_hi = 0u, joule_hi = 0u, kind_n = 0u, kind_s = 0u;
    uint32_t split_pack[3] = {0u, 0u, 0u};  // 4 bits per tile (WEDM_MAX_TILES <= 24)
    for (int t = 0; t < n_tiles; ++t) {
        const uint32_t lo = wt->zj[8 * t], hi = wt->zj[8 * t + 7], kd = wt->kind[t];
        split_pack[t >> 3] |= (wt->split[t] & 15u) << ((t & 7) * 4);
        zone_lo |= ((lo >> c) & 1u) << t;
        joule_lo |= ((lo >> (16 + c)) & 1u) << t;
        zone_hi |= ((hi >> c) & 1u) << t;
        joule_hi |= ((hi >> (16 + c)) & 1u) << t;
        kind_n |= (kd == TILE_N ? 1u : 0u) << t;
        kind_s |= (kd == TILE_S ? 1u : 0u) << t;
    }
    kind_n = F64 ? 0u : __builtin_amdgcn_readfirstlane(kind_n);  // (F64: every tile on the boundary-tile code)
    kind_s = __builtin_amdgcn_readfirstlane(kind_s);
    // tiles that take the regular code although they hold a wire end cell / a contact-flag change (see WalkTable)
    const uint32_t kind_ne = F64 ? 0u : __builtin_amdgcn_readfirstlane(wt->kind_ne_mask), kind_nj = F64 ? 0u : __builtin_amdgcn_readfirstlane(wt->kind_nj_mask);
    const uint32_t kind_n1 = (N1 && !F64) ? (__builtin_amdgcn_readfirstlane(wt->kind_n1_mask) & 0x7fffffffu) : 0u;
#pragma unroll
    for (int q = 0; q < 3; ++q) split_pack[q] = __builtin_amdgcn_readfirstlane(split_pack[q]);
    if (c == 0) col[0] = spool;  // wire cell 0 is held at the spool temperature (wire.py:83)
    // the lane that owns the wire's last cell (Neumann boundary, wire.py:95)
    const bool owns_last = (n >= 2) && (n - 1 >= cbase) && (n - 1 < cbase + C);
    const int t_last = (n - 1 - cbase) >> 3;  // the tile of that cell in the owning lane (its last position, where the tile is regular)
    // A chunk whose length is 1 or 2 cells over a multiple of 8 (400 segments: 25 cells over 16 lanes, 50 over 8) would
    // spend a whole tile on that tail, and a tile costs its dependent chain whatever its width (stamped: 811-843 cycles
    // for the 1- / 2-cell tile against 799-809 for a full regular one).  The tail cells are instead computed like the
    // patched cells: by the interior formula from OLD values before the walk (their chains overlap those of the plasma /
    // last cell), written after it; the walk covers the full tiles only.  Bits per tail cell q: zone, contacts,
    // interior, valid (this lane's chunk).
    const int tail = (!F64 && C > 8 && (C & 7) >= 1 && (C & 7) <= 2) ? (C & 7) : 0;
    uint32_t tail_bits = 0u;
    for (int q = 0; q < tail; ++q) {
        const uint32_t zj = wt->zj[C - tail + q], iv = wt->iv[C - tail + q];
        tail_bits |= (((zj >> c) & 1u) | (((zj >> (16 + c)) & 1u) << 1) | (((iv >> c) & 1u) << 2) | (((iv >> (16 + c)) & 1u) << 3)) << (4 * q);
    }

    WEDM_STAMP_DECL;
    const bool tracing = WEDM_TRACING(k);
    int trace_next = k.trace_next, trace_slot = k.trace_slot;
    (void)trace_next; (void)trace_slot;
    for (int it = 0; it < k.n_substeps; ++it) {
        if (__all(s.done) && !tracing) break;
        WEDM_STAMP(st0);
        Coef cf{0.0f, 0.0f, 0, -1};
        QuietTry qt;
        if (!quiet_prelude_t<kFusedDense>(hv, cold, g, e, gid, s, qt, cf) && !s.done) cf = scalar_prelude(hv, cold, g, e, gid, s, ps, c == 0, qt);
        WEDM_STAMP(st1);
        freeze_wire(s);

#include "wedm_fused_walk.inc"
        WEDM_STAMP(st4);
        WEDM_STAMP_ACC();
    }
    WEDM_STAMP_OUT();

    __syncthreads();
    copy_wire<L, false>(cold->s.T, stride, e0, k.num_envs, n, tid, lds, wire_slot);
    env_close(k, cold, e, s, frozen0, live && c == 0);
}
#undef WEDM_FUSED_WALK_CELLWISE
#undef WEDM_FUSED_WALK_FULL_CELL
#undef WEDM_FUSED_WALK_INTERIOR_CELL
#undef WEDM_FUSED_WALK_TAILS_FROM_OLD
#undef WEDM_FUSED_WALK_BEFORE_PATCHES
#undef WEDM_FUSED_WALK_IS_ONECHANGE
#undef WEDM_FUSED_WALK_TILE_B_OK
#undef WEDM_FUSED_WALK_OUT_REGULAR
#undef WEDM_FUSED_WALK_OUT_B_DECL
#undef WEDM_FUSED_WALK_OUT_B_CELL
#undef WEDM_FUSED_WALK_OUT_B
#undef WEDM_FUSED_WALK_MARK_TILES
#undef WEDM_FUSED_WALK_TILE_BEGIN
#undef WEDM_FUSED_WALK_TILE_END
#undef WEDM_FUSED_WALK_MARK_REDUCED
