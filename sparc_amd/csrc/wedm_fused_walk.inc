// wedm_fused_walk.inc — the one-chunk LDS tile walk: one chunk of C cells per lane in the lane's LDS column (row j = cell j, row C
// the right halo), tiles of 8 cells advanced in float registers.  One microsecond of it, from the halos to the trace point.
// Textually included where it runs: in the microsecond loop of wedm_step_fused (wedm_k_fused.h) and in `rest` of
// wedm_step_stream (wedm_k_stream.h), behind freeze_wire(s).
// Names it expects in scope: L, F, FROZEN_OK, kWalkTiles (compile time: lanes per environment; the kernel's forms;
// the tile code has a copy in which frozen lanes do not store -- false sends a wave with a frozen lane down the predicated
// path; false in an ablation build only: no tiles); k, hv, cold, e, it; c, col (= lds + tid), C, cbase (= c C), n, n_tiles, wt; s, g, cf, ps; spool, tref, alpha,
// tdiel; the lane's tile flags zone_lo, joule_lo, zone_hi, joule_hi and split_pack; the wave-uniform tile masks kind_n,
// kind_s, kind_ne, kind_nj; owns_last, t_last; and what the two kernels really do differently, as macros that expand here (a
// lambda in their place changes the order in which the compiler inlines and, with it, the registers and the schedule of the
// tiles); each includer defines them before its kernel and undefines them after it:
//   WEDM_FUSED_WALK_CELLWISE                 an expression: this wave walks every tile cell by cell in this microsecond
//                                            (all_slow; in wedm_step_stream's float64 typing always)
//   WEDM_FUSED_WALK_FULL_CELL(i, tm, tc, tp) wire cell i by the full predicated formula, in the stencil's typing
//   WEDM_FUSED_WALK_INTERIOR_CELL(tp, zone, contacts, conv, jfe)
//                                            an interior cell from tm1, tc and tp in the stencil's typing: float32 with the
//                                            coefficients conv / jfe, float64 by the flags zone / contacts
//   WEDM_FUSED_WALK_TAILS_FROM_OLD()         declares n_walk, the tiles to walk; wedm_step_fused: also use_tail and the new
//                                            values of a chunk's 1 or 2 tail cells from OLD ones, which then are no tile
//   WEDM_FUSED_WALK_IS_ONECHANGE(t)          an expression: tile t takes the one-change code (wedm_step_fused's F_N1)
//   WEDM_FUSED_WALK_TILE_B_OK                compile time: the instantiation has boundary-tile code
//   WEDM_FUSED_WALK_OUT_REGULAR()            behind a regular tile's column stores, WEDM_FUSED_WALK_OUT_B_DECL / _OUT_B_CELL(u, v)
//   / _OUT_B()                               before / in / behind a boundary tile's cells: wedm_step_stream sends the tiles of a
//                                            launch's last microsecond straight to global memory
//   WEDM_FUSED_WALK_BEFORE_PATCHES()         behind the walk: wedm_step_fused writes its tail cells, wedm_step_stream notes the
//                                            patched cells for its write-back; either kernel's stamp
//   WEDM_FUSED_WALK_MARK_TILES / _TILE_BEGIN / _TILE_END / _MARK_REDUCED
//                                            the includer's instrumentation before the tiles, around one tile, behind the
//                                            reduction over the environment's lanes
        // ---- halos: OLD neighbour values, read before any lane of this wave stores.  The right
        // halo goes into the chunk's extra LDS row C, so cell C-1 is walked like any other.
        const float halo_l = (c > 0) ? col[(C - 1) * 256 - 1] : spool;
        const float halo_r = (c < L - 1) ? col[1] : 0.0f;
        col[C * 256] = halo_r;

        // a wave with a negative plasma heat (or, without FROZEN_OK, with a frozen environment) walks every cell on the
        // predicated path; results are identical, only slower
        const bool frozen_wave = FROZEN_OK && __any(s.done);
        const bool all_slow = __any(cf.q < 0.0f) || (!FROZEN_OK && __any(s.done));
        const uint32_t slow_now = WEDM_FUSED_WALK_CELLWISE ? 0xffffffffu : kind_s;
        // regular tiles of THIS microsecond: a contact-flag change inside a tile only matters while current flows
        const uint32_t n_now = (kind_n | kind_ne | (__any(cf.joule_on && !s.done && cf.jf != 0.0f) ? 0u : kind_nj)) & ~(WEDM_FUSED_WALK_CELLWISE ? 0xffffffffu : 0u);

        // ---- patched cells: the plasma cell and the wire's last cell are computed with the
        // full predicated formula from OLD values now and written after the walk
        const bool owns_pl = !s.done && cf.pidx >= 1 && cf.pidx >= cbase && cf.pidx < cbase + C;
        float tpl = 0.0f, tlast = 0.0f;
        if (__any(owns_pl)) {
            if (owns_pl) {
                const int jp = cf.pidx - cbase;
                float tm = jp > 0 ? col[(jp - 1) * 256] : halo_l;
                if (cf.pidx == 1) tm = spool;
                const float tcc = col[jp * 256];
                const float tp = jp < C - 1 ? col[(jp + 1) * 256] : halo_r;
                tpl = WEDM_FUSED_WALK_FULL_CELL(cf.pidx, tm, tcc, tp);
            }
        }
        if (owns_last && !s.done) {
            const int jl = n - 1 - cbase;
            float tm = jl > 0 ? col[(jl - 1) * 256] : halo_l;
            if (n - 1 == 1) tm = spool;
            tlast = WEDM_FUSED_WALK_FULL_CELL(n - 1, tm, col[jl * 256], 0.0f);
        }
        WEDM_FUSED_WALK_TAILS_FROM_OLD();

        float tmax = spool;
        float tm1 = halo_l;
        float tc = col[0];
        WEDM_FUSED_WALK_MARK_TILES;
        if (kWalkTiles) {
            const float jf_lane = (cf.joule_on && !s.done) ? cf.jf : 0.0f;
            const bool joule_wave = __any(jf_lane != 0.0f);

            // tile t covers cells j = 8t..8t+7; cur[u] = OLD T[j+1+u], loaded at the head of the tile
            // CLAMP = false: all eight rows exist (j + 8 <= C), one base address + immediate offsets
            auto load8 = [&](auto clamp, float (&dst)[8], int j) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int row = j + 1 + u;
                    if (decltype(clamp)::value) row = row < C ? row : C;  // rows past the chunk are never used; row C is the halo
                    dst[u] = col[row * 256];
                }
            };
            auto tile = [&](auto frozen, int t, float (&cur)[8]) {
                constexpr bool FROZEN = decltype(frozen)::value;  // the copy for a wave with frozen lanes: they do not store
                const int j = 8 * t;
                load8(std::true_type{}, cur, j);  // (an unclamped variant for full tiles pays in the packed kernel only)
                const float conv_lo = ((zone_lo >> t) & 1u) ? ps.conv_zone : ps.conv_base;
                const float jfe_lo = ((joule_lo >> t) & 1u) ? jf_lane : 0.0f;
                WEDM_FUSED_WALK_TILE_BEGIN;
                if ((n_now >> t) & 1u) {
                    float old[10], tn[8], cv[8], jv[8];
                    old[0] = tm1; old[1] = tc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) old[u + 2] = cur[u];
                    cv[0] = conv_lo; jv[0] = jfe_lo;
                    if (joule_wave && __any(jfe_lo != 0.0f))
                        tile8_staged<float, true, false>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
                    else
                        tile8_staged<float, false, false>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
                    // the wire's end cells, where a regular tile holds one (kind_ne / kind_nj): cell 0 stays at the spool
                    // temperature; the last cell is kept out of the maximum here and patched after the walk
                    tn[0] = (c == 0 && t == 0) ? spool : tn[0];
                    const float last_v = (owns_last && t == t_last) ? spool : tn[7];
                    if (!FROZEN || !s.done) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) col[(j + u) * 256] = tn[u];
                    }
                    WEDM_FUSED_WALK_OUT_REGULAR();
                    float m0 = fmax_gt(tn[0], tn[1]), m1 = fmax_gt(tn[2], tn[3]);
                    m0 = fmax_gt(m0, fmax_gt(tn[4], tn[5]));
                    m1 = fmax_gt(m1, fmax_gt(tn[6], last_v));
                    tmax = fmax_gt(tmax, fmax_gt(m0, m1));
                    tm1 = cur[6];
                    tc = cur[7];
                } else if (WEDM_FUSED_WALK_IS_ONECHANGE(t)) {
                    // one flag change at `split`, nothing else irregular (end cells apart): stage-major with per-cell
                    // coefficients, stores and maximum as in a regular tile
                    const int split = (int)((split_pack[t >> 3] >> ((t & 7) * 4)) & 15u);
                    const float conv_hi = ((zone_hi >> t) & 1u) ? ps.conv_zone : ps.conv_base;
                    const float jfe_hi = ((joule_hi >> t) & 1u) ? jf_lane : 0.0f;
                    float old[10], tn[8], cv[8], jv[8];
                    old[0] = tm1; old[1] = tc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        old[u + 2] = cur[u];
                        cv[u] = u < split ? conv_lo : conv_hi;
                        jv[u] = u < split ? jfe_lo : jfe_hi;
                    }
                    if (joule_wave) tile8_staged<float, true, true>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
                    else tile8_staged<float, false, true>(old, tn, g.k, g.tuf, cv, tdiel, ps.adv, jv, alpha, tref);
                    tn[0] = (c == 0 && t == 0) ? spool : tn[0];
                    const float last_v = (owns_last && t == t_last) ? spool : tn[7];
                    if (!FROZEN || !s.done) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) col[(j + u) * 256] = tn[u];
                    }
                    float m0 = fmax_gt(tn[0], tn[1]), m1 = fmax_gt(tn[2], tn[3]);
                    m0 = fmax_gt(m0, fmax_gt(tn[4], tn[5]));
                    m1 = fmax_gt(m1, fmax_gt(tn[6], last_v));
                    tmax = fmax_gt(tmax, fmax_gt(m0, m1));
                    tm1 = cur[6];
                    tc = cur[7];
                } else if (WEDM_FUSED_WALK_TILE_B_OK && !((slow_now >> t) & 1u)) {
                    // TILE_B: interior formula everywhere, one flag change at `split`, boundary and
                    // out-of-wire cells excluded from the max (they are patched / never read)
                    const int split = (int)((split_pack[t >> 3] >> ((t & 7) * 4)) & 15u);
                    const int cnt = (C - j) < 8 ? (C - j) : 8;
                    const float conv_hi = ((zone_hi >> t) & 1u) ? ps.conv_zone : ps.conv_base;
                    const float jfe_hi = ((joule_hi >> t) & 1u) ? jf_lane : 0.0f;
                    const uint32_t im1 = (uint32_t)(cbase + j - 1);  // (i - 1) of the tile's first cell
                    const uint32_t span = (uint32_t)(n - 3);         // interior <=> (i - 1) <= n - 3 (unsigned)
                    WEDM_FUSED_WALK_OUT_B_DECL;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (u < cnt) {
                            const float conv = u < split ? conv_lo : conv_hi;
                            const float jfe = u < split ? jfe_lo : jfe_hi;
                            float tn = WEDM_FUSED_WALK_INTERIOR_CELL(cur[u], ((u < split ? zone_lo : zone_hi) >> t) & 1u,
                                                                     ((u < split ? joule_lo : joule_hi) >> t) & 1u, conv, jfe);
                            if (!FROZEN || !s.done) col[(j + u) * 256] = tn;
                            WEDM_FUSED_WALK_OUT_B_CELL(u, tn);
                            const bool inter = (n >= 3) && (im1 + (uint32_t)u <= span);
                            tmax = inter ? fmax_gt(tmax, tn) : tmax;
                            tm1 = tc;
                            tc = cur[u];
                        }
                    }
                    WEDM_FUSED_WALK_OUT_B();
                } else {
#pragma unroll 1
                    for (int u = 0; u < 8; ++u) {
                        const int jj = j + u;
                        const uint32_t zj = wt->zj[jj], iv = wt->iv[jj];
                        const bool zbit = (zj >> c) & 1u, jbit = (zj >> (16 + c)) & 1u;
                        const bool inter = ((iv >> c) & 1u) && !all_slow;
                        const bool valid = ((iv >> (16 + c)) & 1u) && !s.done;
                        const float conv = zbit ? ps.conv_zone : ps.conv_base;
                        const float jfe = jbit ? jf_lane : 0.0f;
                        const float tp1 = cur[0];
                        float tn = WEDM_FUSED_WALK_INTERIOR_CELL(tp1, zbit, jbit, conv, jfe);
                        if (!inter && valid) {  // boundary cells and irregular waves: predicated formula
                            const int i = cbase + jj;
                            tn = (i >= 1) ? WEDM_FUSED_WALK_FULL_CELL(i, (i == 1) ? spool : tm1, tc, tp1) : spool;
                        }
                        if (valid) {
                            col[jj * 256] = tn;
                            tmax = fmax_gt(tmax, tn);
                        }
                        tm1 = tc;
                        tc = tp1;
                        // rotate the tile's window (this fallback is rare; keep its code small)
                        float* w = const_cast<float*>(&cur[0]);
                        float first = w[0];
#pragma unroll
                        for (int q = 0; q < 7; ++q) w[q] = w[q + 1];
                        w[7] = first;
                    }
                }
                WEDM_FUSED_WALK_TILE_END;
            };
            float bufA[8];
            if (!FROZEN_OK || !frozen_wave) {
                for (int t = 0; t < n_walk; ++t) tile(std::false_type{}, t, bufA);
            } else {
                for (int t = 0; t < n_walk; ++t) tile(std::true_type{}, t, bufA);
            }
        }
        // ---- patches (after every store of the walk): boundary condition, last cell, plasma cell
        WEDM_FUSED_WALK_BEFORE_PATCHES();
        if (c == 0 && !s.done) col[0] = spool;
        if (owns_last && !s.done) {
            col[(n - 1 - cbase) * 256] = tlast;
            tmax = fmax_gt(tmax, tlast);
        }
        if (owns_pl) {
            col[(cf.pidx - cbase) * 256] = tpl;
            tmax = fmax_gt(tmax, tpl);
        }
#pragma unroll
        for (int m = 1; m < L; m <<= 1) tmax = fmax_gt(tmax, __shfl_xor(tmax, m));
        WEDM_FUSED_WALK_MARK_REDUCED;
        env_end_us<F>(hv, cold, e, s, tmax, 0, c == 0);
        WEDM_TRACE_POINT(k, it, e, s, c == 0,
                         for (int j = 0; j < C && cbase + j < n; ++j) tT[(int64_t)(cbase + j) * tcnt] = col[j * 256]);
