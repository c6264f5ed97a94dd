// wedm_packed_walk.inc — the packed LDS walk: two virtual chunks A and B of Cv cells per lane, rows interleaved in the lane's LDS
// column (row 2 r = A[r], row 2 r + 1 = B[r], rows 2 Cv and 2 Cv + 1 the right halos), tiles of 8 pairs advanced in float2
// registers.  Textually included where it runs: in wedm_step_packed (wedm_k_packed.h) and in the walkers of wedm_step_served
// (wedm_served.h).  Two sections; the includer defines one of these before each #include and undefines it after:
//   WEDM_PACKED_WALK_SETUP  once per launch: the lane's tile flags gathered from the walk table, the owner of the wire's last
//                           cell, the tail cells' flags, wire cell 0
//   WEDM_PACKED_WALK_US     one microsecond: halos, patched cells and tails from OLD values, the tiles, the patches
// Names it expects in scope, both sections: L, EXTRA, CS (compile time: lanes per environment, the form with one-change tiles
// and tails, the column stride of the LDS image: 256 / the walker threads); c, col (= lds + tid), Cv, R (= 2 Cv), n, n_tiles,
// wt (the table built for 2 L chunks); spool; baseA, baseB (= 2 c Cv, baseA + Cv: the first wire cell of each virtual chunk;
// declared by the includer, because their place among its other loads decides registers in wedm_step_packed<2>'s trace form).
// The microsecond also: FROZEN_OK (compile time: the tile code has a copy in which frozen lanes do not store; false sends a
// wave with a frozen lane down the predicated path) and kWalkTiles (compile time, false in an ablation build only: no tiles);
// g, cf, ps; tref, alpha, tdiel; the running maximum `tmax`; WEDM_PACKED_WALK_DONE (an expression: this lane's environment is
// frozen or past the batch's end; s.done / the mailbox's flag, read where it is used so that neither kernel's registers move); and what each kernel tuned for itself, as macros that expand here (a lambda in their place changes the order in
// which the compiler inlines and, with it, the registers and the schedule of the tiles):
//   WEDM_PACKED_WALK_TAILS_FROM_OLD()     declares the includer's registers for the 1 or 2 tail pairs and, `if (use_tail)`, fills
//                                         them with the new values from OLD ones; WEDM_PACKED_WALK_TAIL_NEW(q, v) reads the new
//                                         value of tail cell q of chunk v
//   WEDM_PACKED_WALK_REGULAR_TILE(JOULE)  tn[] from old[] for a tile with one coefficient pair (cv[0], jv[0])
//   WEDM_PACKED_WALK_ONECHANGE_TILE()     tn[] from old[] for a tile whose coefficients change from conv_lo / jfe_lo to conv_hi /
//                                         jfe_hi at pair `split`; joule_wave: some lane of the wave carries current
//   WEDM_PACKED_WALK_MARK_TILES / _PATCHES   the includer's instrumentation before the tiles / before the patches
#if defined(WEDM_PACKED_WALK_SETUP)
    // per-lane tile flags for both virtual chunks, gathered once (see wedm_step_fused)
    uint32_t zlA = 0u, zlB = 0u, jlA = 0u, jlB = 0u, zhA = 0u, zhB = 0u, jhA = 0u, jhB = 0u, kind_n = 0u, kind_s = 0u;
    uint32_t split_pack[3] = {0u, 0u, 0u};
    for (int t = 0; t < n_tiles; ++t) {
        const uint32_t lo = wt->zj[8 * t], hi = wt->zj[8 * t + 7], kd = wt->kind[t];
        split_pack[t >> 3] |= (wt->split[t] & 15u) << ((t & 7) * 4);
        zlA |= ((lo >> (2 * c)) & 1u) << t;      zlB |= ((lo >> (2 * c + 1)) & 1u) << t;
        jlA |= ((lo >> (16 + 2 * c)) & 1u) << t; jlB |= ((lo >> (17 + 2 * c)) & 1u) << t;
        zhA |= ((hi >> (2 * c)) & 1u) << t;      zhB |= ((hi >> (2 * c + 1)) & 1u) << t;
        jhA |= ((hi >> (16 + 2 * c)) & 1u) << t; jhB |= ((hi >> (17 + 2 * c)) & 1u) << t;
        kind_n |= (kd == TILE_N ? 1u : 0u) << t;
        kind_s |= (kd == TILE_S ? 1u : 0u) << t;
    }
    kind_n = __builtin_amdgcn_readfirstlane(kind_n);
    kind_s = __builtin_amdgcn_readfirstlane(kind_s);
    // tiles that take the regular code although they hold a wire end cell / a contact-flag change (see WalkTable)
    const uint32_t kind_ne = __builtin_amdgcn_readfirstlane(wt->kind_ne_mask), kind_nj = __builtin_amdgcn_readfirstlane(wt->kind_nj_mask);
    const uint32_t kind_n1 = EXTRA ? (__builtin_amdgcn_readfirstlane(wt->kind_n1_mask) & 0x7fffffffu) : 0u;
#pragma unroll
    for (int q = 0; q < 3; ++q) split_pack[q] = __builtin_amdgcn_readfirstlane(split_pack[q]);
    if (c == 0) col[0] = spool;  // wire cell 0 (row 0 of lane 0's chunk A) is held at the spool temperature

    // which of this lane's virtual chunks holds wire cell i (0: none, 1: A, 2: B)
    auto owner = [&](int i) -> int {
        if (i >= baseA && i < baseA + Cv) return 1;
        if (i >= baseB && i < baseB + Cv) return 2;
        return 0;
    };
    const int own_last = (n >= 2) ? owner(n - 1) : 0;
    // the tile of that cell: a regular tile holds it only as the last cell of chunk B (chunk A's would be followed by
    // cells past the wire's end in the same tile), and not necessarily in the chunk's LAST tile (a further, partial tile
    // of cells past the end may follow)
    const int t_last = (n - 1 - baseB) >> 3;
    // tail cells of the two virtual chunks (see wedm_step_fused): bits per tail cell q and chunk v at 4 (2 q + v):
    // zone, contacts, interior, valid
    const int tail = (EXTRA && Cv > 8 && (Cv & 7) >= 1 && (Cv & 7) <= 2) ? (Cv & 7) : 0;
    uint32_t tail_bits = 0u;
    for (int q = 0; q < tail; ++q) {
        const uint32_t zj = wt->zj[Cv - tail + q], iv = wt->iv[Cv - tail + q];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int vc = 2 * c + v;
            tail_bits |= (((zj >> vc) & 1u) | (((zj >> (16 + vc)) & 1u) << 1) | (((iv >> vc) & 1u) << 2) | (((iv >> (16 + vc)) & 1u) << 3)) << (4 * (2 * q + v));
        }
    }
#elif defined(WEDM_PACKED_WALK_US)
        // ---- halos (OLD values, read before any store of this step)
        const float halo_l = (c > 0) ? col[(R - 1) * CS - 1] : spool;  // left neighbour lane's B[Cv-1]
        const float halo_r = (c < L - 1) ? col[1] : 0.0f;              // right neighbour lane's A[0]
        const float a_last = col[(R - 2) * CS];                        // own A[Cv-1]: left halo of B
        const float b_first = col[CS];                                 // own B[0]: right halo of A
        col[R * CS] = b_first;
        col[(R + 1) * CS] = halo_r;

        // a wave with a negative plasma heat (or, without FROZEN_OK, with a frozen environment) walks every cell on the
        // predicated path; results are identical, only slower
        const bool frozen_wave = FROZEN_OK && __any(WEDM_PACKED_WALK_DONE);
        const bool all_slow = __any(cf.q < 0.0f) || (!FROZEN_OK && __any(WEDM_PACKED_WALK_DONE));
        const uint32_t slow_now = all_slow ? 0xffffffffu : kind_s;
        // regular tiles of THIS microsecond: a contact-flag change inside a tile only matters while current flows
        const uint32_t n_now = (kind_n | kind_ne | (__any(cf.joule_on && !WEDM_PACKED_WALK_DONE && cf.jf != 0.0f) ? 0u : kind_nj)) & ~(all_slow ? 0xffffffffu : 0u);

        // full predicated formula for one owned cell, from OLD values (patched cells)
        auto patch_value = [&](int i, int own) -> float {
            // (unconditional LDS reads from clamped rows, then selects: a conditional read made the compiler select
            // between an LDS and a private address and fall back to flat loads; the rows after the last pair are the
            // halo pair (b_first, halo_r), exactly what the last cell of A / B needs on its right)
            const int v = own - 1, r = i - (v ? baseB : baseA), row = 2 * r + v;
            const float left = col[(r > 0 ? row - 2 : row) * CS];
            float tm = r > 0 ? left : (v ? a_last : halo_l);
            if (i == 1) tm = spool;
            const float tp = col[(row + 2) * CS];
            return stencil_cell(i, n, tm, col[row * CS], tp, g, cf, ps, tref, alpha, tdiel);
        };
        const int own_pl = (!WEDM_PACKED_WALK_DONE && cf.pidx >= 1) ? owner(cf.pidx) : 0;
        float tpl = 0.0f, tlast = 0.0f;
        if (__any(own_pl != 0)) {
            if (own_pl) tpl = patch_value(cf.pidx, own_pl);
        }
        if (own_last && !WEDM_PACKED_WALK_DONE) tlast = patch_value(n - 1, own_last);

        // ---- tail cells: new values from OLD ones, now (not on the predicated path, whose last tile covers them)
        const bool use_tail = EXTRA && tail != 0 && !all_slow;
        WEDM_PACKED_WALK_TAILS_FROM_OLD();
        const int n_walk = use_tail ? n_tiles - 1 : n_tiles;

        f2 tm1 = {halo_l, a_last};
        f2 tc = {col[0], col[CS]};
        WEDM_PACKED_WALK_MARK_TILES;
        if (kWalkTiles) {
            const float jf_lane = (cf.joule_on && !WEDM_PACKED_WALK_DONE) ? cf.jf : 0.0f;
            const bool joule_wave = __any(jf_lane != 0.0f);
            const float cz = ps.conv_zone, cb = ps.conv_base;

            // dst[u] = OLD (A[r0+1+u], B[r0+1+u]); CLAMP = false: all eight pairs exist (r0 + 8 <= Cv),
            // one base address + immediate ds_read2st64 offsets
            auto load8 = [&](auto clamp, f2 (&dst)[8], int r0) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    int p = r0 + 1 + u;
                    if (decltype(clamp)::value) p = p < Cv ? p : Cv;  // pair Cv is the halo pair; later pairs are never used
                    dst[u].x = col[(2 * p) * CS];
                    dst[u].y = col[(2 * p + 1) * CS];
                }
            };
            auto store2 = [&](int r, f2 v) {
                col[(2 * r) * CS] = v.x;
                col[(2 * r + 1) * CS] = v.y;
            };
            auto tile = [&](auto frozen, int t, f2 (&cur)[8]) {
                constexpr bool FROZEN = decltype(frozen)::value;  // the copy for a wave with frozen lanes: they do not store
                const int r0 = 8 * t;
                // One buffer only: the tile's eight "next" pairs are loaded at the tile's start.  A
                // second (prefetch) buffer cost 16 VGPRs, pushed the kernel into scratch spills
                // (236 B/lane, ~30 GB of L2 traffic per launch) and was 7 % slower; the other wave of
                // the SIMD covers the LDS latency instead.
                if (r0 + 8 <= Cv) load8(std::false_type{}, cur, r0);
                else load8(std::true_type{}, cur, r0);
                const f2 conv_lo = {((zlA >> t) & 1u) ? cz : cb, ((zlB >> t) & 1u) ? cz : cb};
                const f2 jfe_lo = {((jlA >> t) & 1u) ? jf_lane : 0.0f, ((jlB >> t) & 1u) ? jf_lane : 0.0f};
                if ((n_now >> t) & 1u) {
                    f2 old[10], tn[8], cv[8], jv[8];
                    old[0] = tm1; old[1] = tc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) old[u + 2] = cur[u];
                    cv[0] = conv_lo; jv[0] = jfe_lo;
                    if (joule_wave && __any(jfe_lo.x != 0.0f || jfe_lo.y != 0.0f)) {
                        WEDM_PACKED_WALK_REGULAR_TILE(true);
                    } else {
                        WEDM_PACKED_WALK_REGULAR_TILE(false);
                    }
                    // the wire's end cells, where a regular tile holds one (kind_ne / kind_nj): cell 0 is the first cell
                    // of lane 0's chunk A and stays at the spool temperature; the last cell is the last cell of the last
                    // lane's chunk B: out of the maximum here, patched after the walk
                    tn[0].x = (c == 0 && t == 0) ? spool : tn[0].x;
                    const float last_y = (own_last == 2 && t == t_last) ? spool : tn[7].y;
                    float m0 = fmax_gt(tn[0].x, tn[0].y), m1 = fmax_gt(tn[1].x, tn[1].y);
                    if (!FROZEN || !WEDM_PACKED_WALK_DONE) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) store2(r0 + u, tn[u]);
                    }
#pragma unroll
                    for (int u = 2; u < 6; u += 2) {
                        m0 = fmax_gt(m0, fmax_gt(tn[u].x, tn[u].y));
                        m1 = fmax_gt(m1, fmax_gt(tn[u + 1].x, tn[u + 1].y));
                    }
                    m0 = fmax_gt(m0, fmax_gt(tn[6].x, tn[6].y));
                    m1 = fmax_gt(m1, fmax_gt(tn[7].x, last_y));
                    tmax = fmax_gt(tmax, fmax_gt(m0, m1));
                    tm1 = cur[6];
                    tc = cur[7];
                } else if (EXTRA && (((kind_n1 & ~slow_now) >> t) & 1u)) {
                    // one flag change at `split`, nothing else irregular (end cells apart): per-cell coefficients, stores
                    // and maximum as in a regular tile
                    const int split = (int)((split_pack[t >> 3] >> ((t & 7) * 4)) & 15u);
                    const f2 conv_hi = {((zhA >> t) & 1u) ? cz : cb, ((zhB >> t) & 1u) ? cz : cb};
                    const f2 jfe_hi = {((jhA >> t) & 1u) ? jf_lane : 0.0f, ((jhB >> t) & 1u) ? jf_lane : 0.0f};
                    f2 old[10], tn[8];
                    old[0] = tm1; old[1] = tc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) old[u + 2] = cur[u];
                    WEDM_PACKED_WALK_ONECHANGE_TILE();
                    tn[0].x = (c == 0 && t == 0) ? spool : tn[0].x;
                    const float last_y = (own_last == 2 && t == t_last) ? spool : tn[7].y;
                    if (!FROZEN || !WEDM_PACKED_WALK_DONE) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) store2(r0 + u, tn[u]);
                    }
                    float m0 = fmax_gt(tn[0].x, tn[0].y), m1 = fmax_gt(tn[1].x, tn[1].y);
#pragma unroll
                    for (int u = 2; u < 6; u += 2) {
                        m0 = fmax_gt(m0, fmax_gt(tn[u].x, tn[u].y));
                        m1 = fmax_gt(m1, fmax_gt(tn[u + 1].x, tn[u + 1].y));
                    }
                    m0 = fmax_gt(m0, fmax_gt(tn[6].x, tn[6].y));
                    m1 = fmax_gt(m1, fmax_gt(tn[7].x, last_y));
                    tmax = fmax_gt(tmax, fmax_gt(m0, m1));
                    tm1 = cur[6];
                    tc = cur[7];
                } else if (!((slow_now >> t) & 1u)) {
                    // TILE_B: interior formula everywhere, one flag change at `split`; boundary and
                    // out-of-wire cells stay out of the max (patched afterwards / never read)
                    const int split = (int)((split_pack[t >> 3] >> ((t & 7) * 4)) & 15u);
                    const int cnt = (Cv - r0) < 8 ? (Cv - r0) : 8;
                    const f2 conv_hi = {((zhA >> t) & 1u) ? cz : cb, ((zhB >> t) & 1u) ? cz : cb};
                    const f2 jfe_hi = {((jhA >> t) & 1u) ? jf_lane : 0.0f, ((jhB >> t) & 1u) ? jf_lane : 0.0f};
                    const uint32_t imA = (uint32_t)(baseA + r0 - 1), imB = (uint32_t)(baseB + r0 - 1);
                    const uint32_t span = (uint32_t)(n - 3);
                    f2 old[10], tn[8];
                    old[0] = tm1; old[1] = tc;
#pragma unroll
                    for (int u = 0; u < 8; ++u) old[u + 2] = cur[u];
                    WEDM_PACKED_WALK_ONECHANGE_TILE();
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (u < cnt) {
                            if (!FROZEN || !WEDM_PACKED_WALK_DONE) store2(r0 + u, tn[u]);
                            const bool inA = (n >= 3) && (imA + (uint32_t)u <= span);
                            const bool inB = (n >= 3) && (imB + (uint32_t)u <= span);
                            tmax = inA ? fmax_gt(tmax, tn[u].x) : tmax;
                            tmax = inB ? fmax_gt(tmax, tn[u].y) : tmax;
                        }
                    }
                    // window after the tile: the last REAL pair of the chunk is what the next tile
                    // (if any) needs; a short tile is always the last one, so only full tiles matter
                    tm1 = cur[6];
                    tc = cur[7];
                } else {
                    // TILE_S: per-cell predicated fallback for both components (rare)
#pragma unroll 1
                    for (int u = 0; u < 8; ++u) {
                        const int r = r0 + u;
                        const uint32_t zj = wt->zj[r], iv = wt->iv[r];
                        const f2 tp1 = cur[0];
#pragma unroll
                        for (int v = 0; v < 2; ++v) {
                            const int vcid = 2 * c + v;
                            const bool zbit = (zj >> vcid) & 1u, jbit = (zj >> (16 + vcid)) & 1u;
                            const bool inter = ((iv >> vcid) & 1u) && !all_slow;
                            const bool valid = ((iv >> (16 + vcid)) & 1u) && !WEDM_PACKED_WALK_DONE;
                            const float conv = zbit ? cz : cb, jfe = jbit ? jf_lane : 0.0f;
                            const float m = v ? tm1.y : tm1.x, cc = v ? tc.y : tc.x, pp = v ? tp1.y : tp1.x;
                            float x = interior_cell<true>(m, cc, pp, g.k, g.tuf, conv, tdiel, ps.adv, jfe, alpha, tref);
                            if (!inter && valid) {
                                const int i = (v ? baseB : baseA) + r;
                                x = (i >= 1) ? stencil_cell(i, n, (i == 1) ? spool : m, cc, pp, g, cf, ps, tref, alpha, tdiel) : spool;
                            }
                            if (valid) {
                                col[(2 * r + v) * CS] = x;
                                tmax = fmax_gt(tmax, x);
                            }
                        }
                        tm1 = tc;
                        tc = tp1;
                        f2 first = cur[0];
#pragma unroll
                        for (int q = 0; q < 7; ++q) cur[q] = cur[q + 1];
                        cur[7] = first;
                    }
                }
            };
            f2 bufA[8];
            if (!FROZEN_OK || !frozen_wave) {
                for (int t = 0; t < n_walk; ++t) tile(std::false_type{}, t, bufA);
            } else {
                for (int t = 0; t < n_walk; ++t) tile(std::true_type{}, t, bufA);
            }
        }
        WEDM_PACKED_WALK_MARK_PATCHES;
        // ---- patches (after every store of the walk): tail cells, then boundary condition, last cell, plasma cell
        if (use_tail && !WEDM_PACKED_WALK_DONE) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q < tail) {
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        if ((tail_bits >> (4 * (2 * q + v))) & 4u) {  // interior: exists, counts, and is not the wire's last cell
                            const float x = WEDM_PACKED_WALK_TAIL_NEW(q, v);
                            col[(2 * (Cv - tail + q) + v) * CS] = x;
                            tmax = fmax_gt(tmax, x);
                        }
                    }
                }
            }
        }
        if (c == 0 && !WEDM_PACKED_WALK_DONE) col[0] = spool;
        if (own_last && !WEDM_PACKED_WALK_DONE) {
            const int v = own_last - 1;
            col[(2 * (n - 1 - (v ? baseB : baseA)) + v) * CS] = tlast;
            tmax = fmax_gt(tmax, tlast);
        }
        if (own_pl) {
            const int v = own_pl - 1;
            col[(2 * (cf.pidx - (v ? baseB : baseA)) + v) * CS] = tpl;
            tmax = fmax_gt(tmax, tpl);
        }
#else
#error "wedm_packed_walk.inc: define WEDM_PACKED_WALK_SETUP or WEDM_PACKED_WALK_US before the #include"
#endif
