// wedm_gae.h -- wedm_gae: a rollout's advantages (GAE), returns, valid mask and standardised advantages, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the
// recurrence with every rounding, the step after a done under next-step autoreset, Welford per environment, the pairwise tree
// by global environment index) is in include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// Three kernels, launched in this order on one stream, so that the only synchronisation is the stream's own -- no block ever
// waits for another block, nothing spins, nothing is launched cooperatively, no floating-point atomic exists here:
//   wedm_gae_scan_kernel   (SCAN) one lane per environment, a block of 256 lanes is one tile, the time loop runs in the lane
//       from t = T - 1 down.  Row t of every block is read and written by consecutive lanes at consecutive environments: every
//       access is coalesced.  The recurrence is a short dependent float64 chain (a multiply and two adds per step; with
//       NORMALIZE Welford's division beside it, on a chain of its own), but no load depends on it: the time loop runs in
//       chunks of WEDM_GAE_UNROLL steps, and the loads of a whole chunk are issued before the chain of the chunk before it
//       starts, so that many rows are in flight per lane while it computes.  A
//       step needs the flags of step t - 1 (was the step before a done?); they are loaded with step t and carried to step
//       t - 1 as its own flags, as value[t] is carried to it as its next value: 10 bytes are read and 9 written per step.
//       With NORMALIZE the lane's Welford triple then goes through the tile's tree: six levels in the wave
//       (wedm_norm_wave_tree), two over the four waves' nodes through LDS, the lower wave on the left; thread 0 stores
//       partials[tile_offset + tile].  Lanes past num_envs skip the time loop, hold EMPTY and take every shuffle.
//   wedm_gae_fold_kernel   (APPLY, first) one block: wedm_normalize's tree over the tile index (wedm_norm_fold_tiles) on the
//       one-column workspace; thread 0 stores moments.
//   wedm_gae_apply_kernel  (APPLY, second) element-wise: a block takes a tile's 256 environments and WEDM_GAE_APPLY_ROWS rows,
//       loads first.
// Every index is formed from thread and block numbers and descriptor fields alone, never from data: a NaN or an infinity in a
// block reaches numbers only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_normalize.h"  // wedm_norm_moments, wedm_norm_merge, wedm_norm_wave_tree, wedm_norm_fold_tiles: written once

#ifndef WEDM_GAE_UNROLL  // steps of the scan's time loop whose loads are issued together
#define WEDM_GAE_UNROLL 8  // (-D: tools/build_variant.py, for measuring another choice; sparc_amd.rollout.SCAN_UNROLL names it)
#endif
#define WEDM_GAE_APPLY_ROWS 8  // rows a block of the apply kernel takes

// what a lane carries from step t + 1 to step t
struct wedm_gae_carry {
    double A;             // A_{t+1}; 0 before step T - 1
    double nv;            // (double) value[t+1][e]; last_value[e] before step T - 1
    uint8_t term, trunc;  // of step t itself: loaded with step t + 1, which asks whether the step before it was a done
    wedm_norm_moments w;  // Welford over the valid steps so far
};

// what steps t_hi, t_hi - 1, ..., t_hi - U + 1 (all of them >= 0) load; *_before: the flags of the step before each
template <int U>
struct wedm_gae_rows {
    float r[U], v[U];
    uint8_t term_before[U], trunc_before[U];
};

// every load of U steps of environment e < num_envs: none depends on the recurrence
template <int U>
__device__ __forceinline__ void wedm_gae_load(const wedm_gae_desc& d, const int64_t e, const int32_t t_hi, const uint8_t prev_done,
                                              wedm_gae_rows<U>& x) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int32_t t = t_hi - j;
        const int64_t at = (int64_t)t * d.in_stride + e;
        x.r[j] = d.reward[at];
        x.v[j] = d.value[at];
        x.term_before[j] = prev_done;
        x.trunc_before[j] = 0;
        if (t > 0) {  // (uniform)
            x.term_before[j] = d.terminated[at - d.in_stride];
            x.trunc_before[j] = d.truncated[at - d.in_stride];
        }
    }
}

// the recurrence over the U steps that `x` holds, and their stores
template <int U>
__device__ __forceinline__ void wedm_gae_steps(const wedm_gae_desc& d, const int64_t e, const int32_t t_hi, const double gl,
                                               const wedm_gae_rows<U>& x, wedm_gae_carry& s) {
    const bool skip_after_done = (d.flags & WEDM_GAE_SKIP_AFTER_DONE) != 0, normalize = (d.flags & WEDM_GAE_NORMALIZE) != 0;
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int64_t at = (int64_t)(t_hi - j) * d.out_stride + e;
        const bool term = s.term != 0, done = (s.term | s.trunc) != 0;
        const bool skip = skip_after_done && (x.term_before[j] | x.trunc_before[j]) != 0;
        const double val = (double)x.v[j];
        const double delta = ((double)x.r[j] + (term ? 0.0 : d.gamma * s.nv)) - val;
        const double A = skip ? 0.0 : delta + (done ? 0.0 : gl * s.A);
        const float Af = (float)A;
        d.advantage[at] = Af;
        d.returns[at] = (float)(A + val);
        d.valid[at] = skip ? (uint8_t)0 : (uint8_t)1;
        if (normalize) {  // (uniform)
            const double xa = (double)Af;
            const double n = s.w.n + 1.0;
            const double dx = xa - s.w.m;
            const double m = s.w.m + dx / n;
            const double S = s.w.S + dx * (xa - m);
            s.w.n = skip ? s.w.n : n;
            s.w.m = skip ? s.w.m : m;
            s.w.S = skip ? s.w.S : S;
        }
        s.A = A;
        s.nv = val;
        s.term = x.term_before[j];
        s.trunc = x.trunc_before[j];
    }
}

__global__ void __launch_bounds__(WEDM_NORM_TILE) wedm_gae_scan_kernel(const wedm_gae_desc d) {
    __shared__ double s_node[4][WEDM_NORM_MOMENTS];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t e = (int64_t)blockIdx.x * WEDM_NORM_TILE + tid;
    const bool in = e < d.num_envs;
    const double gl = d.gamma * d.lam;
    wedm_gae_carry s;
    s.w.n = s.w.m = s.w.S = 0.0;
    if (in) {  // the lanes past the batch's end wait at the tree below, with EMPTY
        const int64_t last = (int64_t)(d.T - 1) * d.in_stride + e;
        const uint8_t prev_done = (d.flags & WEDM_GAE_SKIP_AFTER_DONE) && d.prev_done_in ? d.prev_done_in[e] : (uint8_t)0;
        s.A = 0.0;
        s.nv = (double)d.last_value[e];
        s.term = d.terminated[last];
        s.trunc = d.truncated[last];
        if (d.prev_done_out) d.prev_done_out[e] = (s.term | s.trunc) != 0 ? (uint8_t)1 : (uint8_t)0;  // (prev_done_in[e] is read)
        constexpr int U = WEDM_GAE_UNROLL;
        int32_t t = d.T - 1;
        if (t >= U - 1) {  // whole chunks of U steps; the next chunk's loads are issued before this chunk's chain starts
            wedm_gae_rows<U> cur, next;
            wedm_gae_load<U>(d, e, t, prev_done, cur);
            for (; t - U >= U - 1; t -= U) {
                wedm_gae_load<U>(d, e, t - U, prev_done, next);
                wedm_gae_steps<U>(d, e, t, gl, cur, s);
                cur = next;
            }
            wedm_gae_steps<U>(d, e, t, gl, cur, s);
            t -= U;
        }
        for (; t >= 0; --t) {  // the steps that fill no chunk, one by one
            wedm_gae_rows<1> one;
            wedm_gae_load<1>(d, e, t, prev_done, one);
            wedm_gae_steps<1>(d, e, t, gl, one, s);
        }
    }
    if (!(d.flags & WEDM_GAE_NORMALIZE)) return;  // (uniform)
    const wedm_norm_moments node = wedm_norm_wave_tree(s.w);
    if (lane == 0) {
        s_node[w][WEDM_NM_COUNT] = node.n;
        s_node[w][WEDM_NM_MEAN] = node.m;
        s_node[w][WEDM_NM_M2] = node.S;
    }
    __syncthreads();
    if (tid == 0) {
        wedm_norm_moments q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k].n = s_node[k][WEDM_NM_COUNT];
            q[k].m = s_node[k][WEDM_NM_MEAN];
            q[k].S = s_node[k][WEDM_NM_M2];
        }
        const wedm_norm_moments tile = wedm_norm_merge(wedm_norm_merge(q[0], q[1]), wedm_norm_merge(q[2], q[3]));
        double* const out = d.partials + ((int64_t)d.tile_offset + blockIdx.x) * WEDM_NORM_MOMENTS;
        out[WEDM_NM_COUNT] = tile.n;
        out[WEDM_NM_MEAN] = tile.m;
        out[WEDM_NM_M2] = tile.S;
    }
}

__global__ void __launch_bounds__(256) wedm_gae_fold_kernel(const wedm_gae_desc d, const int32_t per) {
    __shared__ double s_node[4][WEDM_NORM_MOMENTS];
    const wedm_norm_moments batch = wedm_norm_fold_tiles(d.partials, d.n_tiles_total, 1, 0, per, s_node);
    if (threadIdx.x == 0) {
        d.moments[WEDM_NM_COUNT] = batch.n;
        d.moments[WEDM_NM_MEAN] = batch.m;
        d.moments[WEDM_NM_M2] = batch.S;
    }
}

// block (x, y): environments [256 x, 256 x + 256), rows [WEDM_GAE_APPLY_ROWS y, + WEDM_GAE_APPLY_ROWS)
__global__ void __launch_bounds__(WEDM_NORM_TILE) wedm_gae_apply_kernel(const wedm_gae_desc d) {
    const int64_t e = (int64_t)blockIdx.x * WEDM_NORM_TILE + (int32_t)threadIdx.x;
    if (e >= d.num_envs) return;
    const double n = d.moments[WEDM_NM_COUNT], m = d.moments[WEDM_NM_MEAN], S = d.moments[WEDM_NM_M2];
    const double den = sqrt(S / n + d.eps);  // (n == 0: not used)
    const int32_t t0 = (int32_t)blockIdx.y * WEDM_GAE_APPLY_ROWS;
    float a[WEDM_GAE_APPLY_ROWS];
    uint8_t ok[WEDM_GAE_APPLY_ROWS];
#pragma unroll
    for (int j = 0; j < WEDM_GAE_APPLY_ROWS; ++j) {
        const int64_t at = (int64_t)min(t0 + j, d.T - 1) * d.out_stride + e;  // (repeats of row T - 1: not stored)
        a[j] = d.advantage[at];
        ok[j] = d.valid[at];
    }
#pragma unroll
    for (int j = 0; j < WEDM_GAE_APPLY_ROWS; ++j) {
        if (t0 + j < d.T)  // (uniform)
            d.advantage_norm[(int64_t)(t0 + j) * d.out_stride + e] =
                ok[j] != 0 && n != 0.0 ? (float)(((double)a[j] - m) / den) : 0.0f;
    }
}
