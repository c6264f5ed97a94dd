// wedm_normalize.h -- wedm_normalize: running observation / reward normalisation and episode statistics, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The one reduction ACROSS
// environments of the library; the definition (columns, moments, merge, the pairwise tree by global environment index, the
// per-environment rows, the outputs) is in include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// Three kernels, launched in this order on one stream, so that the only synchronisation is the stream's own -- no block ever
// waits for another block, nothing spins, nothing is launched cooperatively, no floating-point atomic exists here:
//   wedm_norm_reduce_kernel  (REDUCE) one WAVE per tile of 256 environments and group of four columns: blocks (tile, column
//       group) of 64 lanes, a lane holding four consecutive environments.  The tile's first two tree levels are three merges
//       in the lane's registers, the other six run inside the wave by ORDER-PRESERVING lane shifts (lane i merges itself with
//       lane i + off as (self, other); a butterfly would swap the arguments in half of the lanes, and merge is not commutative
//       in its bits); lane 0 stores partials[tile][moment][column].  No LDS, no barrier.  A merge is two float64 divisions
//       and the launch is bound by issuing them: with one environment per lane and the last two levels through LDS (the first
//       form of this kernel) a tile cost 4 x 6 + 3 wave-wide merges per column and 65 536 x 37 columns 49 us; this form costs
//       3 + 6, and the column groups keep every SIMD busy although a batch has only one wave per tile.  Lanes whose partner
//       lies past the wave read their own value from the shift; what they compute is never used (only lanes that are
//       multiples of 2 * off feed the next level).  The block that holds column D moves the discounted return on.
//   wedm_norm_fold_kernel    (APPLY, first) one block per column.  Lane i takes the tiles [per * i, per * (i + 1)), per the
//       power of two with 256 * per >= n_tiles_total (at most 16), as a tree in registers; the 256 lanes' nodes go through
//       six shift levels and, wave by wave through LDS, two more: the pairwise tree over the tile index, padded with EMPTY.  Lane 0 merges the
//       running statistics with the batch and stores stats_out.  stats_in and stats_out are different memory, so a replay
//       or a second shard's APPLY reads what the first read.
//   wedm_norm_apply_kernel   (APPLY, second) one lane per environment: mean and sqrt(var + eps) of every column once per
//       block into LDS, then the outputs and the episode rows.  The transposing store of obs_out ([env][D], 4 bytes per lane
//       at a pitch of 4 * D) is left plain: a lane's D stores fill its own D * 4 contiguous bytes back to back and meet in L2.
// Every index is formed from thread and block numbers and descriptor fields alone, never from data: a NaN or an infinity in
// a plane reaches numbers only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"

struct wedm_norm_moments {
    double n, m, S;
};

// merge(a, b) of the header, operation for operation (-ffp-contract=off: nothing is fused); the selects come last so that an
// EMPTY argument hands back the other one's bits whatever the arithmetic made of the zeros
__device__ __forceinline__ wedm_norm_moments wedm_norm_merge(const wedm_norm_moments a, const wedm_norm_moments b) {
    const double n = a.n + b.n;
    const double d = b.m - a.m;
    wedm_norm_moments r;
    r.n = n;
    r.m = a.m + d * (b.n / n);
    r.S = a.S + b.S + d * d * (a.n * b.n / n);
    if (a.n == 0.0) r = b;
    if (b.n == 0.0) r = a;
    return r;
}

// six tree levels over the 64 lanes of a wave, lower lane on the left; the wave's node is lane 0's.  Every lane must arrive.
__device__ __forceinline__ wedm_norm_moments wedm_norm_wave_tree(wedm_norm_moments v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        wedm_norm_moments o;
        o.n = __shfl_down(v.n, off);
        o.m = __shfl_down(v.m, off);
        o.S = __shfl_down(v.S, off);
        v = wedm_norm_merge(v, o);
    }
    return v;
}

__device__ __forceinline__ const float* wedm_norm_row(const wedm_norm_desc& d, int32_t c) {
    const int32_t n0 = d.plane[0].n_rows;
    return c < n0 ? d.plane[0].rows + (int64_t)c * d.plane[0].stride : d.plane[1].rows + (int64_t)(c - n0) * d.plane[1].stride;
}

#ifndef WEDM_NORM_GROUP  // columns per block of the reduce kernel, columns in flight per lane of the apply kernel
#define WEDM_NORM_GROUP 4  // (-D: tools/build_variant.py, for measuring another choice)
#endif
#define WEDM_NORM_PER_LANE (WEDM_NORM_TILE / 64)  // environments a lane of the reduce kernel holds: 4

// block (t, y), one wave: tile t, columns [c_first + y * WEDM_NORM_GROUP, + WEDM_NORM_GROUP) of the C.  c_first is 0, or D in
// evaluation mode, where one block per tile only moves the discounted return on.
__global__ void __launch_bounds__(64) wedm_norm_reduce_kernel(const wedm_norm_desc d, const int32_t D, const int32_t c_first) {
    const int32_t lane = (int32_t)threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * WEDM_NORM_TILE + lane * WEDM_NORM_PER_LANE;
    const bool step = (d.flags & WEDM_NORM_STEP) != 0;
    const int32_t C = D + 1;
    const int32_t c0 = c_first + (int32_t)blockIdx.y * WEDM_NORM_GROUP, c1 = min(c0 + WEDM_NORM_GROUP, C);
    bool in[WEDM_NORM_PER_LANE];
    double ret[WEDM_NORM_PER_LANE];
#pragma unroll
    for (int j = 0; j < WEDM_NORM_PER_LANE; ++j) {
        const int64_t e = e0 + j;
        in[j] = e < d.num_envs && (!d.mask || d.mask[e] != 0);
        ret[j] = 0.0;
        if (step && c1 == C && in[j]) {  // the block that holds column D is the one that moves the return on: nobody else reads it
            ret[j] = d.ret[e] * d.gamma + (double)d.reward[e];
            d.ret[e] = ret[j];
        }
    }
    if (!(d.flags & WEDM_NORM_UPDATE)) return;  // (uniform) evaluation mode: no statistics
    for (int32_t c = c0; c < c1; ++c) {  // (uniform: every lane takes every shift)
        wedm_norm_moments leaf[WEDM_NORM_PER_LANE];
#pragma unroll
        for (int j = 0; j < WEDM_NORM_PER_LANE; ++j) {
            const bool have = in[j] && (c < D || step);
            double x = ret[j];
            if (c < D) x = in[j] ? (double)wedm_norm_row(d, c)[e0 + j] : 0.0;
            leaf[j].n = have ? 1.0 : 0.0;
            leaf[j].m = have ? x : 0.0;
            leaf[j].S = 0.0;
        }
        const wedm_norm_moments v =
            wedm_norm_wave_tree(wedm_norm_merge(wedm_norm_merge(leaf[0], leaf[1]), wedm_norm_merge(leaf[2], leaf[3])));
        if (lane == 0) {
            double* const out = d.partials + ((int64_t)d.tile_offset + blockIdx.x) * WEDM_NORM_MOMENTS * C + c;
            out[WEDM_NM_COUNT * C] = v.n;
            out[WEDM_NM_MEAN * C] = v.m;
            out[WEDM_NM_M2 * C] = v.S;
        }
    }
}

#define WEDM_NORM_FOLD_PER 16  // tiles per lane at most: 256 * 16 = WEDM_NORM_MAX_TILES

// the pairwise tree over the tile index, padded with EMPTY, of column c of a [n_tiles_total][WEDM_NORM_MOMENTS][C] workspace,
// by a block of 256 lanes (see wedm_norm_fold_kernel above).  Every thread must arrive; thread 0 returns the tree's root,
// the others a node nobody needs.  s_node: four triples of LDS.
__device__ __forceinline__ wedm_norm_moments wedm_norm_fold_tiles(const double* partials, const int32_t n_tiles_total, const int32_t C,
                                                                   const int32_t c, const int32_t per,
                                                                   double (*s_node)[WEDM_NORM_MOMENTS]) {
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, w = tid >> 6;
    wedm_norm_moments v[WEDM_NORM_FOLD_PER];
#pragma unroll
    for (int j = 0; j < WEDM_NORM_FOLD_PER; ++j) {
        const int32_t t = tid * per + j;
        const bool have = j < per && t < n_tiles_total;
        const double* const p = partials + (int64_t)(have ? t : 0) * WEDM_NORM_MOMENTS * C + c;
        v[j].n = have ? p[WEDM_NM_COUNT * C] : 0.0;
        v[j].m = have ? p[WEDM_NM_MEAN * C] : 0.0;
        v[j].S = have ? p[WEDM_NM_M2 * C] : 0.0;
    }
#pragma unroll
    for (int s = 1; s < WEDM_NORM_FOLD_PER; s <<= 1) {
#pragma unroll
        for (int j = 0; j < WEDM_NORM_FOLD_PER; j += 2 * s) v[j] = wedm_norm_merge(v[j], v[j + s]);
    }
    wedm_norm_moments node = wedm_norm_wave_tree(v[0]);
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
        node = wedm_norm_merge(wedm_norm_merge(q[0], q[1]), wedm_norm_merge(q[2], q[3]));
    }
    return node;
}

__global__ void __launch_bounds__(256) wedm_norm_fold_kernel(const wedm_norm_desc d, const int32_t C, const int32_t per) {
    __shared__ double s_node[4][WEDM_NORM_MOMENTS];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t c = (int32_t)blockIdx.x;
    wedm_norm_moments run;
    run.n = d.stats_in[WEDM_NM_COUNT * C + c];
    run.m = d.stats_in[WEDM_NM_MEAN * C + c];
    run.S = d.stats_in[WEDM_NM_M2 * C + c];
    if (d.flags & WEDM_NORM_UPDATE)  // (uniform)
        run = wedm_norm_merge(run, wedm_norm_fold_tiles(d.partials, d.n_tiles_total, C, c, per, s_node));  // (thread 0's counts)
    if (tid == 0) {
        d.stats_out[WEDM_NM_COUNT * C + c] = run.n;
        d.stats_out[WEDM_NM_MEAN * C + c] = run.m;
        d.stats_out[WEDM_NM_M2 * C + c] = run.S;
    }
}

__device__ __forceinline__ double wedm_norm_clamp(double v, double clip) { return v < -clip ? -clip : (v > clip ? clip : v); }

__global__ void __launch_bounds__(WEDM_NORM_TILE) wedm_norm_apply_kernel(const wedm_norm_desc d, const int32_t D) {
    __shared__ double s_mean[WEDM_NORM_MAX_COLUMNS], s_den[WEDM_NORM_MAX_COLUMNS];
    __shared__ uint8_t s_skip[WEDM_NORM_MAX_COLUMNS];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t C = D + 1;
    if (tid < C) {
        const double n = d.stats_out[WEDM_NM_COUNT * C + tid], S = d.stats_out[WEDM_NM_M2 * C + tid];
        s_mean[tid] = d.stats_out[WEDM_NM_MEAN * C + tid];
        s_den[tid] = sqrt(S / n + d.eps);
        s_skip[tid] = d.skip && tid < D ? d.skip[tid] : (uint8_t)0;
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * WEDM_NORM_TILE + tid;
    if (e >= d.num_envs) return;
    float* const out = d.obs_out + e * D;
    for (int32_t c0 = 0; c0 < D; c0 += WEDM_NORM_GROUP) {  // a group's loads first: the stores behind them may alias for all the compiler knows
        float x[WEDM_NORM_GROUP];
#pragma unroll
        for (int g = 0; g < WEDM_NORM_GROUP; ++g) x[g] = wedm_norm_row(d, min(c0 + g, D - 1))[e];  // (repeats of row D - 1: not stored)
#pragma unroll
        for (int g = 0; g < WEDM_NORM_GROUP; ++g) {
            const int32_t c = c0 + g;
            if (c < D) {
                float y = x[g];
                if (s_skip[c] == 0) y = (float)wedm_norm_clamp(((double)x[g] - s_mean[c]) / s_den[c], d.clip_obs);
                out[c] = y;
            }
        }
    }
    if (!(d.flags & WEDM_NORM_STEP)) return;
    const double r = (double)d.reward[e];
    d.reward_out[e] = (float)wedm_norm_clamp(r / s_den[D], d.clip_reward);
    if (d.mask && d.mask[e] == 0) return;  // left out: every row stays
    const double total = d.ep_return[e] + r;
    const int32_t length = d.ep_length[e] + 1;
    if ((d.terminated[e] | d.truncated[e]) != 0) {
        d.last_return[e] = total;
        d.last_length[e] = length;
        d.ep_count[e] += 1;
        d.finished[e] = 1;
        d.ep_return[e] = 0.0;
        d.ep_length[e] = 0;
        d.ret[e] = 0.0;
    } else {
        d.ep_return[e] = total;
        d.ep_length[e] = length;
        d.finished[e] = 0;
    }
}
