// wedm_eplog.h -- wedm_episode_log: the ordered ring of finished episodes and the per-episode sums, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (live,
// finish, the rank k by global environment index, the slot, the rule k >= n - capacity, the accumulators, head) is in
// include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// Three kernels, launched in this order on one stream, so that the only synchronisation is the stream's own -- no block ever
// waits for another block, nothing spins, nothing is launched cooperatively, and there is no atomic here at all:
//   wedm_elog_count_kernel    (COUNT) a block of 256 is a tile: a wave's finishing lanes are the population count of its 64-bit
//       __ballot, the four waves' counts meet in LDS, thread 0 stores tile_counts[tile_offset + tile].
//   wedm_elog_scatter_kernel  (SCATTER) blocks (tile, plane) of 256 lanes, the plane uniform per block, so that its fields come
//       through scalar loads from the kernarg segment and kind and element width are uniform switches.  Every block forms
//       the ranks of its tile again (they are cheap and nobody has to wait for anybody): a lane's rank inside its wave is
//       the population count of the ballot below the lane (v_mbcnt), the waves before it come through LDS, the tiles below
//       and the call's total n are block sums over the at most 4096 int32 of tile_counts -- integer sums, any order.  A
//       block of a LAST plane whose tile finishes nobody returns at once: with few episodes ending, a step touches the
//       SUM planes only.  LAST rows move through wedm_copy.h's column copy (eight independent loads in flight before
//       the first store, raw integer words: no float instruction touches a payload); SUM rows four at a time, loads
//       first.  The blocks of plane 0 also write env_out and stamp_out.
//   wedm_elog_commit_kernel   (COMMIT) one wave: n once more, then head[0] += n, head[1] = n by lane 0.
// Every offset is formed in 64 bits.  A lane past num_envs takes part in every ballot and barrier and touches no memory.
// A slot is (head[0] + k) mod capacity, in [0, capacity) whatever head and tile_counts hold; only records with k >= n - capacity are stored, so two
// stored records of one call differ by less than capacity in k and never share a slot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_copy.h"

#define WEDM_ELOG_SUM_ROWS 4  // SUM rows a lane has in flight

struct wedm_elog_fin {
    bool live, fin;
};

__device__ __forceinline__ wedm_elog_fin wedm_elog_finishes(const wedm_elog_desc& d, int64_t e) {
    wedm_elog_fin r;
    r.live = e < d.num_envs && (!d.mask || d.mask[e] != 0);
    r.fin = false;
    if (r.live) r.fin = (d.terminated[e] | (d.truncated ? d.truncated[e] : (uint8_t)0)) != 0;
    return r;
}

// the sum of a wave's 64 int32 (every lane must arrive; every lane returns it)
__device__ __forceinline__ int32_t wedm_elog_wave_sum(int32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(WEDM_NORM_TILE) wedm_elog_count_kernel(const wedm_elog_desc d) {
    __shared__ int32_t s_fin[4];
    const int32_t tid = (int32_t)threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * WEDM_NORM_TILE + tid;
    const unsigned long long b = __ballot(wedm_elog_finishes(d, e).fin);
    if ((tid & 63) == 0) s_fin[tid >> 6] = __popcll(b);
    __syncthreads();
    if (tid == 0) d.tile_counts[(int64_t)d.tile_offset + blockIdx.x] = s_fin[0] + s_fin[1] + s_fin[2] + s_fin[3];
}

template <typename S, typename A>
__device__ __forceinline__ void wedm_elog_sum_plane(const wedm_elog_plane& pl, const int64_t num_envs, const int64_t capacity,
                                                    const int64_t e, const int64_t slot, const bool fin, const bool write) {
    const S* const src = (const S*)pl.src + e;
    A* const acc = (A*)pl.acc + e;
    A* const dst = (A*)pl.dst + slot;
    for (int32_t r0 = 0; r0 < pl.n_rows; r0 += WEDM_ELOG_SUM_ROWS) {  // (uniform)
        A v[WEDM_ELOG_SUM_ROWS];
#pragma unroll
        for (int j = 0; j < WEDM_ELOG_SUM_ROWS; ++j) {
            const int64_t r = min(r0 + j, pl.n_rows - 1);  // (repeats of the last row: not stored)
            v[j] = acc[r * num_envs] + (A)src[r * pl.src_stride];
        }
#pragma unroll
        for (int j = 0; j < WEDM_ELOG_SUM_ROWS; ++j) {
            const int64_t r = r0 + j;
            if (r < pl.n_rows) {
                if (write) dst[r * capacity] = v[j];
                acc[r * num_envs] = fin ? (A)0 : v[j];
            }
        }
    }
}

__global__ void __launch_bounds__(WEDM_NORM_TILE) wedm_elog_scatter_kernel(const wedm_elog_desc d) {
    __shared__ int32_t s_fin[4], s_below[4], s_all[4];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t e = (int64_t)blockIdx.x * WEDM_NORM_TILE + tid;
    const wedm_elog_fin f = wedm_elog_finishes(d, e);
    const unsigned long long b = __ballot(f.fin);
    const int32_t tile = d.tile_offset + (int32_t)blockIdx.x;
    int32_t below = 0, all = 0;
    for (int32_t t = tid; t < d.n_tiles_total; t += WEDM_NORM_TILE) {
        const int32_t c = d.tile_counts[t];
        all += c;
        below += t < tile ? c : 0;
    }
    below = wedm_elog_wave_sum(below);
    all = wedm_elog_wave_sum(all);
    if (lane == 0) {
        s_fin[w] = __popcll(b);
        s_below[w] = below;
        s_all[w] = all;
    }
    __syncthreads();
    const wedm_elog_plane& pl = d.plane[blockIdx.y];  // (uniform: scalar loads)
    const bool last = pl.kind == WEDM_ELOG_LAST;
    if (last && s_fin[0] + s_fin[1] + s_fin[2] + s_fin[3] == 0) return;  // (uniform) nobody of this tile finishes
    int64_t k = (int64_t)s_below[0] + s_below[1] + s_below[2] + s_below[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) k += j < w ? s_fin[j] : 0;
    k += (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const int64_t n = (int64_t)s_all[0] + s_all[1] + s_all[2] + s_all[3];
    const bool write = f.fin && k >= n - d.capacity;
    int64_t slot = write ? (d.head[0] + k) % d.capacity : 0;
    if (slot < 0) slot += d.capacity;  // (a head below zero is the caller's mistake: the slot stays inside the ring whatever it holds)
    if (blockIdx.y == 0 && write) {
        d.env_out[slot] = d.env_id_offset + e;
        d.stamp_out[slot] = d.stamp;
    }
    if (last) {
        if (!write) return;
        wedm_copy_plane cp;
        cp.src = pl.src;
        cp.dst = pl.dst;
        cp.src_stride = pl.src_stride;
        cp.dst_stride = d.capacity;
        for (int32_t r0 = 0; r0 < pl.n_rows; r0 += WEDM_COPY_ROWS) {  // (uniform)
            const int32_t rows = min(WEDM_COPY_ROWS, pl.n_rows - r0);
            switch (pl.elem_bytes) {  // (uniform)
                case 1: wedm_copy_item<uint8_t>(cp, r0, rows, e, slot); break;
                case 4: wedm_copy_item<uint32_t>(cp, r0, rows, e, slot); break;
                default: wedm_copy_item<uint64_t>(cp, r0, rows, e, slot); break;
            }
        }
        return;
    }
    if (!f.live) return;
    switch (pl.kind) {  // (uniform)
        case WEDM_ELOG_SUM_F32: wedm_elog_sum_plane<float, double>(pl, d.num_envs, d.capacity, e, slot, f.fin, write); break;
        case WEDM_ELOG_SUM_F64: wedm_elog_sum_plane<double, double>(pl, d.num_envs, d.capacity, e, slot, f.fin, write); break;
        default: wedm_elog_sum_plane<int32_t, int64_t>(pl, d.num_envs, d.capacity, e, slot, f.fin, write); break;
    }
}

__global__ void __launch_bounds__(64) wedm_elog_commit_kernel(const wedm_elog_desc d) {
    const int32_t lane = (int32_t)threadIdx.x;
    int32_t part = 0;  // (at most 4096 * 256 in all: no overflow)
    for (int32_t t = lane; t < d.n_tiles_total; t += 64) part += d.tile_counts[t];
    const int64_t n = wedm_elog_wave_sum(part);
    if (lane == 0) {
        d.head[0] += n;
        d.head[1] = n;
    }
}
