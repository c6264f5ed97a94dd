// wedm_copy.h -- wedm_copy_columns: environments' columns moved between (or within) caller-owned blocks, on the device.
//
// Not a step kernel and not in the registry: it touches no wedm_ctx, no wedm_params and no plan.  Every block of the ABI is
// [rows][stride] of some element width with the environment as the column (the quad-interleaved T block is
// [WEDM_T_QUADS][stride] of 16-byte words), so "environment a becomes environment b" is the same operation on every block:
// column a of every row to column b.  A PLANE (wedm_copy_plane, include/wedm_hip.h) names one block on both sides; one
// launch serves up to WEDM_COPY_MAX_PLANES of them, passed by value in the kernarg segment together with a table that
// cuts every plane into work items of at most WEDM_COPY_ROWS rows.
//
// Shape: blockDim 256; blockIdx.x runs over the index pairs, so consecutive pairs are consecutive lanes (the common
// destination is a contiguous range: coalesced stores; the common source is a contiguous range or one column: coalesced or
// broadcast loads).  blockIdx.y runs over the work items.  Item y of the launch belongs to the first plane p with
// y < item_end[p] and covers its rows [(y - item_end[p - 1]) * 8, + 8) -- the table holds the planes' running item counts,
// which names every (plane, first_row, n_rows) item without bounding the rows of a plane.  Plane and rows are
// wave-uniform: the plane's fields come through scalar loads and the element width is a uniform switch to four bodies.
// A lane reads its index pair once and issues the (at most eight) independent loads of its item before the first store:
// what hides the latency of a 1- to 16-byte gather is those loads in flight, not occupancy.  Eight 16-byte loads are
// 32 VGPRs; more rows per item would buy nothing (a wave may have far more than eight loads outstanding, and the grid
// supplies the rest of the parallelism) and would leave short planes (i8: 8 rows, reward: 1) with fewer items.
// No LDS, plain vector loads and stores of raw integer words (1, 4, 8 or 16 bytes wide): no float instruction
// touches a payload, so NaNs (WEDM_F_SPARK_Y) keep every bit.
//
// Bounds: a pair whose source is outside [0, src_cols) or whose destination is outside [0, dst_cols) of the item's plane
// moves nothing in that plane and ORs bit 0 into *status (where given) with a vector atomic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"

#define WEDM_COPY_ROWS 8

// a 16-byte word as a native vector (an array of HIP's uint4 class does not stay in registers)
typedef uint32_t wedm_u32x4 __attribute__((ext_vector_type(4)));

struct wedm_copy_args {
    wedm_copy_plane plane[WEDM_COPY_MAX_PLANES];
    int32_t item_end[WEDM_COPY_MAX_PLANES];  // work items of planes 0 .. p, running count
    int32_t n_planes;
    int32_t item0;  // first item of this launch (a call with more items than a grid's y extent is several launches)
};

template <typename W>
__device__ __forceinline__ void wedm_copy_item(const wedm_copy_plane& pl, int32_t first_row, int32_t n_rows, int64_t s,
                                               int64_t d) {
    const W* src = (const W*)pl.src + (int64_t)first_row * pl.src_stride + s;
    W* dst = (W*)pl.dst + (int64_t)first_row * pl.dst_stride + d;
    const int64_t ss = pl.src_stride, ds = pl.dst_stride;
    W v[WEDM_COPY_ROWS];
    if (n_rows == WEDM_COPY_ROWS) {  // (uniform)
#pragma unroll
        for (int r = 0; r < WEDM_COPY_ROWS; ++r) v[r] = src[r * ss];
#pragma unroll
        for (int r = 0; r < WEDM_COPY_ROWS; ++r) dst[r * ds] = v[r];
    } else {  // a plane's last item: the rows past its end load its last row again (in bounds, v stays in registers)
#pragma unroll
        for (int r = 0; r < WEDM_COPY_ROWS; ++r) v[r] = src[min(r, n_rows - 1) * ss];
#pragma unroll
        for (int r = 0; r < WEDM_COPY_ROWS; ++r)
            if (r < n_rows) dst[r * ds] = v[r];
    }
}

__global__ void __launch_bounds__(256)
wedm_copy_columns_kernel(const wedm_copy_args a, const int32_t* __restrict__ src_idx, const int32_t* __restrict__ dst_idx,
                         int32_t count, int32_t* status) {
    const int32_t y = (int32_t)blockIdx.y + a.item0;
    int32_t p = 0, before = 0;
    while (p < a.n_planes - 1 && y >= a.item_end[p]) before = a.item_end[p++];
    if (y >= a.item_end[p]) return;  // (never: the host sizes the grid by the table)
    const wedm_copy_plane& pl = a.plane[p];
    const int32_t first_row = (y - before) * WEDM_COPY_ROWS;
    const int32_t n_rows = min(WEDM_COPY_ROWS, pl.rows - first_row);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int32_t s = src_idx[i], d = dst_idx[i];
    if ((uint32_t)s >= (uint32_t)pl.src_cols || (uint32_t)d >= (uint32_t)pl.dst_cols) {
        if (status) atomicOr(status, 1);
        return;
    }
    switch (pl.elem_bytes) {  // (uniform)
        case 1: wedm_copy_item<uint8_t>(pl, first_row, n_rows, s, d); break;
        case 4: wedm_copy_item<uint32_t>(pl, first_row, n_rows, s, d); break;
        case 8: wedm_copy_item<uint64_t>(pl, first_row, n_rows, s, d); break;
        default: wedm_copy_item<wedm_u32x4>(pl, first_row, n_rows, s, d); break;
    }
}
