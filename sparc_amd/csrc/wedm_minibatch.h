// wedm_minibatch.h -- wedm_minibatch_index: the rows of a rollout dealt into minibatches by a seeded permutation, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the ranks k
// and q, the keys, the bijection E, the walk PI, the round-robin placement) is in include/wedm_hip.h and tests hold these
// kernels to it on every byte.  Integers only.
//
// Three kernels, launched in this order on one stream, so that the only synchronisation is the stream's own -- no block ever
// waits for another block, nothing spins, nothing is launched cooperatively, and there is no atomic here at all:
//   wedm_mb_count_kernel    (COUNT) a block of 256 lanes is a tile of 1024 rows, four rows per lane: lane l takes the aligned
//       word l of the tile (`valid` may sit at any byte address, so a tile touches 257 words when it does not start on one;
//       lane 0 takes the last) as one dword load where the whole word lies inside the tile and inside `valid`, byte by byte
//       at the tile's head and tail.  The non-zero bytes of a word are counted by or-folding every byte onto its bit 0; a
//       wave sums by shuffles, the four waves meet in LDS, thread 0 stores tile_counts[tile].
//   wedm_mb_offsets_kernel  (OFFSETS) ONE block of 1024 lanes: an exclusive scan over the tile counts in passes of 1024
//       (a wave's inclusive scan by shuffles, the sixteen waves' totals through LDS, double-buffered: one barrier per pass),
//       the running total carried in a register; thread 0 writes count = {V, rows - V}.
//   wedm_mb_scatter_kernel  (SCATTER) a block of 256 lanes per tile, row = 1024 tile + 256 j + lane for j = 0 .. 3, so that a
//       wave reads 64 consecutive bytes of `valid` and a lane's rank inside them is the population count of the ballot below
//       it (v_mbcnt); the sixteen (j, wave) totals meet in LDS after one barrier.  The eight keys (two Philox blocks), V, b
//       and the masks depend on the kernel's arguments and on count[0] alone: they are uniform, and the compiler keeps them
//       in scalar registers (checked in the assembly: s_mul_i32 / s_mul_hi_u32 chains before the first vector instruction).
//       A live lane then walks -- a divergent loop, under two applications of E on average -- and every row stores one
//       int64 at index[off_p + s].
// The scatter form (one lane per ROW, scattered 8-byte stores) is the one shipped; DESIGN.md section 4.24 says why the gather
// form (one lane per output slot, the inverse walk, a search of tile_base) was not built.
// What SCATTER reads from memory it does not trust: V is count[0] clamped to [0, rows], a live row whose rank is not below V
// and any row whose position is not below `rows` store nothing, so no workspace contents can form an address outside index
// or keep a walk from ending (a rank below V lies on a cycle of E that holds a value below V: itself).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_portable.h"  // philox4

#define WEDM_MB_BLOCK 256          // lanes of a COUNT / SCATTER block: a tile of WEDM_MB_TILE rows, four per lane
#define WEDM_MB_SCAN_BLOCK 1024    // lanes of the OFFSETS block: tile counts per pass

// the sum of a wave's 64 int32 (every lane must arrive; every lane returns it)
__device__ __forceinline__ int32_t wedm_mb_wave_sum(int32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// how many of a word's four bytes are not zero
__device__ __forceinline__ int32_t wedm_mb_nonzero_bytes(uint32_t x) {
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;   // bit 0 of every byte: the or of that byte's eight bits
    return __popc(x & 0x01010101u);
}

// The live rows among the four bytes from the 4-byte aligned address `word` that lie in [lo, hi): one load where all four do.
__device__ __forceinline__ int32_t wedm_mb_count_word(uintptr_t word, uintptr_t lo, uintptr_t hi) {
    if (word >= lo && word + 4 <= hi) return wedm_mb_nonzero_bytes(*(const uint32_t*)word);
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uintptr_t a = word + i;
        if (a >= lo && a < hi) c += *(const uint8_t*)a != 0;
    }
    return c;
}

__global__ void __launch_bounds__(WEDM_MB_BLOCK) wedm_mb_count_kernel(const wedm_mb_desc d) {
    __shared__ int32_t s_live[WEDM_MB_BLOCK / 64];
    const int32_t tid = (int32_t)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * WEDM_MB_TILE;
    const int32_t in_tile = (int32_t)min((int64_t)WEDM_MB_TILE, (int64_t)d.rows - row0);
    if (!d.valid) {  // (uniform) every row is live
        if (tid == 0) d.tile_counts[blockIdx.x] = in_tile;
        return;
    }
    const uintptr_t lo = (uintptr_t)d.valid + (uintptr_t)row0, hi = lo + (uintptr_t)in_tile;
    const uintptr_t word0 = lo & ~(uintptr_t)3;
    int32_t c = wedm_mb_count_word(word0 + 4u * (uint32_t)tid, lo, hi);
    if (tid == 0 && word0 != lo) c += wedm_mb_count_word(word0 + WEDM_MB_TILE, lo, hi);  // the 257th word of a tile that starts inside one
    c = wedm_mb_wave_sum(c);
    if ((tid & 63) == 0) s_live[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) d.tile_counts[blockIdx.x] = s_live[0] + s_live[1] + s_live[2] + s_live[3];
}

__global__ void __launch_bounds__(WEDM_MB_SCAN_BLOCK) wedm_mb_offsets_kernel(const wedm_mb_desc d, const int32_t tiles) {
    __shared__ int32_t s_wave[2][WEDM_MB_SCAN_BLOCK / 64];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int32_t carry = 0;  // the live rows of the passes before this one (at most 2^26: no overflow)
    for (int32_t t0 = 0, pass = 0; t0 < tiles; t0 += WEDM_MB_SCAN_BLOCK, pass ^= 1) {  // (uniform)
        const int32_t t = t0 + tid;
        const int32_t c = t < tiles ? d.tile_counts[t] : 0;
        int32_t incl = c;  // the wave's inclusive scan
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_wave[pass][w] = incl;
        __syncthreads();
        int32_t before = 0, all = 0;  // the waves before this lane's, and all sixteen
#pragma unroll
        for (int j = 0; j < WEDM_MB_SCAN_BLOCK / 64; ++j) {
            const int32_t v = s_wave[pass][j];
            all += v;
            before += j < w ? v : 0;
        }
        if (t < tiles) d.tile_base[t] = carry + before + (incl - c);
        carry += all;
    }
    if (tid == 0) {
        d.count[0] = carry;
        d.count[1] = (int64_t)d.rows - carry;
    }
}

__device__ __forceinline__ uint32_t wedm_mb_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// the keys and widths of a call's bijection: uniform
struct wedm_mb_cipher {
    uint32_t key[8];
    uint32_t hl, mask_lo, mask_hi;
};

__device__ __forceinline__ uint32_t wedm_mb_E(const wedm_mb_cipher& c, uint32_t x) {
    uint32_t lo = x & c.mask_lo, hi = x >> c.hl;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        hi ^= wedm_mb_mix(lo ^ c.key[i]) & c.mask_hi;
        lo ^= wedm_mb_mix(hi ^ c.key[i + 1]) & c.mask_lo;
    }
    return hi << c.hl | lo;
}

__global__ void __launch_bounds__(WEDM_MB_BLOCK) wedm_mb_scatter_kernel(const wedm_mb_desc d) {
    __shared__ int32_t s_live[4][WEDM_MB_BLOCK / 64];
    const int32_t tid = (int32_t)threadIdx.x, w = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * WEDM_MB_TILE;
    const int64_t rows = d.rows;
    // uniform: the live count, the widths, the keys
    const int64_t v_mem = d.count[0];
    const uint32_t V = (uint32_t)(v_mem < 0 ? 0 : v_mem > rows ? rows : v_mem);
    const uint32_t b = V <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(V - 1u);
    wedm_mb_cipher c;
    c.hl = b >> 1;
    c.mask_lo = (1u << c.hl) - 1u;
    c.mask_hi = (1u << (b - c.hl)) - 1u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const wedm::W4 k = wedm::philox4((uint32_t)d.seed, (uint32_t)(d.seed >> 32), (uint32_t)d.draw, (uint32_t)(d.draw >> 32),
                                         0u, WEDM_MB_STREAM0 + (uint32_t)q);
        c.key[4 * q] = k.x;
        c.key[4 * q + 1] = k.y;
        c.key[4 * q + 2] = k.z;
        c.key[4 * q + 3] = k.w;
    }
    // the ranks inside the tile: row = row0 + 256 j + tid
    bool live[4];
    int32_t rank[4];  // live rows of the same (j, wave) below this lane
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = row0 + j * WEDM_MB_BLOCK + tid;
        live[j] = r < rows && (!d.valid || d.valid[r] != 0);
        const unsigned long long bal = __ballot(live[j]);
        rank[j] = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if ((tid & 63) == 0) s_live[j][w] = __popcll(bal);
    }
    __syncthreads();
    const uint32_t n = (uint32_t)d.n_parts;
    const uint32_t per = (uint32_t)rows / n, extra = (uint32_t)rows % n;
    int32_t below = d.tile_base[blockIdx.x];  // live rows below (j, wave), which come in the rows' order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int32_t mine = 0, all = 0;
#pragma unroll
        for (int ww = 0; ww < WEDM_MB_BLOCK / 64; ++ww) {
            const int32_t here = s_live[j][ww];
            mine += ww < w ? here : 0;
            all += here;
        }
        const int64_t r = row0 + j * WEDM_MB_BLOCK + tid;
        const int64_t k = (int64_t)below + mine + rank[j];
        below += all;
        int64_t pos = -1;  // the list position, or nothing to store
        if (live[j]) {
            if (k >= 0 && k < (int64_t)V) {
                uint32_t x = (uint32_t)k;
                do x = wedm_mb_E(c, x);
                while (x >= V);
                pos = x;
            }
        } else if (r < rows) {
            pos = (int64_t)V + (r - k);
        }
        if (pos >= 0 && pos < rows) {
            const uint32_t p = (uint32_t)pos % n, s = (uint32_t)pos / n;
            d.index[(int64_t)p * per + min(p, extra) + s] = r;
        }
    }
}
