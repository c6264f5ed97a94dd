// wedm_profile.h -- wedm_wire_profile: every named environment's wire reduced to a profile, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  A pure read-reduce over the
// quad-interleaved wire block T[quad][stride][4]: quads * 16 B per environment in, (4 + 2 * bins) * 4 B out (the zone
// mean, the wire's mean, maximum and hottest cell, and per bin its maximum and mean; definitions in include/wedm_hip.h).
//
// Shape: a block is W waves (4, 8 or 16, chosen by the host) that all serve the SAME 64 output columns: lane l of every
// wave is column blockIdx.x * 64 + l, so a wave reads contiguous 1-KB runs of 16-byte words (with env_idx == NULL or an
// ascending list) and stores coalesced rows.  The wire's quads are split over the waves in contiguous runs of `chunk`
// quads -- one lane per environment over the whole wire would be one wave per SIMD at 65 536 x 128 -- and a wave loads
// WEDM_PROFILE_LOADS independent quads before it consumes the first.  Four, not wedm_copy.h's eight: the 32 cells of eight
// quads are unrolled with their float64 conversions hoisted, 142 / 151 VGPRs (three waves per SIMD, and spills under the
// 128 that a 16-wave block may have); four quads take 63 / 74 without scratch, eight or six waves per SIMD, so a SIMD has
// as many loads in flight from more waves.
// What makes the split legal is the header's exactness argument: every mean is a float64 sum of float32 cells that is
// exact, so partial sums combine in any order to the same bits.  They combine in LDS, [row][lane] so that no two lanes share
// a bank: float64 adds for the sums, unsigned maxima of an order-preserving key of the float for the maxima (a lane's own
// running maxima are plain floats; the key is formed where they meet other waves'), and for the
// hottest cell one 64-bit maximum of (key << 32 | ~index) -- the largest value, and among equals the lowest index.
// The bins: for n >= bins they partition the wire in order, so a lane carries ONE running bin (index, its end, sum, key)
// through its cells and adds it into LDS row [bin] when a cell index reaches the end -- no accumulator is indexed by a
// run-time bin number (registers so indexed go to scratch).  The bin of a wave's first cell is found by bisection over the
// bin edges (a multiply and a shift each, `edge` below), the next end follows from the last by the integer step of
// floor((b + 1) * n / bins) (quotient and remainder of n / bins, carried remainder): no division per bin.  For n < bins
// (at most 63 cells) a bin is one cell, read directly when the rows are written.
// PER_ENV = false: n, the zone and so every bin end are kernel arguments, c and the bin state are wave-uniform (scalar
// registers, uniform branches).  PER_ENV = true: they come from the geometry rows, per lane.
// Cells past n (the tail quad, cells up to n_seg_max of a shorter wire, the quads a short last batch of loads repeats) are
// masked by selects, never branched around; their values (NaN, anything) reach nothing.  Lanes that write nothing (past
// count, an index out of range, a bad n_seg) walk environment 0's column with n = 1 or the uniform n: in bounds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"

#ifndef WEDM_PROFILE_LOADS  // (-D: tools/build_variant.py, for measuring another choice)
#define WEDM_PROFILE_LOADS 4
#endif
#define WEDM_PROFILE_MAX_WAVES 16
#ifndef WEDM_PROFILE_WAVES_PER_SIMD  // what the host sizes a block for (wedm_wire_profile)
#define WEDM_PROFILE_WAVES_PER_SIMD 4
#endif
// LDS, in 8-byte words: zone sum, wire sum, hot word [64] each, then bins x 64 bin sums, then bins x 64 4-byte bin keys
#define WEDM_PROFILE_LDS_BYTES(bins) (8 * (192 + 64 * (bins)) + 4 * 64 * (bins))

typedef float wedm_f32x4 __attribute__((ext_vector_type(4)));

struct wedm_profile_args {
    wedm_profile_desc d;
    int32_t count;
    int32_t chunk;   // quads per wave: wave w walks quads [w * chunk, (w + 1) * chunk) of WEDM_T_QUADS(n_seg_max)
    uint32_t inv_b;  // ceil(2^20 / bins): x / bins == (x * inv_b) >> 20 for 0 <= x < 4096 (error x / 2^20 < 1 / 256 < 1 / bins)
};

// unsigned keys in the order of the floats (-inf < ... < -0 < +0 < ... < +inf); 0 is below every non-NaN float's key
__device__ __forceinline__ uint32_t wedm_profile_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float wedm_profile_unkey(uint32_t k) {
    return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}

template <bool PER_ENV>
__global__ void __launch_bounds__(WEDM_PROFILE_MAX_WAVES * 64)
wedm_wire_profile_kernel(const wedm_profile_args a, const int32_t* __restrict__ env_idx, int32_t* status) {
    extern __shared__ double wedm_profile_lds[];
    const wedm_profile_desc& d = a.d;
    const int32_t B = d.bins;
    double* const s_zone = wedm_profile_lds;
    double* const s_wire = wedm_profile_lds + 64;
    unsigned long long* const s_hot = (unsigned long long*)(wedm_profile_lds + 128);
    double* const s_bsum = wedm_profile_lds + 192;
    uint32_t* const s_bkey = (uint32_t*)(wedm_profile_lds + 192 + 64 * B);

    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int32_t w = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x >> 6), W = (int32_t)blockDim.x >> 6;
    {
        uint32_t* z = (uint32_t*)wedm_profile_lds;
        const int32_t words = WEDM_PROFILE_LDS_BYTES(B) / 4;
        for (int32_t k = (int32_t)threadIdx.x; k < words; k += (int32_t)blockDim.x) z[k] = 0u;
    }

    // ---- this lane's column, environment and geometry
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    bool ok = i < a.count;
    int32_t e = 0;
    if (ok) {
        e = env_idx ? env_idx[i] : (int32_t)i;
        if ((uint32_t)e >= (uint32_t)d.num_envs) {
            if (status && w == 0) atomicOr(status, 1);
            ok = false;
            e = 0;
        }
    }
    int32_t n = d.n_seg, zs = d.az_start, ze = d.az_end;
    if (PER_ENV) {
        const int32_t* g = d.geom_i32 + e;
        n = g[WEDM_GI_N_SEG * d.stride];
        zs = g[WEDM_GI_AZ_START * d.stride];
        ze = g[WEDM_GI_AZ_END * d.stride];
        if ((uint32_t)(n - 1) >= (uint32_t)d.n_seg_max) {
            if (ok && status && w == 0) atomicOr(status, 2);
            ok = false;
            n = 1;
        }
    }
    if (!(zs >= 0 && zs < ze && ze <= n)) zs = 0, ze = n;

    // ---- this wave's run of quads and the bin its first cell lies in
    const int32_t quads = WEDM_T_QUADS(d.n_seg_max);
    const int32_t q0 = w * a.chunk, q1 = min(q0 + a.chunk, quads);
    const int32_t c0 = q0 * 4, c_end = min(n, q1 * 4);
    int32_t bq = 0, br = 0;  // n = bq * B + br
    if (B > 0) {
        bq = (int32_t)((uint32_t)n / (uint32_t)B);
        br = n - bq * B;
    }
    // floor(k * n / B) for 0 <= k <= B without a division: k * bq + floor(k * br / B), and k * br <= 64 * 63 < 4096
    const auto edge = [&](int32_t k) { return k * bq + (int32_t)(((uint32_t)(k * br) * a.inv_b) >> 20); };
    // the running bin: cells [.., hi) belong to bin b, and (b + 1) * n = hi * B + rem.  b == B: no bin is being walked
    int32_t b = B, hi = INT32_MAX, rem = 0;
    if (B > 0 && n >= B && c0 < n) {
        b = 0;  // the largest b with floor(b * n / B) <= c0, by bisection over [0, B)
#pragma unroll
        for (int32_t step = WEDM_PROFILE_MAX_BINS / 2; step; step >>= 1) {
            const int32_t t = b + step;
            if (t < B && edge(t) <= c0) b = t;
        }
        hi = edge(b + 1);
        rem = (b + 1) * br - (hi - (b + 1) * bq) * B;
    }
    // (the maxima as floats here, as keys only where they meet other waves': a NaN cell loses every comparison)
    const float ninf = -__builtin_inff();
    double zone = 0.0, wire = 0.0, bsum = 0.0;  // bsum: the cells since the last flush, whether a bin is walked or not
    float bmax = ninf, wmax = ninf;
    int32_t widx = c0;
    __syncthreads();  // the LDS rows are zero

    const auto flush = [&]() {
        atomicAdd(&s_bsum[b * 64 + lane], bsum);
        atomicMax(&s_bkey[b * 64 + lane], wedm_profile_key(bmax));
    };
    const auto cell = [&](float v, int32_t c) {
        if (c == hi) {  // (uniform without PER_ENV) bin b is complete; b < B here, because hi <= n only while b < B
            flush();
            wire += bsum;
            bsum = 0.0, bmax = ninf;
            if (++b < B) {
                rem += br;
                hi += bq + (rem >= B ? 1 : 0);
                rem -= rem >= B ? B : 0;
            } else {
                hi = INT32_MAX;
            }
        }
        const bool live = c < c_end;
        const double x = (double)(live ? v : 0.0f);
        const float m = live ? v : ninf;
        bsum += x;
        zone += (c >= zs && c < ze) ? x : 0.0;
        bmax = fmaxf(bmax, m);
        if (m > wmax) wmax = m, widx = c;  // ascending c: the first of equals stays
    };

    const wedm_f32x4* Tq = (const wedm_f32x4*)d.T + e;
    for (int32_t q = q0; q < q1; q += WEDM_PROFILE_LOADS) {
        wedm_f32x4 v[WEDM_PROFILE_LOADS];
#pragma unroll
        for (int k = 0; k < WEDM_PROFILE_LOADS; ++k) v[k] = Tq[(int64_t)min(q + k, q1 - 1) * d.stride];  // (repeats: masked, c >= c_end)
#pragma unroll
        for (int k = 0; k < WEDM_PROFILE_LOADS; ++k) {
            const int32_t c = (q + k) * 4;
            cell(v[k].x, c);
            cell(v[k].y, c + 1);
            cell(v[k].z, c + 2);
            cell(v[k].w, c + 3);
        }
    }
    if (b < B) flush();
    atomicAdd(&s_zone[lane], zone);
    atomicAdd(&s_wire[lane], wire + bsum);
    atomicMax(&s_hot[lane], ((unsigned long long)wedm_profile_key(wmax) << 32) | (uint32_t)~(uint32_t)widx);
    __syncthreads();

    // ---- the rows: wave w writes rows w, w + W, ... of this block's 64 columns
    const int32_t rows = WEDM_PROFILE_ROWS(B);
    float* const out = d.out + i;
    for (int32_t r = w; r < rows; r += W) {
        float y;
        if (r == WEDM_PR_ZONE_MEAN) {
            y = (float)(s_zone[lane] / (double)(ze - zs));
        } else if (r == WEDM_PR_WIRE_MEAN) {
            y = (float)(s_wire[lane] / (double)n);
        } else if (r == WEDM_PR_WIRE_MAX) {
            y = wedm_profile_unkey((uint32_t)(s_hot[lane] >> 32));
        } else if (r == WEDM_PR_HOT_CELL) {
            y = (float)(~(uint32_t)s_hot[lane]);
        } else {
            const bool mean = r >= WEDM_PR_FIXED + B;
            const int32_t bb = r - WEDM_PR_FIXED - (mean ? B : 0);
            const int32_t lo = edge(bb);
            if (n >= B) {
                const int32_t up = edge(bb + 1);
                y = mean ? (float)(s_bsum[bb * 64 + lane] / (double)(up - lo)) : wedm_profile_unkey(s_bkey[bb * 64 + lane]);
            } else {  // one cell: its own maximum and mean
                y = d.T[WEDM_T_INDEX(lo, d.stride, e)];
            }
        }
        if (ok) out[(int64_t)r * d.out_stride] = y;
    }
}
