// wedm_sensor.h -- wedm_sensor: what a machine measures of the observation -- delay, calibration error, noise, quantisation
// and saturation per channel -- on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the order
// of the stages, every rounding, the Philox counters of the calibration words and of the noise, the clamps of the table's
// integers, the canonical NaN) is in include/wedm_hip.h and tests hold this kernel to it on every byte.
//
// One kernel, one lane per environment in blocks of 256, so that every read and write of a struct-of-arrays block -- the
// source planes, the ring, the output -- is one coalesced run along the environment index.  The lane owns its environment's
// ring slot, pos and age: nothing is shared between lanes, so there is no LDS, no atomic and no waiting, and the bits cannot
// depend on the launch shape.  The channel loop's counter is wave-uniform and the table pointers are kernel arguments, so a
// channel's eight settings are scalar loads and "does this channel draw" is a scalar branch: a channel without calibration
// skips its Philox block, one without noise the polar method.  The only divergence is the polar method's retry (21 % of the
// attempts) and a delayed sample's ring slot.  A delayed sample (d_eff > 0) lies in a slot other than pos, written by an
// earlier call: the lane never reads what it wrote in this call.  Every offset is formed in 64 bits.  A lane past num_envs,
// or of an environment outside the mask, touches no memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_portable.h"

#define WEDM_SN_BLOCK 256

// source column s of [0, C_in): a row of plane 0 or, behind them, of plane 1 (s is wave-uniform: a scalar select)
__device__ __forceinline__ const float* wedm_sn_source(const wedm_sensor_desc& d, int32_t s) {
    const int32_t n0 = d.plane[0].n_rows;
    return s < n0 ? d.plane[0].rows + (int64_t)s * d.plane[0].stride : d.plane[1].rows + (int64_t)(s - n0) * d.plane[1].stride;
}

// `chan` and `route` are the descriptor's, passed beside it as restrict-qualified read-only arguments: that no store of the
// kernel can change the table is what lets the compiler keep its loads scalar.
__global__ void __launch_bounds__(WEDM_SN_BLOCK) wedm_sensor_kernel(const wedm_sensor_desc d, const double* __restrict__ chan,
                                                                    const int32_t* __restrict__ route) {
    const int64_t e = (int64_t)blockIdx.x * WEDM_SN_BLOCK + (int64_t)threadIdx.x;
    if (e >= d.num_envs) return;
    if (d.mask && d.mask[e] == 0) return;
    const int32_t L = d.ring_len, C_in = d.plane[0].n_rows + d.plane[1].n_rows, C_out = d.n_out;
    const uint32_t key0 = (uint32_t)d.seed, key1 = (uint32_t)(d.seed >> 32);
    const uint32_t t0 = (uint32_t)d.t, t1 = (uint32_t)(d.t >> 32);
    const uint32_t g = d.env_id_offset + (uint32_t)e;
    const uint64_t k = d.episode ? (uint64_t)d.episode[e] : 0u;
    const uint32_t k0 = (uint32_t)k, k1 = (uint32_t)(k >> 32);

    // 1. the episode's clock
    int32_t pos = 0, age = 0;
    if (d.first && d.first[e] == 0) {
        const int32_t p = d.pos[e], a = d.age[e];
        pos = (p < 0 ? 0 : p > L - 1 ? L - 1 : p) + 1;
        if (pos >= L) pos = 0;
        age = (a < 0 ? 0 : a > L - 1 ? L - 1 : a) + 1;
        if (age > L - 1) age = L - 1;
    }
    d.pos[e] = pos;
    d.age[e] = age;

    // 2. the newest sample of every source column into the ring
    const int64_t slot = (int64_t)C_in * d.ring_stride;  // elements of one ring slot
    if (L > 1) {
        float* const to = d.ring + (int64_t)pos * slot + e;
        for (int32_t s = 0; s < C_in; ++s) to[(int64_t)s * d.ring_stride] = wedm_sn_source(d, s)[e];
    }

    // 3. the channels (c, and with it everything read from the table, is wave-uniform)
    for (int32_t c = 0; c < C_out; ++c) {
        const double sigma = chan[(int64_t)WEDM_SN_SIGMA * C_out + c], gs = chan[(int64_t)WEDM_SN_GAIN_SPREAD * C_out + c];
        const double os = chan[(int64_t)WEDM_SN_OFFSET_SPREAD * C_out + c], lsb = chan[(int64_t)WEDM_SN_LSB * C_out + c];
        const double lo = chan[(int64_t)WEDM_SN_LO * C_out + c], hi = chan[(int64_t)WEDM_SN_HI * C_out + c];
        int32_t s = route[(int64_t)WEDM_SN_SOURCE * C_out + c], md = route[(int64_t)WEDM_SN_MAX_DELAY * C_out + c];
        s = s < 0 ? 0 : s > C_in - 1 ? C_in - 1 : s;
        md = md < 0 ? 0 : md > L - 1 ? L - 1 : md;
        const bool calibrated = gs != 0.0 || os != 0.0;
        double ua = 0.0, ub = 0.0;
        uint32_t delay = 0;
        if (calibrated || md != 0) {
            const wedm::W4 w = wedm::philox4(key0, key1, k0, k1, g, WEDM_SENSOR_STREAM0 + 0x100000u + (uint32_t)c);
            ua = wedm::u32_to_unit(w.x);
            ub = wedm::u32_to_unit(w.y);
            delay = (uint32_t)(((uint64_t)w.z * (uint64_t)(uint32_t)(md + 1)) >> 32);
        }
        const int32_t d_eff = (int32_t)delay < age ? (int32_t)delay : age;  // (delay <= md <= L - 1)
        float x;
        if (d_eff == 0) {
            x = wedm_sn_source(d, s)[e];
        } else {
            int32_t from = pos - d_eff;
            if (from < 0) from += L;
            x = d.ring[(int64_t)from * slot + (int64_t)s * d.ring_stride + e];
        }
        double y = (double)x;
        if (calibrated) {
            const double gain = 1.0 + gs * (2.0 * ua - 1.0);
            const double off = os * (2.0 * ub - 1.0);
            y = (y * gain) + off;
        }
        if (sigma != 0.0) y = y + sigma * wedm::philox_std_normal(key0, key1, t0, t1, g, WEDM_SENSOR_STREAM0 + 64u * (uint32_t)c);
        if (lsb > 0.0) y = lsb * rint(y / lsb);
        if (y < lo) y = lo;
        if (y > hi) y = hi;
        d.out[(int64_t)c * d.out_stride + e] = y != y ? __uint_as_float(0x7FC00000u) : (float)y;
    }
}
