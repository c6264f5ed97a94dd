// wedm_reward.h -- wedm_reward: the shaped reward of a control step, ten weighted terms of the state blocks, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the ten
// terms and the rows they read -- the *_ACC rows, not the *_LAST ones --, live, the order of the additions, the single
// rounding to float32, the canonical NaN) is in include/wedm_hip.h and tests hold this kernel to it on every byte.
//
// One kernel, one lane per environment in blocks of 256, so that every row read and every store is one coalesced run along
// the environment index; plain vector loads and stores, no LDS, no atomic, no scratch.  The descriptor travels by value in
// the kernel arguments: weights and thresholds are scalar registers, "is this term on" is a wave-uniform scalar branch, and
// the row of a term that is off is never addressed (its block may be NULL).  The lane first issues every load the call
// needs -- they are independent, at most eleven -- and then forms the terms in ascending k: weight * x rounded, then the
// addition (-ffp-contract=off keeps them two roundings; there is no fma here).  Every offset is formed in 64 bits.  A lane
// past num_envs touches no memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"

#define WEDM_RW_BLOCK 256

// what the call stores for a float64 / as the float32 reward: a NaN in its one canonical form
__device__ __forceinline__ double wedm_rw_f64(double x) { return x != x ? __longlong_as_double(0x7FF8000000000000LL) : x; }
__device__ __forceinline__ float wedm_rw_f32(double x) { return x != x ? __uint_as_float(0x7FC00000u) : (float)x; }

__global__ void __launch_bounds__(WEDM_RW_BLOCK) wedm_reward_kernel(const wedm_reward_desc d) {
    const int64_t e = (int64_t)blockIdx.x * WEDM_RW_BLOCK + (int64_t)threadIdx.x;
    if (e >= d.num_envs) return;
    const int64_t S = d.stride;
    bool on[WEDM_RW_COUNT];  // (uniform: scalar compares of kernel arguments)
#pragma unroll
    for (int k = 0; k < WEDM_RW_COUNT; ++k) on[k] = d.weight[k] != 0.0;
    const bool live = !d.mask || d.mask[e] != 0;
    double x[WEDM_RW_COUNT];
#pragma unroll
    for (int k = 0; k < WEDM_RW_COUNT; ++k) x[k] = 0.0;
    if (live) {
        // the loads, all of them before the first use
        double pos = 0.0, p0 = 0.0, samples = 0.0, gap_min = 0.0, tmax_peak = 0.0;
        uint8_t restarted = 0;
        int8_t broken = 0, reached = 0;
        int32_t sparks = 0, shorts = 0, short_steps = 0;
        if (on[WEDM_RW_PROGRESS]) {
            pos = d.f64[(int64_t)WEDM_F_WORKPIECE_POS * S + e];
            p0 = d.pos_before[e];
            if (d.restart) restarted = d.restart[e];
        }
        if (on[WEDM_RW_WIRE_BREAK]) broken = d.i8[(int64_t)WEDM_B_WIRE_BROKEN * S + e];
        if (on[WEDM_RW_TARGET]) reached = d.i8[(int64_t)WEDM_B_TARGET_REACHED * S + e];
        if (on[WEDM_RW_SPARKS]) sparks = d.pulse[(int64_t)WEDM_P_SPARK_ACC * S + e];
        if (on[WEDM_RW_SHORTS]) shorts = d.pulse[(int64_t)WEDM_P_SHORT_ACC * S + e];
        if (on[WEDM_RW_SHORT_STEPS]) short_steps = d.pulse[(int64_t)WEDM_P_SHORT_STEPS_ACC * S + e];
        if (on[WEDM_RW_ENERGY]) x[WEDM_RW_ENERGY] = d.sig[(int64_t)WEDM_SG_ENERGY_ACC * S + e];
        if (on[WEDM_RW_GAP_BELOW] || on[WEDM_RW_TMAX_ABOVE]) samples = d.sig[(int64_t)WEDM_SG_SAMPLES_ACC * S + e];
        if (on[WEDM_RW_GAP_BELOW]) gap_min = d.sig[(int64_t)WEDM_SG_GAP_MIN_ACC * S + e];
        if (on[WEDM_RW_TMAX_ABOVE]) tmax_peak = d.sig[(int64_t)WEDM_SG_TMAX_PEAK_ACC * S + e];
        // x_k (a term that is off keeps 0.0 and is not used)
        x[WEDM_RW_PROGRESS] = pos - (restarted != 0 ? d.pos_restart : p0);
        x[WEDM_RW_STEP] = 1.0;
        x[WEDM_RW_WIRE_BREAK] = broken != 0 ? 1.0 : 0.0;
        x[WEDM_RW_TARGET] = reached != 0 ? 1.0 : 0.0;
        x[WEDM_RW_SPARKS] = (double)sparks;
        x[WEDM_RW_SHORTS] = (double)shorts;
        x[WEDM_RW_SHORT_STEPS] = (double)short_steps;
        x[WEDM_RW_GAP_BELOW] = (samples > 0.0 && d.gap_floor > gap_min) ? d.gap_floor - gap_min : 0.0;
        x[WEDM_RW_TMAX_ABOVE] = (samples > 0.0 && tmax_peak > d.tmax_ceiling) ? tmax_peak - d.tmax_ceiling : 0.0;
    }
    double r = 0.0;
    double* const terms = d.terms_out ? d.terms_out + e : nullptr;  // (uniform whether)
#pragma unroll
    for (int k = 0; k < WEDM_RW_COUNT; ++k) {
        double t = 0.0;
        if (on[k]) {  // (uniform)
            if (live) {
                t = d.weight[k] * x[k];
                r = r + t;
            }
        }
        if (terms) terms[(int64_t)k * d.terms_stride] = wedm_rw_f64(t);
    }
    d.reward_out[e] = wedm_rw_f32(r);
}
