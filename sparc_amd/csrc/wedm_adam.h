// wedm_adam.h -- wedm_adam: Adam with global-norm gradient clipping and a KL gate over one flat parameter block, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the tree of
// the squared gradient, the decision, the element's update with every rounding) is in include/wedm_hip.h and tests hold
// these kernels to it on every byte.  Nothing here waits for another block, nothing spins, nothing is launched
// cooperatively, there is no atomic; every value goes out through an ordinary store.
//
// Two forms, the same bytes in every block (partials included):
//   the phased form, at most three launches in this order on one stream:
//     wedm_adam_norm_kernel    (NORM) one block per tile of 256 elements: q = g * g, six shift levels in the wave (lower lane
//         on the left), two over the four waves' nodes through LDS; thread 0 stores partials[tile].
//     wedm_adam_decide_kernel  (DECIDE) one wave: the tiles' nodes into LDS, padded with +0.0 to a power of two, the tree
//         level by level (x[i] = x[i] + x[i + s] for i a multiple of 2 s: no node is read and written at one level), then
//         lane 0 decides and stores state and info.
//     wedm_adam_apply_kernel   (APPLY) one lane per element in blocks of 256; the four words of info it needs are read once
//         per block and handed round through LDS.  A call that is not applied stores nothing.
//   the one-block form, wedm_adam_one_kernel: one block of up to 1 024 lanes walks its tiles a pass of block-size elements at
//     a time (a wave holds a quarter of a tile: its node goes to LDS), forms and stores the tiles' nodes, runs the same tree
//     in LDS, decides in thread 0, passes a barrier and applies with the decision taken from LDS.
// A padding leaf is +0.0 and every real leaf is >= +0.0 or a NaN, so adding a padding changes no bit.
// Every index is formed from thread and block numbers and descriptor fields and compared with n before use.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_head.h"
#include "wedm_ppo.h"

#define WEDM_ADAM_BLOCK 256  // == WEDM_NORM_TILE: a block of the phased form is a tile
#define WEDM_ADAM_ONE_BLOCK 1024  // lanes of the one-block form at most
#define WEDM_ADAM_ONE_TILES ((WEDM_OPT_ONE_BLOCK_MAX + 255) / 256)  // tiles of the one-block form at most
static_assert(WEDM_ADAM_ONE_TILES <= 256, "the one-block form keeps four doubles per tile in LDS");

namespace wedm {

// what DECIDE hands to APPLY
struct adam_decision {
    double applied, c, bc1, bc2;
};

// the tree over the tile index in LDS: x[0 .. padded), padded a power of two; x[0] is the root after the last barrier
__device__ __forceinline__ void adam_tile_tree(double* const x, const int padded, const int tid, const int threads) {
    for (int s = 1; s < padded; s <<= 1) {
        __syncthreads();
        for (int i = tid * 2 * s; i < padded; i += threads * 2 * s) x[i] = x[i] + x[i + s];
    }
    __syncthreads();
}

// DECIDE of the header on the root S, by one thread: state and info are stored
__device__ __forceinline__ adam_decision adam_decide(const wedm_opt_desc& d, const double S) {
    const bool clip = (d.flags & WEDM_OPT_CLIP) != 0, gate = (d.flags & WEDM_OPT_KL_GATE) != 0;
    double latch = d.state[WEDM_OS_LATCH];
    if (d.flags & WEDM_OPT_NEW_UPDATE) latch = 0.0;
    const double klv = gate ? d.kl[0] : 0.0;
    if (gate && latch == 0.0 && !(klv <= d.kl_limit)) latch = 1.0;
    const bool finite = S < __longlong_as_double(0x7FF0000000000000LL);
    const double norm = sqrt(S);
    double c = 1.0;
    if (clip) {
        c = d.max_norm / (norm + 1e-6);
        if (!(c < 1.0)) c = 1.0;
    }
    double b1pow = d.state[WEDM_OS_B1POW], b2pow = d.state[WEDM_OS_B2POW], t = d.state[WEDM_OS_T];
    double skipped_nonfinite = d.state[WEDM_OS_SKIPPED_NONFINITE], skipped_kl = d.state[WEDM_OS_SKIPPED_KL];
    if (latch != 0.0) skipped_kl += 1.0;
    else if (!finite) skipped_nonfinite += 1.0;
    else {
        t += 1.0;
        b1pow = b1pow * d.beta1;
        b2pow = b2pow * d.beta2;
    }
    adam_decision r;
    r.applied = (latch == 0.0 && finite) ? 1.0 : 0.0;
    r.c = c;
    r.bc1 = 1.0 - b1pow;
    r.bc2 = 1.0 - b2pow;
    d.state[WEDM_OS_B1POW] = ppo_f64(b1pow);
    d.state[WEDM_OS_B2POW] = ppo_f64(b2pow);
    d.state[WEDM_OS_T] = ppo_f64(t);
    d.state[WEDM_OS_SKIPPED_NONFINITE] = ppo_f64(skipped_nonfinite);
    d.state[WEDM_OS_SKIPPED_KL] = ppo_f64(skipped_kl);
    d.state[WEDM_OS_LATCH] = ppo_f64(latch);
    d.state[6] = 0.0;
    d.state[7] = 0.0;
    d.info[WEDM_OI_SUMSQ] = ppo_f64(S);
    d.info[WEDM_OI_NORM] = ppo_f64(norm);
    d.info[WEDM_OI_SCALE] = ppo_f64(c);
    d.info[WEDM_OI_LR] = ppo_f64(d.lr);
    d.info[WEDM_OI_APPLIED] = r.applied;
    d.info[WEDM_OI_KL] = ppo_f64(klv);
    d.info[WEDM_OI_BC1] = ppo_f64(r.bc1);
    d.info[WEDM_OI_BC2] = ppo_f64(r.bc2);
    return r;
}

// APPLY of the header on element e < n
__device__ __forceinline__ void adam_apply_element(const wedm_opt_desc& d, const int32_t e, const double c, const double bc1,
                                                   const double bc2) {
    const double g = (double)d.grad[e] * c;
    double p = (double)d.theta[e];
    if (d.weight_decay != 0.0) p = p - (d.lr * d.weight_decay) * p;  // (uniform)
    const float mf = head_f32(d.beta1 * (double)d.m[e] + (1.0 - d.beta1) * g);
    const float vf = head_f32(d.beta2 * (double)d.v[e] + (1.0 - d.beta2) * (g * g));
    const double mh = (double)mf / bc1, vh = (double)vf / bc2;
    p = p - d.lr * (mh / (sqrt(vh) + d.eps));
    d.theta[e] = head_f32(p);
    d.m[e] = mf;
    d.v[e] = vf;
}

}  // namespace wedm

__global__ void __launch_bounds__(WEDM_ADAM_BLOCK) wedm_adam_norm_kernel(const wedm_opt_desc d) {
    using namespace wedm;
    __shared__ double s_node[4];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t e = (int64_t)blockIdx.x * WEDM_ADAM_BLOCK + tid;
    const double g = e < d.n ? (double)d.grad[e] : 0.0;
    const double node = ppo_wave_sum(g * g);
    if (lane == 0) s_node[wv] = node;
    __syncthreads();
    if (tid == 0) d.partials[blockIdx.x] = ppo_f64((s_node[0] + s_node[1]) + (s_node[2] + s_node[3]));
}

// tiles: ceil(n / 256); padded: the smallest power of two >= tiles
__global__ void __launch_bounds__(64) wedm_adam_decide_kernel(const wedm_opt_desc d, const int32_t tiles, const int32_t padded) {
    using namespace wedm;
    __shared__ double s_x[WEDM_NORM_MAX_TILES];
    const int32_t tid = (int32_t)threadIdx.x;
    for (int32_t t = tid; t < padded; t += 64) s_x[t] = t < tiles ? d.partials[t] : 0.0;
    adam_tile_tree(s_x, padded, tid, 64);
    if (tid == 0) adam_decide(d, s_x[0]);
}

__global__ void __launch_bounds__(WEDM_ADAM_BLOCK) wedm_adam_apply_kernel(const wedm_opt_desc d) {
    using namespace wedm;
    __shared__ double s_info[4];
    const int32_t tid = (int32_t)threadIdx.x;
    if (tid < 4) s_info[tid] = d.info[tid == 0 ? WEDM_OI_APPLIED : (tid == 1 ? WEDM_OI_SCALE : (tid == 2 ? WEDM_OI_BC1 : WEDM_OI_BC2))];
    __syncthreads();
    if (!(s_info[0] == 1.0)) return;
    const int64_t e = (int64_t)blockIdx.x * WEDM_ADAM_BLOCK + tid;
    if (e < d.n) adam_apply_element(d, (int32_t)e, s_info[1], s_info[2], s_info[3]);
}

// one block of 256, 512, 768 or 1 024 lanes; tiles <= WEDM_ADAM_ONE_TILES
__global__ void __launch_bounds__(WEDM_ADAM_ONE_BLOCK) wedm_adam_one_kernel(const wedm_opt_desc d, const int32_t tiles, const int32_t padded) {
    using namespace wedm;
    __shared__ double s_quarter[4 * WEDM_ADAM_ONE_TILES];
    __shared__ double s_x[WEDM_ADAM_ONE_TILES];
    __shared__ double s_info[4];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, threads = (int32_t)blockDim.x;
    const int32_t span = tiles * WEDM_ADAM_BLOCK;  // the elements with their padding
    for (int32_t base = 0; base < span; base += threads) {  // (uniform: every lane of a wave takes every shift)
        const int32_t e = base + tid;
        const double g = e < d.n ? (double)d.grad[e] : 0.0;
        const double node = ppo_wave_sum(g * g);
        if (lane == 0 && e < span) s_quarter[e >> 6] = node;
    }
    __syncthreads();
    for (int32_t t = tid; t < padded; t += threads) {
        double node = 0.0;
        if (t < tiles) {
            node = (s_quarter[4 * t] + s_quarter[4 * t + 1]) + (s_quarter[4 * t + 2] + s_quarter[4 * t + 3]);
            d.partials[t] = ppo_f64(node);
        }
        s_x[t] = node;
    }
    adam_tile_tree(s_x, padded, tid, threads);
    if (tid == 0) {
        const adam_decision r = adam_decide(d, s_x[0]);
        s_info[0] = r.applied;
        s_info[1] = r.c;
        s_info[2] = r.bc1;
        s_info[3] = r.bc2;
    }
    __syncthreads();
    if (!(s_info[0] == 1.0)) return;
    const double c = s_info[1], bc1 = s_info[2], bc2 = s_info[3];
    for (int32_t e = tid; e < d.n; e += threads) adam_apply_element(d, e, c, bc1, bc2);
}
