// wedm_head.h -- wedm_policy_head: a policy's action head on the device -- sample, log-probability and entropy, gradient.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (four
// tanh-squashed Gaussians mapped to bounds and a categorical over listed modes, float64 with every rounding, the Philox
// streams of a draw, where a NaN goes) is in include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// One kernel template, one launch per call, one lane per row in blocks of 256; no block waits for another, nothing spins,
// nothing is launched cooperatively, no atomic exists here.
//   rows   A row-major [rows][P] block read lane-per-row puts 64 addresses 4 P bytes apart into every load instruction.
//       When the stride is P and the base is 16-byte aligned (IN_LDS), the block's 256 P contiguous floats go through LDS:
//       16-byte loads by consecutive lanes, written to LDS rows of P | 1 words -- an odd pitch, so that the 32 lanes of a
//       ds_read_b32 group, each reading word c of its own row, hit 32 banks -- and each lane then reads its row from LDS.
//       BACKWARD writes grad_params back the same way (OUT_LDS), through the same LDS rows: a lane overwrites word c of
//       its own row only after it has read it for the last time.  With a larger stride or an unaligned base the lanes
//       load and store directly.  The tail block stages the floats of the rows it has, never one past them.
//   u, mode_index, the action leaves, log_prob, entropy, the upstream gradients are indexed by the row: coalesced as they
//       are, u as one 16-byte access per lane.
//   the softmax  M is a kernel argument, so the loops over the logits are wave-uniform.  w_j = exp(l_j - m) is needed
//       twice by BACKWARD (in W, then in p_j).  It KEEPS them (KEEP below): an array indexed by a loop counter would
//       live in scratch, so both passes are unrolled over all 19 possible logits under the uniform j < M, every index is
//       a constant and the 19 doubles are registers -- 86 VGPRs and no scratch, against 101 for the form that computes
//       them again (DESIGN.md section 4.17 has both measured: keeping saves a quarter of BACKWARD at M = 9).  Either way
//       the bits are the same.  EVALUATE needs each w_j once; a draw's search computes them again (one row per environment).
//   divergence  the polar method's rejection loop, the early exit of a draw's search and the branches of portable_exp
//       diverge per lane; that is accepted (the search and the rejection are SAMPLE's, one row per environment).
// Every index is formed from thread and block numbers and descriptor fields alone; the one index that comes from data,
// mode_index[r], is clamped to [0, M - 1] before it is used.  A NaN or an infinity in a row reaches numbers only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_portable.h"

#define WEDM_HEAD_BLOCK 256

namespace wedm {

constexpr double HEAD_LN2 = 0.6931471805599453, HEAD_HALF_LOG_2PI = 0.9189385332046727, HEAD_HALF_LOG_2PIE = 1.4189385332046727;

// portable_log reads its argument's bits: a NaN stays the NaN it is
__device__ __forceinline__ double head_log(double x) { return x != x ? x : portable_log(x); }

// every float32 the call stores: a NaN carries no sign or payload of the operation that made it
__device__ __forceinline__ float head_f32(double x) { return x != x ? __uint_as_float(0x7FC00000u) : (float)x; }

// words of an LDS row of P floats: odd (the launch sizes the dynamic LDS by it)
__host__ __device__ __forceinline__ constexpr int head_pitch(int P) { return P | 1; }

// what the continuous component i makes of (mu, ls, sigma = exp(ls), u)
struct head_component {
    double z, action, c;
};

// Desc: a descriptor with lo[4], hi[4] and log_span[4] (wedm_head_desc; wedm_ppo_desc of wedm_ppo.h)
template <class Desc>
__device__ __forceinline__ head_component head_continuous(const Desc& d, const int i, const double mu, const double ls,
                                                          const double sigma, const double u) {
    head_component out;
    out.z = (u - mu) / sigma;
    const double a = __builtin_fabs(u);
    const double e = portable_exp(-2.0 * a);
    const double s = u >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    double x = d.lo[i] + (d.hi[i] - d.lo[i]) * s;
    x = x > d.lo[i] ? x : d.lo[i];
    out.action = x < d.hi[i] ? x : d.hi[i];
    const double logjac = ((d.log_span[i] + HEAD_LN2) - 2.0 * a) - 2.0 * head_log(1.0 + e);
    out.c = (((-0.5 * out.z) * out.z - ls) - HEAD_HALF_LOG_2PI) - logjac;
    return out;
}

// the categorical's row statistics
struct head_softmax {
    double m, W, logW, H;
};

// KEEP: also leaves w_j in `kept` -- a loop unrolled over all WEDM_HEAD_MAX_MODES under the uniform j < M, so that every index
// is a constant and the array lives in registers; the operations and their order are the same
template <bool KEEP>
__device__ __forceinline__ head_softmax head_mode_stats(const float* l, const int M, double (&kept)[KEEP ? WEDM_HEAD_MAX_MODES : 1]) {
    head_softmax s;
    s.m = (double)l[0];
    for (int j = 1; j < M; ++j) {
        const double lj = (double)l[j];
        s.m = lj > s.m ? lj : s.m;
    }
    double S = 0.0;
    s.W = 0.0;
    if (KEEP) {
#pragma unroll
        for (int j = 0; j < WEDM_HEAD_MAX_MODES; ++j) {
            if (j < M) {
                const double dj = (double)l[j] - s.m;
                const double w = portable_exp(dj);
                kept[KEEP ? j : 0] = w;
                s.W = s.W + w;
                S = S + w * dj;
            }
        }
    } else {
        for (int j = 0; j < M; ++j) {
            const double dj = (double)l[j] - s.m;
            const double w = portable_exp(dj);
            s.W = s.W + w;
            S = S + w * dj;
        }
    }
    s.logW = head_log(s.W);
    s.H = s.logW - S / s.W;
    return s;
}

__device__ __forceinline__ double head_entropy(const double ls[4], const double H) {
    return ((((ls[0] + HEAD_HALF_LOG_2PIE) + (ls[1] + HEAD_HALF_LOG_2PIE)) + (ls[2] + HEAD_HALF_LOG_2PIE)) +
            (ls[3] + HEAD_HALF_LOG_2PIE)) + H;
}

// the block's n contiguous floats (rows of P) from global memory into LDS rows of `pitch` words; src is 16-byte aligned
__device__ __forceinline__ void head_stage_in(const float* __restrict__ src, float* lds, const int n, const int P, const int pitch) {
    const int n4 = n >> 2;
    for (int i = (int)threadIdx.x; i < n4; i += WEDM_HEAD_BLOCK) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        const float x[4] = {v.x, v.y, v.z, v.w};
        int row = (4 * i) / P, col = 4 * i - row * P;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lds[row * pitch + col] = x[q];
            if (++col == P) {
                col = 0;
                ++row;
            }
        }
    }
    for (int f = 4 * n4 + (int)threadIdx.x; f < n; f += WEDM_HEAD_BLOCK) {  // (the tail block's last one to three floats)
        const int row = f / P;
        lds[row * pitch + (f - row * P)] = src[f];
    }
}

// the inverse: LDS rows of `pitch` words into the block's n contiguous floats; dst is 16-byte aligned
__device__ __forceinline__ void head_stage_out(float* __restrict__ dst, const float* lds, const int n, const int P, const int pitch) {
    const int n4 = n >> 2;
    for (int i = (int)threadIdx.x; i < n4; i += WEDM_HEAD_BLOCK) {
        float x[4];
        int row = (4 * i) / P, col = 4 * i - row * P;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = lds[row * pitch + col];
            if (++col == P) {
                col = 0;
                ++row;
            }
        }
        reinterpret_cast<float4*>(dst)[i] = make_float4(x[0], x[1], x[2], x[3]);
    }
    for (int f = 4 * n4 + (int)threadIdx.x; f < n; f += WEDM_HEAD_BLOCK) {
        const int row = f / P;
        dst[f] = lds[row * pitch + (f - row * P)];
    }
}

}  // namespace wedm

// OP: enum wedm_head_op.  IN_LDS: params go through LDS (param_stride == P, 16-byte aligned); OUT_LDS (BACKWARD): grad_params
// does (grad_stride == P, 16-byte aligned).  Dynamic LDS: 256 * (P | 1) floats when either is set, else none.
template <int OP, bool IN_LDS, bool OUT_LDS>
__global__ void __launch_bounds__(WEDM_HEAD_BLOCK) wedm_head_kernel(const wedm_head_desc d) {
    using namespace wedm;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int M = d.n_modes, P = 8 + M, pitch = head_pitch(P), tid = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * WEDM_HEAD_BLOCK, r = r0 + tid;
    const int here = (int)(d.rows - r0 < WEDM_HEAD_BLOCK ? d.rows - r0 : WEDM_HEAD_BLOCK);  // rows of this block
    const bool in = tid < here;
    if (IN_LDS) {
        head_stage_in(d.params + r0 * P, lds, here * P, P, pitch);
        __syncthreads();
    }
    if (in) {
        const float* const row = IN_LDS ? lds + tid * pitch : d.params + r * d.param_stride;
        const float* const l = row + 8;
        float* const grow = OUT_LDS ? lds + tid * pitch : d.grad_params + r * d.grad_stride;  // (BACKWARD only)
        double mu[4], ls[4], sigma[4], u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mu[i] = (double)row[i];
            ls[i] = (double)row[4 + i];
            sigma[i] = portable_exp(ls[i]);
        }
        int k = 0;
        if (OP == WEDM_HEAD_SAMPLE) {
            const uint32_t gid = d.env_id_offset + (uint32_t)r;
            const uint32_t key0 = (uint32_t)d.seed, key1 = (uint32_t)(d.seed >> 32), t0 = (uint32_t)d.t, t1 = (uint32_t)(d.t >> 32);
            const bool draw = !(d.flags & WEDM_HEAD_DETERMINISTIC);  // (uniform)
            float uf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uf[i] = (float)mu[i];
                if (draw) uf[i] = head_f32(mu[i] + sigma[i] * philox_std_normal(key0, key1, t0, t1, gid, WEDM_HEAD_STREAM0 + 64u * i));
                u[i] = (double)uf[i];
            }
            reinterpret_cast<float4*>(d.u)[r] = make_float4(uf[0], uf[1], uf[2], uf[3]);
        } else {
            const float4 v = reinterpret_cast<const float4*>(d.u)[r];
            u[0] = (double)v.x, u[1] = (double)v.y, u[2] = (double)v.z, u[3] = (double)v.w;
            k = d.mode_index[r];
            k = k < 0 ? 0 : (k > M - 1 ? M - 1 : k);
        }
        head_component c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = head_continuous(d, i, mu[i], ls[i], sigma[i], u[i]);
        constexpr bool KEEP = OP == WEDM_HEAD_BACKWARD;  // BACKWARD keeps w_j = exp(l_j - m) in registers between its two passes
        double w[KEEP ? WEDM_HEAD_MAX_MODES : 1];
        const head_softmax s = head_mode_stats<KEEP>(l, M, w);
        if (OP == WEDM_HEAD_SAMPLE) {
            if (d.flags & WEDM_HEAD_DETERMINISTIC) {  // (uniform) the first largest logit
                k = 0;
                double best = (double)l[0];
                for (int j = 1; j < M; ++j) {
                    const double lj = (double)l[j];
                    if (lj > best) {
                        best = lj;
                        k = j;
                    }
                }
            } else {
                const uint32_t gid = d.env_id_offset + (uint32_t)r;
                const W4 w = philox4((uint32_t)d.seed, (uint32_t)(d.seed >> 32), (uint32_t)d.t, (uint32_t)(d.t >> 32), gid,
                                     WEDM_HEAD_STREAM0 + 256u);
                const double tau = u32_to_unit(w.x) * s.W;
                double run = 0.0;
                k = M - 1;
                for (int j = 0; j < M; ++j) {
                    run = run + portable_exp((double)l[j] - s.m);
                    if (run > tau) {
                        k = j;
                        break;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) d.action[i][r] = c[i].action;
            int32_t mode = d.modes[0];  // (a select chain: an array in kernel-argument memory takes no per-lane index)
#pragma unroll
            for (int j = 1; j < WEDM_HEAD_MAX_MODES; ++j) mode = j == k ? d.modes[j] : mode;
            d.current_mode[r] = mode;
            d.mode_index[r] = k;
        }
        if (OP != WEDM_HEAD_BACKWARD) {
            const double logp_k = ((double)l[k] - s.m) - s.logW;
            d.log_prob[r] = head_f32((((c[0].c + c[1].c) + c[2].c) + c[3].c) + logp_k);
            d.entropy[r] = head_f32(head_entropy(ls, s.H));
        } else {
            const double glp = (double)d.g_log_prob[r], gen = d.g_entropy ? (double)d.g_entropy[r] : 0.0;
            // (word 8 + j of an LDS row is read here for the last time, then written)
            const auto logit_gradient = [&](const int j, const double wj) {
                const double p = wj / s.W, logp = ((double)l[j] - s.m) - s.logW;
                grow[8 + j] = head_f32(glp * ((j == k ? 1.0 : 0.0) - p) - gen * (p * (logp + s.H)));
            };
            if (KEEP) {
#pragma unroll
                for (int j = 0; j < WEDM_HEAD_MAX_MODES; ++j)
                    if (j < M) logit_gradient(j, w[KEEP ? j : 0]);
            } else {
                for (int j = 0; j < M; ++j) logit_gradient(j, portable_exp((double)l[j] - s.m));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                grow[i] = head_f32(glp * (c[i].z / sigma[i]));
                grow[4 + i] = head_f32(glp * (c[i].z * c[i].z - 1.0) + gen);
            }
        }
    }
    if (OP == WEDM_HEAD_BACKWARD && OUT_LDS) {
        __syncthreads();
        head_stage_out(d.grad_params + r0 * P, lds, here * P, P, pitch);
    }
}
