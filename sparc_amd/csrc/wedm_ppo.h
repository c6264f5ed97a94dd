// wedm_ppo.h -- wedm_ppo_loss: PPO's clipped loss, its statistics and its gradient over a minibatch, on the device.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the row's
// terms with every rounding, which rows are live, the pairwise tree over the row number, the gradient) is in
// include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// Up to four launches in this order on one stream, so that the only synchronisation is the stream's own -- no block ever
// waits for another block, nothing spins, nothing is launched cooperatively, no floating-point atomic exists here:
//   wedm_ppo_zero_kernel / wedm_ppo_count_kernel  (COUNT, only with valid or index) the number of live rows has to be known
//       before a gradient is scaled by 1 / n.  A few hundred blocks stride over the rows, count in registers, add up in
//       the wave and through LDS, and issue one integer atomic per block and counter: integers add in any order.
//   wedm_ppo_main_kernel  (MAIN) one lane per row in blocks of 256, a block is one tile of the tree.  The head's row goes
//       through the head's LDS staging in (IN_LDS) and the gradient row out (OUT_LDS) when stride and alignment allow, through
//       the same LDS rows; otherwise the lanes load and store directly.  The stored inputs are read at src = index[r]: a
//       gather of 4- and 16-byte elements, left plain.  The distribution is evaluated once: w_j = exp(l_j - m) stay in
//       registers between the softmax and the logits' gradient (the unrolled j < M of wedm_head.h).  The row's seven
//       summands go through six shift levels in the wave (lower lane on the left) and two through LDS over the four waves;
//       thread 0 stores partials[tile].  A lane without a live row skips the arithmetic, holds zeros and takes every shift.
//   wedm_ppo_fold_kernel  (FOLD) one block: the pairwise tree over the tile index, padded to the smallest power of two that
//       holds the tiles.  Lane i takes tiles [per i, per (i + 1)) as a tree in registers, the 256 lanes' nodes go through
//       six shift levels and two through LDS.  A node whose right child starts at or past the padded length is its left
//       child unchanged (adding the +0.0 of a padding that the definition does not have would turn a -0.0 into +0.0).
//       Thread 0 forms the means and the loss and stores stats.
// Every index is formed from thread and block numbers and descriptor fields, or from index[r] after it has been compared
// with [0, n_src); mode_index[src] is clamped before use.  A NaN or an infinity in a row reaches numbers only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wedm_hip.h"
#include "wedm_head.h"

#define WEDM_PPO_BLOCK 256  // == WEDM_NORM_TILE: a block is a tile
#define WEDM_PPO_COUNT_BLOCKS 256  // blocks of the count kernel at most
#define WEDM_PPO_FOLD_PER 16  // tiles per lane of the fold at most: 256 * 16 = WEDM_NORM_MAX_TILES

namespace wedm {

// every float64 the call stores: a NaN carries no sign or payload of the operation that made it
__device__ __forceinline__ double ppo_f64(double x) { return x != x ? __longlong_as_double(0x7FF8000000000000LL) : x; }

// where row r's stored inputs lie and whether the row is live; bad: src outside [0, n_src), which is never dereferenced
__device__ __forceinline__ bool ppo_row(const wedm_ppo_desc& d, const int64_t r, int64_t& src, bool& bad) {
    src = d.index ? d.index[r] : r;
    bad = src < 0 || src >= d.n_src;
    if (bad) return false;
    return !d.valid || d.valid[src] != 0;
}

// six tree levels of plain additions over the 64 lanes of a wave, lower lane on the left; the wave's node is lane 0's
__device__ __forceinline__ double ppo_wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_down(v, off);
    return v;
}

}  // namespace wedm

__global__ void __launch_bounds__(64) wedm_ppo_zero_kernel(const wedm_ppo_desc d) {
    if (threadIdx.x < WEDM_PPO_COUNT_WORDS) d.count[threadIdx.x] = 0;
}

// at most WEDM_PPO_COUNT_BLOCKS blocks stride over the rows: two atomics per block on the two words, a few hundred in all
// (one per wave of one block per tile was 16 384 on one address at 1 048 576 rows, and 187 us)
__global__ void __launch_bounds__(WEDM_PPO_BLOCK) wedm_ppo_count_kernel(const wedm_ppo_desc d) {
    __shared__ int32_t s_count[4][2];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t n_live = 0, n_bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * WEDM_PPO_BLOCK + tid; r < d.rows; r += (int64_t)gridDim.x * WEDM_PPO_BLOCK) {
        int64_t src;
        bool bad;
        n_live += wedm::ppo_row(d, r, src, bad) ? 1 : 0;
        n_bad += bad ? 1 : 0;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        n_live += __shfl_down(n_live, off);
        n_bad += __shfl_down(n_bad, off);
    }
    if (lane == 0) {
        s_count[wv][0] = n_live;
        s_count[wv][1] = n_bad;
    }
    __syncthreads();
    if (tid < 2) {
        const int32_t n = (s_count[0][tid] + s_count[1][tid]) + (s_count[2][tid] + s_count[3][tid]);
        if (n) atomicAdd(d.count + tid, n);
    }
}

// n_known: the number of live rows where the host knows it (no valid, no index: rows), else -1: count[0] holds it.
// Dynamic LDS: 256 * (P | 1) floats when IN_LDS or OUT_LDS, else none.
template <bool IN_LDS, bool OUT_LDS>
__global__ void __launch_bounds__(WEDM_PPO_BLOCK) wedm_ppo_main_kernel(const wedm_ppo_desc d, const int32_t n_known) {
    using namespace wedm;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double s_node[4][WEDM_PPO_SUMS];
    const int M = d.n_modes, P = 8 + M, pitch = head_pitch(P), tid = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * WEDM_PPO_BLOCK, r = r0 + tid;
    const int here = (int)(d.rows - r0 < WEDM_PPO_BLOCK ? d.rows - r0 : WEDM_PPO_BLOCK);  // rows of this block
    const bool in = tid < here;
    const bool clip_value = (d.flags & WEDM_PPO_CLIP_VALUE) != 0, want_gp = d.grad_params != nullptr, want_gv = d.grad_value != nullptr;
    const int32_t n = n_known >= 0 ? n_known : d.count[0];
    const double scale = n > 0 ? 1.0 / (double)n : 0.0;  // the s of the definition
    if (IN_LDS) {
        head_stage_in(d.params + r0 * P, lds, here * P, P, pitch);
        __syncthreads();
    }
    double sum[WEDM_PPO_SUMS];
#pragma unroll
    for (int c = 0; c < WEDM_PPO_SUMS; ++c) sum[c] = 0.0;
    if (in) {
        int64_t src;
        bool bad;
        const bool live = ppo_row(d, r, src, bad);
        sum[WEDM_PS_BAD] = bad ? 1.0 : 0.0;
        float* const grow = OUT_LDS ? lds + tid * pitch : d.grad_params + r * d.grad_stride;
        if (live) {
            const float* const row = IN_LDS ? lds + tid * pitch : d.params + r * d.param_stride;
            const float* const l = row + 8;
            double mu[4], ls[4], sigma[4], u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                mu[i] = (double)row[i];
                ls[i] = (double)row[4 + i];
                sigma[i] = portable_exp(ls[i]);
            }
            const float4 uf = reinterpret_cast<const float4*>(d.u)[src];
            u[0] = (double)uf.x, u[1] = (double)uf.y, u[2] = (double)uf.z, u[3] = (double)uf.w;
            int k = d.mode_index[src];
            k = k < 0 ? 0 : (k > M - 1 ? M - 1 : k);
            const double old = (double)d.old_log_prob[src], A = (double)d.advantage[src], R = (double)d.returns[src];
            const double v = (double)d.value[r];
            head_component c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = head_continuous(d, i, mu[i], ls[i], sigma[i], u[i]);
            double w[WEDM_HEAD_MAX_MODES];
            const head_softmax s = head_mode_stats<true>(l, M, w);
            const double lp64 = (((c[0].c + c[1].c) + c[2].c) + c[3].c) + (((double)l[k] - s.m) - s.logW);
            const double ent64 = head_entropy(ls, s.H);
            // the policy term
            const double lp = (double)head_f32(lp64);
            const double lr = lp - old;
            const double ratio = portable_exp(lr);
            const double lo_c = 1.0 - d.clip, hi_c = 1.0 + d.clip;
            const double rc = ratio < lo_c ? lo_c : (ratio > hi_c ? hi_c : ratio);
            const double s1 = ratio * A, s2 = rc * A;
            const bool clipped = s2 < s1;
            const double pol = -(clipped ? s2 : s1);
            const double dlp = clipped ? 0.0 : -(A * ratio);
            const double kl = (ratio - 1.0) - lr;
            const double cf = (ratio < lo_c || ratio > hi_c) ? 1.0 : 0.0;
            // the value term
            const double e = v - R;
            double vl = e * e, dv = e;
            if (clip_value) {  // (uniform)
                const double ov = (double)d.old_value[src];
                const double dd = v - ov;
                const double dc = dd < -d.clip_value ? -d.clip_value : (dd > d.clip_value ? d.clip_value : dd);
                const double ec = (ov + dc) - R;
                const double vlc = ec * ec;
                if (vlc > vl) {
                    vl = vlc;
                    dv = dc == dd ? ec : 0.0;
                }
            }
            sum[WEDM_PS_LIVE] = 1.0;
            sum[WEDM_PS_POLICY] = pol;
            sum[WEDM_PS_VALUE] = 0.5 * vl;
            sum[WEDM_PS_ENTROPY] = ent64;
            sum[WEDM_PS_KL] = kl;
            sum[WEDM_PS_CLIPPED] = cf;
            if (want_gv) d.grad_value[r] = head_f32((d.vf_coef * dv) * scale);
            if (want_gp) {  // (uniform) WEDM_HEAD_BACKWARD's formulas; word j of an LDS row is read for the last time, then written
                const double glp = dlp * scale, gen = -d.ent_coef * scale;
#pragma unroll
                for (int j = 0; j < WEDM_HEAD_MAX_MODES; ++j) {
                    if (j < M) {
                        const double p = w[j] / s.W, logp = ((double)l[j] - s.m) - s.logW;
                        grow[8 + j] = head_f32(glp * ((j == k ? 1.0 : 0.0) - p) - gen * (p * (logp + s.H)));
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    grow[i] = head_f32(glp * (c[i].z / sigma[i]));
                    grow[4 + i] = head_f32(glp * (c[i].z * c[i].z - 1.0) + gen);
                }
            }
        } else {
            if (want_gv) d.grad_value[r] = 0.0f;
            if (want_gp)
                for (int j = 0; j < P; ++j) grow[j] = 0.0f;
        }
    }
    // the tile's tree: six levels in the wave, two over the waves' nodes
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int c = 0; c < WEDM_PPO_SUMS; ++c) {
        const double node = ppo_wave_sum(sum[c]);
        if (lane == 0) s_node[wv][c] = node;
    }
    __syncthreads();
    if (tid < WEDM_PPO_SUMS)
        d.partials[(int64_t)blockIdx.x * WEDM_PPO_SUMS + tid] = ppo_f64((s_node[0][tid] + s_node[1][tid]) + (s_node[2][tid] + s_node[3][tid]));
    if (OUT_LDS) head_stage_out(d.grad_params + r0 * P, lds, here * P, P, pitch);
}

// tiles: ceil(rows / 256); padded: the smallest power of two >= tiles; per: the power of two with 256 * per >= tiles
__global__ void __launch_bounds__(256) wedm_ppo_fold_kernel(const wedm_ppo_desc d, const int32_t tiles, const int32_t padded,
                                                             const int32_t per) {
    using namespace wedm;
    __shared__ double s_node[4][WEDM_PPO_SUMS];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll 1
    for (int c = 0; c < WEDM_PPO_SUMS; ++c) {
        double v[WEDM_PPO_FOLD_PER];
#pragma unroll
        for (int j = 0; j < WEDM_PPO_FOLD_PER; ++j) {
            const int32_t t = tid * per + j;
            const bool have = j < per && t < tiles;
            v[j] = have ? d.partials[(int64_t)t * WEDM_PPO_SUMS + c] : 0.0;
        }
#pragma unroll
        for (int s = 1; s < WEDM_PPO_FOLD_PER; s <<= 1) {
#pragma unroll
            for (int j = 0; j < WEDM_PPO_FOLD_PER; j += 2 * s)
                v[j] = (j + s < per && tid * per + j + s < padded) ? v[j] + v[j + s] : v[j];
        }
        double node = v[0];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_down(node, off);
            node = (tid + off) * per < padded ? node + o : node;
        }
        if (lane == 0) s_node[wv][c] = node;
    }
    __syncthreads();
    if (tid != 0) return;
    double S[WEDM_PPO_SUMS];
#pragma unroll
    for (int c = 0; c < WEDM_PPO_SUMS; ++c) {
        const double a = 64 * per < padded ? s_node[0][c] + s_node[1][c] : s_node[0][c];
        const double b = 192 * per < padded ? s_node[2][c] + s_node[3][c] : s_node[2][c];
        S[c] = 128 * per < padded ? a + b : a;
    }
    const double n = S[WEDM_PS_LIVE];
    const double scale = n > 0.0 ? 1.0 / n : 0.0;
    const double pl = S[WEDM_PS_POLICY] * scale, vl = S[WEDM_PS_VALUE] * scale, en = S[WEDM_PS_ENTROPY] * scale;
    d.stats[WEDM_PT_N] = ppo_f64(n);
    d.stats[WEDM_PT_N_BAD] = ppo_f64(S[WEDM_PS_BAD]);
    d.stats[WEDM_PT_LOSS] = ppo_f64((pl + d.vf_coef * vl) - d.ent_coef * en);
    d.stats[WEDM_PT_POLICY] = ppo_f64(pl);
    d.stats[WEDM_PT_VALUE] = ppo_f64(vl);
    d.stats[WEDM_PT_ENTROPY] = ppo_f64(en);
    d.stats[WEDM_PT_KL] = ppo_f64(S[WEDM_PS_KL] * scale);
    d.stats[WEDM_PT_CLIP_FRACTION] = ppo_f64(S[WEDM_PS_CLIPPED] * scale);
}
