// wedm_policy_net.h -- wedm_policy_net: a two-hidden-layer actor-critic MLP, forward and backward, on the float32 MFMA.
//
// Not a step kernel and not in the registry: no wedm_ctx, no wedm_params, no plan, no form bits.  The definition (the input
// cleaning, the layers as k-ordered fma chains, the tanh, the backward products, the row sum's chunks and tree) is in
// include/wedm_hip.h and tests hold these kernels to it on every byte.
//
// v_mfma_f32_16x16x4_f32 is bit for bit four steps of a k-ordered fmaf chain per output element, so every product of the
// definition is a run of them into one accumulator with k ascending:
//   lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register g of the result is D[4 (l >> 4) + g][l & 15].
// PADDING is an identity in bits: where a chain's k runs past its length (D up to a multiple of 4, O up to 28, rows past
// `rows` in the last chunk) the A operand is +0.0 and the B operand -0.0, so the step adds the product -0.0, which leaves
// every accumulator as it was, a -0.0 included (a +0.0 product would turn it into +0.0).  Output columns past a matrix's
// width are computed and dropped.
//
// Up to three launches on one stream; no block waits for another, nothing spins, no atomic:
//   wedm_net_kernel<false, ..>  (FORWARD) a block of four waves takes 128 rows: the three layers one after the other, two
//       16 x 16 output tiles side by side per wave and step (they share A), h1 and h2 in LDS only.
//   wedm_net_kernel<true, ..>   (BACKWARD's MAIN) a block is a tile of 256 rows in two passes of 128 rows (two chunks): h1, h2
//       recomputed into LDS, go staged into LDS, then per layer from the top: the weight gradient's tiles (the layer's
//       input transposed as A with a row of ones under it for the bias, the row as k: 16 steps per chunk, one accumulator
//       per chunk and column tile, two column tiles at once, added lower chunk on the left), a barrier, the back-propagated product times act' written over the
//       activation it was taken from.  The first pass parks the node of chunks 0 and 1 (in LDS where it fits, else in the
//       tile's partials, which the same lane reads back), the second adds the node of chunks 2 and 3 on its right and
//       stores partials[tile] -- once where the park is LDS.
//   wedm_net_fold_kernel    (FOLD) a block takes 32 parameters, its eight groups of lanes an eighth of the padded tile range
//       each: the pairwise tree over a group's tiles as a binary counter of complete subtrees in registers, what is left at
//       the end joined from the top, so a node without a right child is its left child unchanged; the groups' nodes meet in
//       LDS for the last three levels.
// theta is staged into LDS once per block where it fits beside the activations (WLDS; rows of N + 4 floats: the transposed
// reads of the back-propagated products then fall on distinct banks); otherwise the operands come from global memory.
// Observations are read at src = index[r] with a plain gather, as in wedm_ppo.h.
// Every index is formed from thread and block numbers and descriptor fields, or from index[r] after it has been compared
// with [0, n_src).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/wedm_hip.h"

#define WEDM_NET_BLOCK 256   // four waves
#define WEDM_NET_PASS 128    // rows of a pass: two chunks
#define WEDM_NET_GO_PITCH 36 // an LDS row of go: 32 columns + 4
#define WEDM_NET_LDS_LIMIT (160 * 1024)

namespace wedm {

typedef float net_f4 __attribute__((ext_vector_type(4)));

// The shape of a call and where its pieces lie in theta (offsets in floats) and in LDS (offsets in floats from the base).
struct net_shape {
    int D, H1, H2, O;
    int w1, w2, w3, n_theta;           // W1 | b1, W2 | b2, W3 | b3 start at w1, w2, w3: (K + 1) rows of N
    int act1, act2, go, src, park, wts; // LDS; park / wts: -1 where it is not in LDS
    int lw1, lw2, lw3;                 // the staged layers inside wts, rows of N + 4
    int lds_floats;
};

__host__ __device__ inline net_shape net_make_shape(int D, int H1, int H2, int O, bool backward) {
    net_shape s;
    s.D = D, s.H1 = H1, s.H2 = H2, s.O = O;
    s.w1 = 0;
    s.w2 = (D + 1) * H1;
    s.w3 = s.w2 + (H1 + 1) * H2;
    s.n_theta = s.w3 + (H2 + 1) * O;
    int at = 0;
    s.src = at, at += 2 * WEDM_NET_PASS;  // int64 src per row of the pass
    s.act1 = at, at += WEDM_NET_PASS * (H1 + 4);
    s.act2 = at, at += WEDM_NET_PASS * (H2 + 4);
    s.go = at, at += backward ? WEDM_NET_PASS * WEDM_NET_GO_PITCH : 0;
    const int limit = WEDM_NET_LDS_LIMIT / 4;
    s.park = -1;
    if (backward && at + s.n_theta <= limit) s.park = at, at += s.n_theta;
    const int staged = (D + 1) * (H1 + 4) + (H1 + 1) * (H2 + 4) + (H2 + 1) * (O + 4);
    s.wts = -1, s.lw1 = s.lw2 = s.lw3 = 0;
    if (at + staged <= limit) {
        s.wts = at, at += staged;
        s.lw1 = s.wts;
        s.lw2 = s.lw1 + (D + 1) * (H1 + 4);
        s.lw3 = s.lw2 + (H1 + 1) * (H2 + 4);
    }
    s.lds_floats = at;
    return s;
}

__device__ __forceinline__ float net_canon(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }

__device__ __forceinline__ float net_clean(float o) { return o != o ? 0.0f : (o < -FLT_MAX ? -FLT_MAX : (o > FLT_MAX ? FLT_MAX : o)); }

// WEDM_NET_TANH of include/wedm_hip.h, step for step
__device__ __forceinline__ float net_tanh(float a) {
    const uint32_t ua = __float_as_uint(a);
    const float m = __uint_as_float(ua & 0x7FFFFFFFu);
    const float z = m + m;
    const float t = fmaf(z, 0x1.715476p+0f, 12582912.0f);
    const float n = t - 12582912.0f;
    float r = fmaf(n, -0x1.62e400p-1f, z);
    r = fmaf(n, -0x1.7f7d1cp-20f, r);
    float p = fmaf(r, 0x1.a01a02p-16f, 0x1.a01a02p-13f);
    p = fmaf(r, p, 0x1.6c16c2p-10f);
    p = fmaf(r, p, 0x1.111112p-7f);
    p = fmaf(r, p, 0x1.555556p-5f);
    p = fmaf(r, p, 0x1.555556p-3f);
    p = fmaf(r, p, 0.5f);
    const float q = fmaf(r * r, p, r);
    const float s = __uint_as_float((__float_as_uint(t) << 23) + 0x3F800000u);
    const float e = fmaf(s, q, s - 1.0f);
    const float d = e + 2.0f;
    float g = m < 0.5f ? e / d : 1.0f - 2.0f / d;
    g = m > 10.0f ? 1.0f : g;
    return __uint_as_float(__float_as_uint(g) | (ua & 0x80000000u));
}

template <bool TANH>
__device__ __forceinline__ float net_act(float a) {
    return TANH ? net_tanh(a) : (a > 0.0f ? a : 0.0f);
}
template <bool TANH>
__device__ __forceinline__ float net_dact(float h) {
    return TANH ? fmaf(-h, h, 1.0f) : (h > 0.0f ? 1.0f : 0.0f);
}

// Two 16 x 16 output tiles side by side (columns j0 and j1 = j0 + 16; the second only where has1, which is uniform) by one
// wave: into each accumulator k = 0 .. K - 1 ascending in steps of four, the two chains independent of each other, which
// is what keeps the matrix pipe fed.  a_at(i, k) and b_at(k, j) give the operands for k < K; past K the step is the
// identity.  i, j0 and j1 are the row and the columns of this lane's operands.
template <class AF, class BF>
__device__ __forceinline__ void net_tile2(net_f4& acc0, net_f4& acc1, const int K, const int i, const int j0, const int j1, const bool has1,
                                          const int lane, AF a_at, BF b_at) {
    const int kq = lane >> 4;
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kq;
        const bool in = k < K;
        const float a = in ? a_at(i, k) : 0.0f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, in ? b_at(k, j0) : -0.0f, acc0, 0, 0, 0);
        if (has1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, in ? b_at(k, j1) : -0.0f, acc1, 0, 0, 0);
    }
}

}  // namespace wedm

// FORWARD (BWD false): grid = ceil(rows / 128), one pass.  MAIN (BWD true): grid = tiles of 256 rows, two passes.
// Dynamic LDS: net_make_shape(...).lds_floats floats.
// WLDS: theta is staged in LDS (the host asks net_make_shape whether it fits).
template <bool BWD, bool TANH, bool WLDS>
__global__ void __launch_bounds__(WEDM_NET_BLOCK) wedm_net_kernel(const wedm_net_desc d) {
    using namespace wedm;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = d.obs_dim, H1 = d.hidden1, H2 = d.hidden2, P = 8 + d.n_modes, O = P + 1;
    const net_shape S = net_make_shape(D, H1, H2, O, BWD);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
    const int p1 = H1 + 4, p2 = H2 + 4;
    float* const act1 = lds + S.act1;
    float* const act2 = lds + S.act2;
    float* const gol = lds + S.go;
    int64_t* const srcs = reinterpret_cast<int64_t*>(lds + S.src);
    // theta: staged once per block where it fits
    const float* const G1 = d.theta + S.w1;
    const float* const G2 = d.theta + S.w2;
    const float* const G3 = d.theta + S.w3;
    if (WLDS) {
        for (int e = tid; e < (D + 1) * H1; e += WEDM_NET_BLOCK) lds[S.lw1 + (e / H1) * (H1 + 4) + e % H1] = G1[e];
        for (int e = tid; e < (H1 + 1) * H2; e += WEDM_NET_BLOCK) lds[S.lw2 + (e / H2) * (H2 + 4) + e % H2] = G2[e];
        for (int e = tid; e < (H2 + 1) * O; e += WEDM_NET_BLOCK) lds[S.lw3 + (e / O) * (O + 4) + e % O] = G3[e];
    }
    const float* const W1 = WLDS ? lds + S.lw1 : G1;
    const float* const W2 = WLDS ? lds + S.lw2 : G2;
    const float* const W3 = WLDS ? lds + S.lw3 : G3;
    const int q1 = WLDS ? H1 + 4 : H1, q2 = WLDS ? H2 + 4 : H2, q3 = WLDS ? O + 4 : O;  // the pitch of a layer's rows
    const int64_t base = (int64_t)blockIdx.x * (BWD ? 256 : WEDM_NET_PASS);
    const int n_pass = BWD ? ((int64_t)d.rows - base > WEDM_NET_PASS ? 2 : 1) : 1;
    float* const part = BWD ? d.partials + (int64_t)blockIdx.x * S.n_theta : nullptr;
    float* const park = !BWD ? nullptr : (S.park >= 0 ? lds + S.park : part);

    for (int pass = 0; pass < n_pass; ++pass) {
        const int64_t r0 = base + (int64_t)pass * WEDM_NET_PASS;
        const int here = (int)((int64_t)d.rows - r0 < WEDM_NET_PASS ? (int64_t)d.rows - r0 : WEDM_NET_PASS);  // >= 1
        __syncthreads();  // the staged theta; the pass before is done with the LDS
        if (tid < WEDM_NET_PASS) {
            int64_t src = -1;
            if (tid < here) {
                src = d.index ? d.index[r0 + tid] : r0 + tid;
                if (src < 0 || src >= d.n_src) src = -1;
            }
            srcs[tid] = src;
        }
        if (BWD) {  // go: rows of the pass, 32 columns; +0.0 past O, for a bad src and past the rows
            for (int e = tid; e < WEDM_NET_PASS * 32; e += WEDM_NET_BLOCK) {
                const int row = e >> 5, j = e & 31;
                float g = 0.0f;
                if (row < here && j < O) {
                    const int64_t r = r0 + row;
                    int64_t src = d.index ? d.index[r] : r;
                    if (src >= 0 && src < d.n_src) g = j < P ? d.grad_params[r * d.grad_stride + j] : d.grad_value[r];
                }
                gol[row * WEDM_NET_GO_PITCH + j] = g;
            }
        }
        __syncthreads();
        const int n_rt = (here + 15) >> 4;  // row tiles that hold a row
        const auto x_at = [&](const int row, const int k) -> float {
            const int64_t src = srcs[row];
            return src >= 0 ? net_clean(d.obs[src * d.obs_stride + k]) : 0.0f;
        };
        // a product over the rows of the pass, its column tiles in pairs: start(j) the accumulator's first value,
        // store(rt, j, acc) what becomes of a tile
        const auto product = [&](const int K, const int n_ct, auto a_at, auto b_at, auto start, auto store) {
            const int n_cp = (n_ct + 1) >> 1;
            for (int it = wave; it < n_rt * n_cp; it += 4) {
                const int rt = it / n_cp, cp = it % n_cp, j0 = 32 * cp + lo, j1 = j0 + 16;
                const bool has1 = 2 * cp + 1 < n_ct;
                const float s0 = start(j0), s1 = has1 ? start(j1) : 0.0f;
                net_f4 acc0 = {s0, s0, s0, s0}, acc1 = {s1, s1, s1, s1};
                net_tile2(acc0, acc1, K, 16 * rt + lo, j0, j1, has1, lane, a_at, b_at);
                store(rt, j0, acc0);
                if (has1) store(rt, j1, acc1);
            }
        };
        // layer 1: h1 = act(x W1 + b1)
        product(D, H1 >> 4, x_at, [&](int k, int j) { return W1[k * q1 + j]; }, [&](int j) { return W1[D * q1 + j]; },
                [&](int rt, int j, const net_f4& acc) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) act1[(16 * rt + 4 * hi + g) * p1 + j] = net_act<TANH>(acc[g]);
                });
        __syncthreads();
        // layer 2: h2 = act(h1 W2 + b2)
        product(H1, H2 >> 4, [&](int row, int k) { return act1[row * p1 + k]; }, [&](int k, int j) { return W2[k * q2 + j]; },
                [&](int j) { return W2[H1 * q2 + j]; },
                [&](int rt, int j, const net_f4& acc) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) act2[(16 * rt + 4 * hi + g) * p2 + j] = net_act<TANH>(acc[g]);
                });
        __syncthreads();
        if (!BWD) {
            // layer 3: out = h2 W3 + b3; columns [0, P) are the head's row, column P the value, columns from O on are dropped
            product(H2, 2, [&](int row, int k) { return act2[row * p2 + k]; }, [&](int k, int j) { return j < O ? W3[k * q3 + j] : 0.0f; },
                    [&](int j) { return j < O ? W3[H2 * q3 + j] : 0.0f; },
                    [&](int rt, int j, const net_f4& acc) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int row = 16 * rt + 4 * hi + g;
                            if (row < here && j < O) {
                                const int64_t r = r0 + row;
                                if (j < P) d.params[r * d.param_stride + j] = net_canon(acc[g]);
                                else d.value[r] = net_canon(acc[g]);
                            }
                        }
                    });
            continue;
        }
        // ---- backward.  A weight gradient's node of this pass: chunk a (rows [0, 64) of the pass) and, where it holds a
        // row, chunk b on its right; then the park and the tile's partials.
        const bool two = here > 64;
        // in_at(k, row): the layer's input transposed, a row of ones under it; g_at(row, j): the gradient at the layer's output
        const auto wgrad = [&](const int K, const int N, const int goff, auto in_at, auto g_at) {
            const int n_cp = (((N + 15) >> 4) + 1) >> 1, n_kt = (K + 1 + 15) >> 4;  // column tiles in pairs that share A
            for (int it = wave; it < n_kt * n_cp; it += 4) {
                const int kt = it / n_cp, cp = it % n_cp;
                const int kx = 16 * kt + lo, j0 = 32 * cp + lo, j1 = j0 + 16;  // this lane's A row and B columns
                const bool has1 = 32 * cp + 16 < N;
                // (rows past `here` inside a chunk that holds a row: A +0.0, B -0.0, the identity)
                const auto a_at = [&](int row) { return row < here ? (kx < K ? in_at(kx, row) : (kx == K ? 1.0f : 0.0f)) : 0.0f; };
                const auto b_at = [&](int row, int j) { return row < here ? (j < N ? g_at(row, j) : 0.0f) : -0.0f; };
                net_f4 na0 = {0.0f, 0.0f, 0.0f, 0.0f}, nb0 = na0, na1 = na0, nb1 = na0;
#pragma unroll 4
                for (int k0 = 0; k0 < 64; k0 += 4) {
                    const int ra = k0 + hi, rb = 64 + k0 + hi;
                    const float aa = a_at(ra);
                    na0 = __builtin_amdgcn_mfma_f32_16x16x4f32(aa, b_at(ra, j0), na0, 0, 0, 0);
                    if (has1) na1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aa, b_at(ra, j1), na1, 0, 0, 0);
                    if (two) {
                        const float ab = a_at(rb);
                        nb0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ab, b_at(rb, j0), nb0, 0, 0, 0);
                        if (has1) nb1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ab, b_at(rb, j1), nb1, 0, 0, 0);
                    }
                }
                const auto store = [&](const int j, const net_f4& na, const net_f4& nb) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k = 16 * kt + 4 * hi + g;
                        if (k <= K && j < N) {
                            const int e = goff + k * N + j;
                            const float node = two ? na[g] + nb[g] : na[g];
                            if (n_pass == 2 && pass == 0) park[e] = node;
                            else part[e] = net_canon(n_pass == 2 ? park[e] + node : node);
                        }
                    }
                };
                store(j0, na0, nb0);
                if (has1) store(j1, na1, nb1);
            }
        };
        // back-propagated product into `act` (rows x K, pitch p): dh = g W^T from +0.0 over j < N, then dh * act'(h) in place
        const auto bprop = [&](const int K, const int N, float* const act, const int p, const float* const W, const int q, auto g_at) {
            product(N, K >> 4, g_at, [&](int j, int kc) { return W[kc * q + j]; }, [](int) { return 0.0f; },
                    [&](int rt, int kc, const net_f4& acc) {  // kc: the output column, the layer's input index
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            float* const h = act + (16 * rt + 4 * hi + g) * p + kc;
                            *h = acc[g] * net_dact<TANH>(*h);
                        }
                    });
        };
        const auto go_at = [&](int row, int j) { return gol[row * WEDM_NET_GO_PITCH + j]; };
        const auto a2_at = [&](int row, int j) { return act2[row * p2 + j]; };
        const auto a1_at = [&](int row, int j) { return act1[row * p1 + j]; };
        wgrad(H2, O, S.w3, [&](int k, int row) { return act2[row * p2 + k]; }, go_at);
        __syncthreads();
        bprop(H2, O, act2, p2, W3, q3, go_at);  // act2: da2
        __syncthreads();
        wgrad(H1, H2, S.w2, [&](int k, int row) { return act1[row * p1 + k]; }, a2_at);
        __syncthreads();
        bprop(H1, H2, act1, p1, W2, q2, a2_at);  // act1: da1
        __syncthreads();
        wgrad(D, H1, S.w1, [&](int k, int row) { return x_at(row, k); }, a1_at);
    }
}

// A block takes 32 parameters, its eight groups of 32 lanes an eighth of the padded tile range each (`per` tiles, a power
// of two): a lane walks its group's tiles for its parameter with a binary counter of complete subtrees in registers and
// joins what is left from the top; the eight groups' nodes meet in LDS and group 0 joins them, three levels.  A group or a
// subtree that holds no tile is absent: its sibling goes up unchanged.
#define WEDM_NET_FOLD_PARAMS 32
__global__ void __launch_bounds__(256) wedm_net_fold_kernel(const wedm_net_desc d, const int32_t n_theta, const int32_t tiles,
                                                            const int32_t per, const int32_t accumulate) {
    __shared__ float s_node[8][WEDM_NET_FOLD_PARAMS];
    const int32_t g = (int32_t)threadIdx.x >> 5, e = (int32_t)blockIdx.x * WEDM_NET_FOLD_PARAMS + ((int32_t)threadIdx.x & 31);
    const int32_t t0 = g * per, n = tiles - t0 < per ? tiles - t0 : per;  // this group's tiles: [t0, t0 + n), n <= 0: none
    float st[13];  // st[L]: a complete subtree of 2^L tiles waiting for its right sibling
#pragma unroll
    for (int L = 0; L < 13; ++L) st[L] = 0.0f;
    if (e < n_theta) {
        for (int32_t t = 0; t < n; ++t) {
            float v = d.partials[(int64_t)(t0 + t) * n_theta + e];
            bool placed = false;
#pragma unroll
            for (int L = 0; L < 13; ++L) {
                if (!placed) {
                    if ((t >> L) & 1) v = st[L] + v;
                    else st[L] = v, placed = true;
                }
            }
        }
    }
    float node = 0.0f;
    bool have = false;
#pragma unroll
    for (int L = 0; L < 13; ++L) {
        if (n > 0 && ((n >> L) & 1)) {
            node = have ? st[L] + node : st[L];
            have = true;
        }
    }
    s_node[g][threadIdx.x & 31] = node;
    __syncthreads();
    if (g != 0 || e >= n_theta) return;
    const int l = (int)threadIdx.x;
    const auto join = [&](float a, bool ha, float b, bool hb, bool& h) {  // hb implies ha: tiles fill the groups from the left
        h = ha;
        return hb ? a + b : a;
    };
    bool h01, h23, h45, h67, h03, h47, h07;
    const float n01 = join(s_node[0][l], 0 * per < tiles, s_node[1][l], 1 * per < tiles, h01);
    const float n23 = join(s_node[2][l], 2 * per < tiles, s_node[3][l], 3 * per < tiles, h23);
    const float n45 = join(s_node[4][l], 4 * per < tiles, s_node[5][l], 5 * per < tiles, h45);
    const float n67 = join(s_node[6][l], 6 * per < tiles, s_node[7][l], 7 * per < tiles, h67);
    const float n03 = join(n01, h01, n23, h23, h03);
    const float n47 = join(n45, h45, n67, h67, h47);
    const float root = join(n03, h03, n47, h47, h07);
    d.grad_theta[e] = wedm::net_canon(accumulate ? d.grad_theta[e] + root : root);
}
