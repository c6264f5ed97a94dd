// wedm_portable.h — the device functions that are pure arithmetic: the float64 bit casts, exp / log / cube from IEEE basic
// operations (the expression trees the CPU oracle evaluates in its PORTABLE math mode), CPython's float `//`, the spark's
// cell, and Philox4x32-10 with the variates drawn from it.
//
// No Env, no state row, no kernel form: the step kernels take these through wedm_device.h, the stateless kernel families
// that need them (wedm_head.h, wedm_geometry.h, wedm_randomize.h, wedm_minibatch.h) include this file alone.  The
// bit-exactness rules are those at the head of wedm_device.h (compile with -ffp-contract=off -fno-fast-math).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wedm {

// ---------------------------------------------------------------- small helpers
__device__ __forceinline__ double bits2d(uint64_t u) { return __longlong_as_double((long long)u); }
__device__ __forceinline__ uint64_t d2bits(double d) { return (uint64_t)__double_as_longlong(d); }

// exp(x) from IEEE basic operations (ln2 hi/lo reduction + degree-5 minimax)
__device__ __forceinline__ double portable_exp(double x) {
    const double ln2hi = 6.93147180369123816490e-01, ln2lo = 1.90821492927058770002e-10;
    const double invln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03;
    const double P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06;
    const double P5 = 4.13813679705723846039e-08;
    if (x != x) return x;
    if (x > 709.0) return __builtin_huge_val();
    if (x < -708.0) return 0.0;
    double hi = x, lo = 0.0;
    int k = 0;
    double ax = __builtin_fabs(x);
    if (ax > 0.34657359027997264) {
        k = (int)(invln2 * x + (x < 0 ? -0.5 : 0.5));
        hi = x - (double)k * ln2hi;
        lo = (double)k * ln2lo;
        x = hi - lo;
    } else if (ax < 3.725290298461914e-09) {
        return 1.0 + x;
    }
    double t = x * x;
    double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    return y * bits2d((uint64_t)(k + 1023) << 52);
}

// log(x) for positive normal x (only use: the polar method's s in (0,1))
__device__ __forceinline__ double portable_log(double x) {
    const double ln2hi = 6.93147180369123816490e-01, ln2lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01;
    const double Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01;
    const double Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01;
    const double Lg7 = 1.479819860511658591e-01;
    uint64_t ux = d2bits(x);
    uint32_t hx = (uint32_t)(ux >> 32);
    int k = (int)(hx >> 20) - 1023;
    hx &= 0x000fffffu;
    uint32_t i = (hx + 0x95f64u) & 0x100000u;
    ux = ((uint64_t)(hx | (i ^ 0x3ff00000u)) << 32) | (ux & 0xffffffffu);
    k += (int)(i >> 20);
    double f = bits2d(ux) - 1.0;
    double dk = (double)k;
    double hfsq = 0.5 * f * f;
    double s = f / (2.0 + f);
    double z = s * s;
    double w = z * z;
    double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    double R = t2 + t1;
    return dk * ln2hi - ((hfsq - (s * (hfsq + R) + dk * ln2lo)) - f);
}

// correctly rounded x^3 (double-double product; `(g/g_ref)**3`, dielectric.py:118)
__device__ __forceinline__ double cube_cr(double x) {
    double p = x * x, e = __builtin_fma(x, x, -p);
    double q = p * x, eq = __builtin_fma(p, x, -q);
    return q + (eq + e * x);
}

// CPython float `//` (float_divmod); wire.py:290-294 `int(y_spark // segment_len)`
__device__ __forceinline__ double py_floordiv(double vx, double wx) {
    double mod = fmod(vx, wx);
    double div = (vx - mod) / wx;
    if (mod != 0.0) {
        if ((wx < 0) != (mod < 0)) {
            mod += wx;
            div -= 1.0;
        }
    }
    double fd;
    if (div != 0.0) {
        fd = floor(div);
        if (div - fd > 0.5) fd += 1.0;
    } else {
        fd = __builtin_copysign(0.0, vx / wx);
    }
    return fd;
}

// int(y // seg) for the spark's cell (wire.py:290-294).  For y >= 0, seg > 0 CPython's float_divmod returns the exact
// floor of the real quotient (fmod is exact, (y - mod) / seg is within half a unit of the integer it then rounds to),
// and that integer is also what one division, a floor and ONE fused remainder give: r = fma(-n, seg, y) is the
// correctly rounded y - n seg, so its sign and its comparison with seg are those of the exact remainder, which
// corrects a floor(y / seg) that the division's rounding put one off.  ~20 instructions instead of ~105 (fmod is a
// software loop); anything else (negative, NaN, huge) takes CPython's own sequence.
__device__ __forceinline__ int spark_cell_offset(double y, double seg) {
    const double q = y / seg;
    const bool fast = y >= 0.0 && seg > 0.0 && q < 1.0e9;
    double n = floor(q);
    const double r = __builtin_fma(-n, seg, y);
    n = r < 0.0 ? n - 1.0 : (r >= seg ? n + 1.0 : n);
    if (!fast) n = py_floordiv(y, seg);
    return (int)n;
}

// ------------------------------------------------------------------------- RNG
// Philox4x32-10, counter {time, episode, global env id, stream}, key = reset seed.
// Counter-based: a variate is a pure function of (seed, env, episode, time, slot),
// so results do not depend on launch geometry, fusion depth or sharding.
//   stream 0   : the four uniforms one microsecond can need (debris-short roll,
//                random-short roll, ignition roll, spark location), u = (w+0.5)*2^-32;
//   stream 1+j : 53-bit pair j of the polar method (crater normal).
struct W4 { uint32_t x, y, z, w; };

__device__ __forceinline__ W4 philox4(uint32_t key0, uint32_t key1, uint32_t time, uint32_t episode,
                                      uint32_t gid, uint32_t stream) {
    uint32_t c0 = time, c1 = episode, c2 = gid, c3 = stream, k0 = key0, k1 = key1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // 64-bit products: one v_mad_u64_u32 each instead of a mul_lo + mul_hi pair
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return W4{c0, c1, c2, c3};
}

__device__ __forceinline__ double u32_to_unit(uint32_t w) { return ((double)w + 0.5) * 2.3283064365386963e-10; }

struct U2 { double a, b; };
__device__ __forceinline__ U2 philox_pair(uint32_t key0, uint32_t key1, uint32_t time, uint32_t episode,
                                           uint32_t gid, uint32_t stream) {
    W4 w = philox4(key0, key1, time, episode, gid, stream);
    U2 u;
    u.a = ((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) / 9007199254740992.0;
    u.b = ((double)(w.z >> 5) * 67108864.0 + (double)(w.w >> 6)) / 9007199254740992.0;
    return u;
}

// Marsaglia polar method on Philox streams 1, 2, ... (material.py:127's N(0,1)); the policy head draws its normals on
// streams of its own (stream_base of wedm_head.h)
__device__ __forceinline__ double philox_std_normal(uint32_t key0, uint32_t key1, uint32_t time,
                                                    uint32_t episode, uint32_t gid, uint32_t stream_base = 1u) {
    for (uint32_t j = 0; j < 64; ++j) {
        U2 u = philox_pair(key0, key1, time, episode, gid, stream_base + j);
        double v1 = 2.0 * u.a - 1.0, v2 = 2.0 * u.b - 1.0;
        double s = v1 * v1 + v2 * v2;
        if (s < 1.0 && s != 0.0) return v1 * sqrt(-2.0 * portable_log(s) / s);
    }
    return 0.0;
}

}  // namespace wedm
