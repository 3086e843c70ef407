/*
 * dnn_math.h -- the two elementary functions of the DNN mask estimator (dnn_kernel.hip), stated once
 * for the device and for the plain-C model of the tests (tests/dnn_model_driver.c):
 *
 *   sea_lnf (y)    natural logarithm, y >= 1 (finite): the cochleagram's compression
 *   sea_expf (x)   exponential of x clamped to [-88, 88]: the sigmoid
 *
 * Only correctly rounded float + - * /, conversions between int and float that are exact, and integer arithmetic on the
 * exponent field: no libm call, no double, and no a * b + c that a compiler may fuse (contraction is switched off inside the
 * bodies, and both builds pass -ffp-contract=off).  gcc on the host and hipcc for gfx950 therefore give the same bits.
 * sea_fmaf is the one fused operation of the network's arithmetic: fmaf for gcc, __fmaf_rn on the device.
 *
 * Both kernels are fdlibm's float forms (e_logf.c, e_expf.c: the argument reductions and the minimax coefficients are
 * published there).  Measured over every argument that can occur (tests/test_dnn_cpu.py): sea_lnf within 1 ulp of the
 * double log on every float of [1, 2^39] (and of (2^39, 2^41], which only the scores of score_kernel.hip reach:
 * tests/test_scores_cpu.py); sea_expf within 2^-23 relative wherever the result is a normal float.
 */
#ifndef SEA_DNN_MATH_H
#define SEA_DNN_MATH_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SEA_DNN_FN __host__ __device__ static inline
#else
#include <math.h>
#include <stdint.h>
#define SEA_DNN_FN static inline
#endif

#if defined(__clang__)
#define SEA_DNN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SEA_DNN_NO_CONTRACT
#endif

SEA_DNN_FN float sea_fmaf(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}

SEA_DNN_FN uint32_t sea_dnn_bits(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

SEA_DNN_FN float sea_dnn_float(uint32_t u)
{
    float v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

/* ln y for finite y >= 1.  y = 2^k m with m in [sqrt(1/2), sqrt 2); f = m - 1, s = f / (2 + f);
 * ln m = f - f^2/2 + s (f^2/2 + R (s^2)), R of degree 4 in s^2; k ln 2 enters as a high part with 9 trailing zero bits
 * (k <= 127 makes k * ln2_hi exact) and a low part.  y = 1 gives +0. */
SEA_DNN_FN float sea_lnf(float y)
{
    SEA_DNN_NO_CONTRACT
    const float ln2_hi = 6.9313812256e-01f; /* 0x3f317180 */
    const float ln2_lo = 9.0580006145e-06f; /* 0x3717f7d1 */
    const float Lg1 = 0.66666662693f, Lg2 = 0.40000972152f, Lg3 = 0.28498786688f, Lg4 = 0.24279078841f;
    uint32_t ix = sea_dnn_bits(y);
    ix += 0x3f800000u - 0x3f3504f3u;
    const int k = (int)(ix >> 23) - 0x7f;
    ix = (ix & 0x007fffffu) + 0x3f3504f3u;
    const float f = sea_dnn_float(ix) - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * (Lg2 + w * Lg4);
    const float t2 = z * (Lg1 + w * Lg3);
    const float R = t2 + t1;
    const float hfsq = 0.5f * f * f;
    const float dk = (float)k;
    return s * (hfsq + R) + dk * ln2_lo - hfsq + f + dk * ln2_hi;
}

/* exp x, x clamped to [-88, 88] (a NaN stays one).  k = round (x / ln 2), r = x - k ln 2 in two parts,
 * exp r = 1 + (r c / (2 - c) - lo + hi) with c = r - r^2 (P1 + P2 r^2); times 2^k through the exponent field.  k >= -127:
 * below 2^-126 the scaling takes two steps, the second of which rounds once into the subnormals. */
SEA_DNN_FN float sea_expf(float x)
{
    SEA_DNN_NO_CONTRACT
    const float ln2_hi = 6.9314575195e-01f; /* 0x3f317200 */
    const float ln2_lo = 1.4286067653e-06f; /* 0x35bfbe8e */
    const float inv_ln2 = 1.4426950216e+00f;
    const float P1 = 1.6666625440e-01f, P2 = -2.7667332906e-03f;
    if (x > 88.0f) x = 88.0f;
    if (x < -88.0f) x = -88.0f;
    const int k = (int)(x * inv_ln2 + (x < 0.0f ? -0.5f : 0.5f)); /* truncation of a value within +-128 */
    const float dk = (float)k;
    const float hi = x - dk * ln2_hi;
    const float lo = dk * ln2_lo;
    const float r = hi - lo;
    const float rr = r * r;
    const float c = r - rr * (P1 + rr * P2);
    const float e = 1.0f + (r * c / (2.0f - c) - lo + hi);
    if (k >= -126) return e * sea_dnn_float((uint32_t)(k + 127) << 23);
    return (e * sea_dnn_float((uint32_t)(k + 127 + 24) << 23)) * 5.9604644775390625e-08f; /* 2^-24 */
}

/* the network's activations: 0 identity, 1 the logistic function, 2 the rectifier */
SEA_DNN_FN float sea_dnn_act(float z, int act)
{
    if (act == 1) return 1.0f / (1.0f + sea_expf(-z));
    if (act == 2) return z > 0.0f ? z : 0.0f;
    return z;
}

#endif
