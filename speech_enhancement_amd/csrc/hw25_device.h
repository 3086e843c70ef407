/*
 * hw25_device.h -- what the Hu-Wang kernel files share on the device: the gammatone recurrence of the analysis
 * (hw25_kernel.hip, hw64_kernel.hip) and of the resynthesis that inverts it (hw25_resynth_kernel.hip, hw64_resynth_kernel.hip:
 * the tile's constants, a group of the second pass and the (short) conversion), the hair cell's step of
 * both banks' analysis, and the constants, the lane fence and
 * the label propagation of the estimator's two segmentations, initGroup's (hw25_pitch_kernel.hip, hw64_pitch_kernel.hip) and
 * finalSeg's reSegmentation (hw25_am_kernel.hip, hw64_am_kernel.hip), over 25 and over 64 lanes, and what both banks' AM stage
 * shares: the utterance decode, N of the FFT, bessi0, and the bodies of the FFT's global stages and of the normalisation.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "sea_tables.h"

namespace sea {

/* gammaToneFilter:231-251 for one sample: returns p[3] * gain taken BEFORE the update */
struct Gt25 {
    float p[4], q[4];
};
__device__ __forceinline__ float gt25_step(Gt25 &s, float in, float f1, float f2, float gain)
{
    const float out = s.p[3] * gain;
    float x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[i] = f1 * s.p[i] - f2 * s.q[i];
        y[i] = f2 * s.p[i] + f1 * s.q[i];
    }
    s.p[0] = in * f1 + x[0];
    s.q[0] = in * f2 + y[0];
    s.p[1] = s.p[0] + x[1];
    s.q[1] = s.q[0] + y[1];
    s.p[2] = s.p[1] + x[1] + x[2];
    s.q[2] = s.q[1] + y[1] + y[2];
    s.p[3] = s.p[2] + x[1] + 2 * x[2] + x[3];
    s.q[3] = s.q[2] + y[1] + 2 * y[2] + y[3];
    return out;
}

/* ---- what the resynthesis kernels of both banks share (hw25_resynth_kernel.hip, hw64_resynth_kernel.hip): one wave per
 * utterance walks it in tiles of kResynthTile samples, the channel lanes fetching kResynthGroup samples at a time ---- */
constexpr int kResynthTile = 64;                   /* samples per tile: one per lane in the summing half */
constexpr int kResynthGroup = 8;                   /* samples per fetch of the recurrence */
constexpr int kResynthStride = kResynthTile + 1;   /* words per channel row of the LDS tile */

/* resynthesis:1513-1519 for the eight samples tg .. tg + 7 of one channel, the latest first; kPartial: the group that holds
 * the utterance's last sample, whose samples at or past L are skipped */
template <bool kPartial>
__device__ __forceinline__ void resynth_group(Gt25 &s, const float (&x)[kResynthGroup], long long tg, long long L, float f1, float f2,
                                              float gain, float ear, float *row)
{
    const int j = (int)(tg & (kResynthTile - 1));
#pragma unroll
    for (int k = kResynthGroup - 1; k >= 0; --k) {
        if (kPartial && tg + k >= L) continue;
        const float g2 = gt25_step(s, x[k] / ear, f1, f2, gain);
        row[j + k] = g2 / ear;
    }
}

/* (short) of a float as the x86-64 build converts it (cvttss2si + low half): truncation toward zero to int32, the low 16 bits
 * kept; NaN or a magnitude of 2^31 and more give 0 */
__device__ __forceinline__ short resynth_to_short(float v)
{
    const int i = fabsf(v) < 2147483648.0f ? (int)v : 0;
    return (short)(unsigned short)((unsigned)i & 0xffffu);
}

/* hairCell:279-297 for one sample.  kt is a double expression of the input (float + double literal), rounded once; the rest
 * is float arithmetic; comparisons against the double literals 0.0 and 1.0 are exact in float.  Every constant comes from the
 * bank's tables (sea_hw25_tables or sea_hw64_tables). */
struct Hair25 {
    float q, c, w;
};
template <class Tables>
__device__ __forceinline__ float hair25_step(Hair25 &h, float in, const Tables &t)
{
    const double s = (double)in + 3.0;
    const float kt = (s > 0.0) ? (float)((double)t.gdt * s / (s + 300.0)) : 0.0f;
    const float replenish = (h.q < 1.0f) ? (t.ymdt - t.ydt * h.q) : 0.0f;
    const float eject = kt * h.q;
    const float reuptakeandloss = t.lplusrdt * h.c;
    const float reuptake = t.rdt * h.c;
    const float reprocess = t.xdt * h.w;
    h.q = h.q + replenish - eject + reprocess;
    if (h.q < 0.0f) h.q = 0.0f;
    h.c = h.c + eject - reuptakeandloss;
    if (h.c < 0.0f) h.c = 0.0f;
    h.w = h.w + reuptake - reprocess;
    if (h.w < 0.0f) h.w = 0.0f;
    return t.hdt * h.c;
}

constexpr int kHw25None = 0x7fffffff;                             /* no label, no key */
constexpr unsigned kHw25ChanBits = (1u << SEA_HW25_NCHAN) - 1u;    /* the channel lanes of a ballot */

/* between a write by one lane and a later read by another lane of the same wave */
__device__ __forceinline__ void lanes_fence() { __threadfence(); }

/* what the pitch tracking of both banks shares (hw25_pitch_kernel.hip, hw64_pitch_kernel.hip): the maximum from mvalue = 0
 * (findPitch, the Developes) out of the stored maximum from -inf */
__device__ __forceinline__ float mvalue_of(float mraw) { return mraw > 0.0f ? mraw : 0.0f; }

/* pitchCrn:887-899 */
__device__ __forceinline__ bool pitch_crn(int d1, int d2)
{
    float lowerP = (float)(0.8 * (double)(float)d1);
    float upperP = (float)(1.2 * (double)(float)d1);
    if (d1 > d2)
        upperP = (float)(1.2 * (double)(float)d2);
    else
        lowerP = (float)(0.8 * (double)(float)d2);
    return ((float)d1 > lowerP) && ((float)d1 < upperP) && ((float)d2 > lowerP) && ((float)d2 < upperP);
}

/* One wave per utterance.  lab [F][25]: the unit's own index where it is marked, kHw25None elsewhere.  On return every marked
 * unit holds the smallest unit index of its 4-connected component.  Lane = channel; a frame takes the label of the frame
 * before it in sweep direction (carried in registers), then every run of marked channels takes its minimum.  Forward and
 * backward sweeps until neither changes anything.  The caller fences before and after. */
__device__ __forceinline__ void hw25_label_components(int *lab, int F, int lane)
{
    constexpr int kCh = SEA_HW25_NCHAN;
    bool again = true;
    while (again) {
        bool changed = false;
        for (int dir = 0; dir < 2; ++dir) {
            int carry = kHw25None;
            for (int k = 0; k < F; ++k) {
                const int f = dir ? F - 1 - k : k;
                const int old = lane < kCh ? lab[f * kCh + lane] : kHw25None;
                int v = old;
                if (v != kHw25None && carry < v) v = carry;
                const unsigned m = (unsigned)__ballot(v != kHw25None) & kHw25ChanBits;
                /* the run [start, end] of marked channels around this lane */
                const unsigned below = ~m & ((1u << (lane & 31)) - 1u);
                const int start = below ? 32 - __clz((int)below) : 0;
                const unsigned above = lane < 31 ? (~m >> (lane + 1)) : 1u;
                const int end = lane + (__ffs((int)above) - 1);
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) {
                    const int o = __shfl_up(v, d);
                    if (lane - d >= start && o < v) v = o;
                }
                const int r = __shfl(v, end & 63);
                if (old != kHw25None) {
                    v = r;
                    if (v != old) {
                        lab[f * kCh + lane] = v;
                        changed = true;
                    }
                } else {
                    v = kHw25None;
                }
                carry = v;
            }
        }
        again = __any(changed);
    }
}

/* hw25_label_components with a channel in every lane, for the 64-channel bank's two segmentations (hw64_pitch_kernel.hip,
 * hw64_am_kernel.hip).  lab [F][64]: the unit's own index where it is marked, kHw25None elsewhere.  On return every marked
 * unit holds the smallest unit index of its 4-connected component.  A frame takes the label of the frame before it in sweep
 * direction (carried in registers), then every run of marked channels takes its minimum: a prefix minimum over the 64 lanes
 * that stops at the run's start, read back from the run's end.  Forward and backward sweeps until neither changes anything.
 * The caller fences before and after. */
__device__ __forceinline__ void hw64_label_components(int *lab, int F, int lane)
{
    constexpr int kCh = SEA_HW64_NCHAN;
    bool again = true;
    while (again) {
        bool changed = false;
        for (int dir = 0; dir < 2; ++dir) {
            int carry = kHw25None;
            for (int k = 0; k < F; ++k) {
                const int f = dir ? F - 1 - k : k;
                const int old = lab[f * kCh + lane];
                int v = old;
                if (v != kHw25None && carry < v) v = carry;
                const unsigned long long m = __ballot(v != kHw25None);
                /* the run [start, end] of marked channels around this lane */
                const unsigned long long below = ~m & ((1ull << lane) - 1ull);
                const int start = below ? 64 - __clzll((long long)below) : 0;
                const unsigned long long above = lane < 63 ? (~m >> (lane + 1)) : 0ull;
                const int end = above ? lane + (__ffsll((long long)above) - 1) : 63;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(v, d);
                    if (lane - d >= start && o < v) v = o;
                }
                const int r = __shfl(v, end);
                if (old != kHw25None) {
                    v = r;
                    if (v != old) {
                        lab[f * kCh + lane] = v;
                        changed = true;
                    }
                } else {
                    v = kHw25None;
                }
                carry = v;
            }
        }
        again = __any(changed);
    }
}

/* ---- what the AM stage of both banks shares (hw25_am_kernel.hip, hw64_am_kernel.hip): the utterance a workgroup works on, N
 * of the FFT, bessi0, and the bodies of the FFT's global stages and of the normalisation kernel, which know of the bank only its channel count (in
 * two address expressions) and its hop.  Args is Hw25AmArgs (sea_kernels.h).  Internal to each unit, as they were in
 * hw25_am_kernel.hip. ---- */
namespace {

/* computeAM:1156 for lengths 240 .. 150000: the integer ceil (log2 (L)), and at a power of two the constant that the
 * reference's double expression gave on a CPU (SEA_HW25_N_AT_POW2) */
__device__ __forceinline__ int fft_log2(long long L)
{
    constexpr int at_pow2[11] = SEA_HW25_N_AT_POW2;
    const int up = 64 - __clzll(L - 1);
    if ((L & (L - 1)) == 0 && up >= 7 && up <= 17) return at_pow2[up - 7];
    return up;
}

struct AmUtt {
    int u, nfr, N;
    long long off, L, pitch, row0;
};
template <int kHop, class Args>
__device__ __forceinline__ AmUtt am_utterance(const Args &a)
{
    AmUtt t;
    t.u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    t.off = a.offsets[t.u];
    t.L = a.lengths[t.u];
    t.pitch = (t.L + 7) & ~7LL;
    t.nfr = t.L > 0 ? (int)(t.L / kHop) : 0;
    t.row0 = a.row_offsets[t.u];
    t.N = a.info[t.u];
    return t;
}

/* bessi0:1603-1614, its polynomial branch (|x| < 3.75 always: beta < 3.75 and the square root is at most 1) */
__device__ __forceinline__ float bessi0_small(float x)
{
    float y = (float)((double)x / 3.75);
    y *= y;
    const double d = y;
    return (float)(1.0 + d * (3.5156229 + d * (3.0899424 + d * (1.2067492 + d * (0.2659732 + d * (0.360768e-1 + d * 0.45813e-2))))));
}

/* stage a.stage (above kLdsLog2) in place over global memory: the butterflies of one stage touch disjoint pairs */
template <int kCh, int kHop, class Args>
__device__ __forceinline__ void am_fft_stage(const Args &a)
{
    const int z = blockIdx.z, c = a.chan0 + z, n = a.stage;
    const AmUtt t = am_utterance<kHop>(a);
    if (t.N < n || c >= kCh) return;
    const long long half = 1LL << (t.N - 1);
    const long long period = 1LL << (n - 1);
    float2 *x = (a.inverse ? a.fb : a.fa) + t.off * a.chunk * 2 + (long long)z * 2 * t.pitch;
    const float2 *tw = a.tw + (period - 1);
    const float sign = a.inverse ? -1.0f : 1.0f;
    for (long long b = (long long)blockIdx.y * 256 + threadIdx.x; b < half; b += (long long)gridDim.y * 256) {
        const long long j = b & (period - 1);
        const long long i = ((b >> (n - 1)) << n) + j;
        const float uR = tw[j].x, uI = sign * tw[j].y;
        const float2 lo = x[i], hi = x[i + period];
        const float tmpR = hi.x * uR - hi.y * uI;
        const float tmpI = hi.x * uI + hi.y * uR;
        x[i + period] = make_float2(lo.x - tmpR, lo.y - tmpI);
        x[i] = make_float2(lo.x + tmpR, lo.y + tmpI);
    }
}

/* computeAM:1177-1178: sqrtf of a float, a float over (float) sigL, then a double sum and a double quotient rounded to float */
template <int kCh, int kHop, class Args>
__device__ __forceinline__ void am_norm(const Args &a)
{
    const int z = blockIdx.z, c = a.chan0 + z;
    const AmUtt t = am_utterance<kHop>(a);
    if (t.N < 0 || c >= kCh) return;
    const float sigL = (float)(1LL << t.N);
    const float2 *x = a.fb + t.off * a.chunk * 2 + (long long)z * 2 * t.pitch;
    const float *pat = a.ampatt + t.off * kCh + c * t.pitch;
    float *am = a.am + t.off * kCh + c * t.pitch;
    for (long long n = (long long)blockIdx.y * 256 + threadIdx.x; n < t.L; n += (long long)gridDim.y * 256) {
        const float2 v = x[n];
        const float env = sqrtf(v.x * v.x + v.y * v.y) / sigL;
        am[n] = (float)((double)pat[n] / ((double)env + 1e-30));
    }
}

} // namespace

} // namespace sea
