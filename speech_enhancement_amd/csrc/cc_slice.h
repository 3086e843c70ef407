/*
 * cc_slice.h -- what the time-slice forms of CompCeps (cc_slice_kernel.hip) and of the feature chain (afe_slice_kernel.hip) have
 * in common: which cepstral frames complete in a slice, the staging of a wideband tile's high-band and code rows, and the carry
 * of the history from one slice to the next.  The callers pass fields, not their argument structs, and say where in their state
 * (sea_kernels.h) each part lies.  Internal to the library.
 *
 * What completes in a slice.  Cepstral frame j of an utterance whose first output is frame f0 reads the float stream from sample
 * 80 (f0 + j) - 1 for 201 values and, in the wideband mode, the high-band and code rows of frame f0 + j; the VAD takes the speech
 * flag of frame f0 + j + 2 with it.  It completes when output frame f0 + j + 2 exists: a slice of the frames [fb, fb + n)
 * completes j in [max(0, fb - f0 - 2), fb + n - f0 - 2).  Up to two frames and one sample of the stream, and two rows of either
 * kind, lie before the slice and come from the state.
 */
#pragma once
#include "ns_core.h"

namespace sea {

namespace {

/* the cepstral frames of an utterance that complete in the slice: [jLo, jLo + nc); nfr = the slice's whole frames */
struct SliceSpan {
    long long nfr, jLo, nc;
    int f0;
};
__device__ __forceinline__ SliceSpan slice_span(int f0, long long nfr, long long fb)
{
    SliceSpan p;
    p.f0 = f0;
    p.nfr = nfr;
    p.jLo = 0;
    p.nc = 0;
    if (p.f0 >= 0) {
        p.jLo = fb - p.f0 - 2 > 0 ? fb - p.f0 - 2 : 0;
        const long long jHi = fb + p.nfr - p.f0 - 2;
        p.nc = jHi > p.jLo ? jHi - p.jLo : 0;
    }
    return p;
}

/* the slice's sample loc of the float stream, -kAfStKeep <= loc: what lies before the slice's first sample is the history */
__device__ __forceinline__ float slice_sample(const float *cur0, const float *hist, int loc, bool resume)
{
    if (loc >= 0) return cur0[loc];
    return resume ? hist[kAfStKeep + loc] : 0.0f;
}

/* a tile's nv rows of high-band energies and code values into LDS: frame r0 + f of the slice (r0 >= -2), the state's two rows
 * (stHp, stCode) before it; row0 = the utterance's first row of the slice's row buffers */
__device__ __forceinline__ void stage_wb_rows(float *hpS, float *codeS, const float *hp_rows, const float *code_rows,
                                              long long row0, int r0, int nv, const float *stHp, const float *stCode,
                                              bool resume, int lane)
{
    for (int i = lane; i < nv * 9; i += kLanes) {
        const int r = r0 + i / 9, c = i % 9;
        codeS[i] = r >= 0 ? code_rows[(row0 + r) * 9 + c] : (resume ? stCode[(2 + r) * 9 + c] : 0.0f);
    }
    if (lane < nv * 3) {
        const int r = r0 + lane / 3, c = lane % 3;
        hpS[lane] = r >= 0 ? hp_rows[(row0 + r) * 3 + c] : (resume ? stHp[(2 + r) * 3 + c] : 0.0f);
    }
}

/* The carry.  Element i of a history of n is element i + m of (old history, the slice's m new ones): everything is read into
 * LDS (keep: kAfStKeep floats for the stream, kCarryRows more for the wideband rows), the caller puts a barrier, then it is
 * stored.  A slice without a whole frame stores back what it read. */
constexpr int kCarryRows = 8 + 24;
__device__ __forceinline__ void carry_load(float *keep, const float *cur, const float *hist, long long nfr, bool resume, int lane)
{
    const long long m8 = nfr * SEA_HOP;
    for (int i = lane; i < kAfStKeep; i += kLanes) {
        const long long j = i + m8;
        keep[i] = j >= kAfStKeep ? cur[j - kAfStKeep] : (resume ? hist[j] : 0.0f);
    }
}
__device__ __forceinline__ void carry_load_rows(float *keep, const float *hp_rows, const float *code_rows, long long row0,
                                                long long nfr, const float *stHp, const float *stCode, bool resume, int lane)
{
    if (lane < 24) {
        const float *rows = lane < 6 ? hp_rows : code_rows, *old = lane < 6 ? stHp : stCode;
        const int wd = lane < 6 ? 3 : 9, i = lane < 6 ? lane : lane - 6;
        const long long r = i / wd + nfr; /* row of (the state's two, the slice's nfr) */
        keep[kAfStKeep + (lane < 6 ? 0 : 8) + i] =
            r >= 2 ? rows[(row0 + r - 2) * wd + i % wd] : (resume ? old[r * wd + i % wd] : 0.0f);
    }
}
__device__ __forceinline__ void carry_store(float *hist, const float *keep, int lane)
{
    for (int i = lane; i < kAfStKeep; i += kLanes) hist[i] = keep[i];
}
__device__ __forceinline__ void carry_store_rows(float *stHp, float *stCode, const float *keep, int lane)
{
    if (lane < 8) stHp[lane] = lane < 6 ? keep[kAfStKeep + lane] : 0.0f;
    if (lane < 24) stCode[lane] = lane < 18 ? keep[kAfStKeep + 8 + lane] : 0.0f;
}

} // namespace

} // namespace sea
