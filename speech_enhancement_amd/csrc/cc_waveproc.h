/*
 * cc_waveproc.h -- DoWaveProc (etsi/cpp/WaveProc.c) in three wave-wide steps, shared by afe_ceps_kernel (cc_kernel.hip) and
 * afe_wb_ceps_kernel (afe_wb_kernel.hip): WaveProc.c never reads Do16kHzProc.  Internal to the library.
 */
#pragma once
#include "ns_core.h"

namespace sea {

namespace {

/* DoWaveProc: the peak searches of four frames run side by side, one per row of 16 lanes (feature pass 4.19 -> 3.82 ms against
 * one frame at a time, wave-wide).  Dealing the Teager / smoothing / window steps of the four frames to the lanes as 800 samples as
 * well (13 rounds, one sync per group) measured SLOWER, 4.39 ms: per-lane frame index, divisions by 200 and a divergent loop over
 * each frame's own peak list */

struct __attribute__((aligned(16))) WpLds { /* scratch of DoWaveProc: four frames in flight */
    float tw[200];
    int q[200];
    int sm[4][200];
    int pos[4][24];
    int nom[4];
};

/* maximum over each ROW of 16 lanes, left in every lane of the row: an xor butterfly in four DPP steps
 * (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror) */
__device__ __forceinline__ int row_max_i32(int v)
{
    auto mx = [](int a, int b) { return a > b ? a : b; };
    v = mx(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));
    return v;
}

/* arg-max of (value >= 0, index < 256) pairs per row of 16 lanes (every lane of a row gets its row's answer); ties go to the
 * LOWER index if lowWins, else the higher.  Entries with valid == false never win.  Returns the winning index, -1 if none. */
__device__ __forceinline__ int row_argmax(int value, int index, bool valid, bool lowWins)
{
    const int m = row_max_i32(valid ? value : -1);
    const int code = (valid && value == m) ? (lowWins ? 255 - index : index) : -1;
    const int c = row_max_i32(code);
    return (m < 0) ? -1 : (lowWins ? 255 - c : c);
}

/* DoWaveProc (WaveProc.c:397-455) on a frame d[0..199] whose low-energy check (:423-427: in-order sum of squares >= 100,
 * evaluated by the caller lane = frame) has passed, in three steps:
 *   wp_smooth   Teager energy (:216-226) and its 9-point integer smoothing                      -> W.sm[slot]
 *   wp_peaks4   maxima 25..79 samples apart (:102-190), four frames side by side               -> W.pos[slot], W.nom[slot]
 *   wp_window   a two-level window around them (:244-330), applied in place
 * Each ends with wave_sync(). */
__device__ __forceinline__ void wp_smooth(WpLds &W, int slot, const float *d, int lane)
{
    constexpr int N = 200;
    /* Teager energy and its integer quarter, (int)floor(T * 0.25 + 0.5) in double */
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        if (i < N) {
            const float a = d[i], l = d[i > 0 ? i - 1 : 0], r = d[i < N - 1 ? i + 1 : N - 1];
            /* ends: |d0*d0 - d0*d1| and |dN-1*dN-1 - dN-2*dN-1| (the missing neighbour is the sample itself) */
            const float t = (i == 0) ? fabsf(a * a - a * r) : ((i == N - 1) ? fabsf(a * a - l * a) : fabsf(a * a - l * r));
            W.q[i] = (int)floor((double)t * 0.25 + 0.5);
        }
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        if (i < N) {
            unsigned acc = 0;
#pragma unroll
            for (int j = -4; j <= 4; ++j) {
                int idx = i + j;
                idx = idx < 0 ? 0 : (idx > N - 1 ? N - 1 : idx);
                acc += (unsigned)W.q[idx];
            }
            W.sm[slot][i] = (int)acc;
        }
    }
    wave_sync();
}

/* the search for up to four frames at once, frame `slot` = row `slot` of 16 lanes (mask: bit slot = that frame takes
 * part): the searches are short dependent chains of wave-wide reductions, so four of them side by side cost what one does */
__device__ __forceinline__ void wp_peaks4(WpLds &W, unsigned mask, int lane)
{
    constexpr int N = 200;
    const int row = lane >> 4, l = lane & 15;
    const int *sm = W.sm[row];
    const bool on = (mask >> row) & 1u;
    int bv = 0, bi = -1;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const int i = l + 16 * k;
        if (i < N) {
            const int v = sm[i];
            if (v > bv) { /* ascending i per lane: strict > keeps the first */
                bv = v;
                bi = i;
            }
        }
    }
    const int p0 = row_argmax(bv, bi, on && bi >= 0, true);
    int nom = 0;
    int R[10], Lf[10], cR = 0, cL = 0;
    R[0] = Lf[0] = p0;
    int cur = p0;
    bool go = p0 >= 0 && cur + 25 < N;
#pragma unroll 1
    while (__ballot(go) != 0ull) { /* to the right: last of equals = the higher index */
        int v = -1, vi = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int off = l + 16 * k, idx = cur + 25 + off;
            if (go && off < 55 && idx < N) {
                const int x = sm[idx];
                if (x >= v) { /* ascending idx per lane: >= keeps the last */
                    v = x;
                    vi = idx;
                }
            }
        }
        const int nx = row_argmax(v, vi, go && v >= 0, false);
        if (go) {
            if (nx >= 0) {
#pragma unroll
                for (int c = 0; c < 9; ++c)
                    if (c == cR) R[c + 1] = nx;
                cR++;
                cur = nx;
                go = cur + 25 < N;
            } else
                go = false;
        }
    }
    cur = p0;
    go = p0 >= 0 && cur - 25 > 0;
#pragma unroll 1
    while (__ballot(go) != 0ull) { /* to the left: last of equals in scan order = the lower index */
        int v = -1, vi = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int off = l + 16 * k, idx = cur - 25 - off;
            if (go && off < 55 && idx > -1) {
                const int x = sm[idx];
                if (x >= v) { /* descending idx per lane: >= keeps the lowest */
                    v = x;
                    vi = idx;
                }
            }
        }
        const int nx = row_argmax(v, vi, go && v >= 0, true);
        if (go) {
            if (nx >= 0) {
#pragma unroll
                for (int c = 0; c < 9; ++c)
                    if (c == cL) Lf[c + 1] = nx;
                cL++;
                cur = nx;
                go = cur - 25 > 0;
            } else
                go = false;
        }
    }
    if (p0 >= 0) {
        if (l == 0) { /* ascending: left ones (farthest first), centre, right ones */
#pragma unroll
            for (int c = 9; c >= 1; --c)
                if (c <= cL) W.pos[row][nom++] = Lf[c];
#pragma unroll
            for (int c = 0; c < 10; ++c)
                if (c <= cR) W.pos[row][nom++] = R[c];
        }
        nom = cL + cR + 1;
    }
    if (l == 0) W.nom[row] = nom;
    wave_sync();
}

__device__ __forceinline__ void wp_window(WpLds &W, int slot, float *d, int lane)
{
    constexpr int N = 200;
    constexpr int kMaxPeaks = 12; /* maxima are at least 25 samples apart: at most 8 in 200 samples */
    const int nom = W.nom[slot];
    const int *pos = W.pos[slot];
    const float eps = (float)0.2;
    const float lowVal = (float)((double)(1 - eps) / 2.0), highVal = (float)((double)(1 + eps) / 2.0);
    /* the peak list once into registers (one LDS round trip instead of one per peak and round); entries beyond the
     * list sit past every sample */
    int pk[kMaxPeaks];
#pragma unroll
    for (int c = 0; c < kMaxPeaks; ++c) pk[c] = (c < nom) ? pos[c] : (1 << 20);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = lane + 64 * k;
        if (j < N) {
            /* the raised segments [pos_i - 4, pos_i - 4 + ceil(0.8 gap_i)) are ordered and disjoint: the only
             * one that can hold j is the last one starting at or before j */
            bool high = false;
            if (nom > 1) {
                int cnt = 0;
#pragma unroll
                for (int c = 0; c < kMaxPeaks; ++c) cnt += (pk[c] - 4 <= j) ? 1 : 0;
                if (cnt > 0) {
                    const int i = cnt - 1;
                    const int gap = (i < nom - 1) ? (pos[i + 1] - pos[i]) : (pos[nom - 1] - pos[nom - 2]);
                    high = j < pos[i] - 4 + (80 * gap + 99) / 100;
                }
            }
            W.tw[j] = high ? highVal : lowVal;
        }
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        if (i < N) d[i] *= (W.tw[i] + W.tw[i < N - 1 ? i + 1 : N - 1]);
    }
    wave_sync();
}

} // namespace

/* frames per tile of afe_ceps_kernel: 8 (same-box A/B of the feature pass: 16 frames 3.71 ms, 8 frames 3.05 ms -- half the
 * LDS per wave, 15.6 instead of 25 KB, lets the CU hold the eight waves its registers allow instead of six; compceps_kernel
 * itself is fastest with 16: 0.715 ms against 0.77-0.79 with 8 and 1.42 with 4) */
constexpr int kAfeT = 8;

} // namespace sea
