/*
 * cc_tile.h -- the tiled CompCeps shared by the kernels of cc_kernel.hip and afe_wb_kernel.hip: a wave's tile of frames in LDS
 * -> rows of 14 coefficients.  Internal to the library; every including unit gets its own copy (anonymous namespace).
 */
#pragma once
#include "ns_core.h" /* the kernels' own double log and its guard (ns_ln, ns_near_float_boundary, ns_ln_cr) */

namespace sea {

/* ==================================================================================================
 * Tiled CompCeps: one wave owns a TILE of kCcT consecutive frames.
 *
 * A one-frame-per-wave form (round 1: 2.5 ms for 810 511 frames) spends most of its time on work that every one of
 * its 64 lanes repeats: the frame's 200-term in-order energy sum (CompCeps.c:413-423) and its double-precision log.
 * Here the tile's samples are staged in LDS once and
 *   * the energy sums run LANE = FRAME (lane f adds the 200 squares of frame f in order; the hop
 *     blocks sit 81 words apart -- one pad word per 80 samples -- so the 16 lanes hit 16 banks),
 *     and the log of the sum is evaluated once per frame, again lane = frame;
 *   * two frames at a time go through the dual transform (lanes 0..31 / 32..63, swizzled work area,
 *     five LDS round trips instead of six), their power spectra and the 23 mel triangles (lane =
 *     (frame, band));
 *   * the 23 log energies of all frames are taken lane = (frame, band) flattened (6 evaluations of the
 *     double log per tile instead of 16), the DCT lane = (frame, coefficient) flattened (4 passes).
 * Arithmetic per value is WI8CompCeps' (CompCeps.c:368-549), operation by operation: pre-emphasis in double
 * (:427-429), power spectrum products and sum in double (:451-459), taps / DCT terms in their order.  Zero-weight taps stand in for the band length test (acc + p * 0 == acc: p is a
 * finite power, acc >= +0) and c0's plain sum is a DCT row of ones (x * 1.0f == x).
 * ================================================================================================ */
namespace {

constexpr int kCcT = 16; /* frames per tile of compceps_kernel (afe_ceps_kernel: kAfeT) */

/* (float)log((double)v) for a positive normal float v, as CompCeps.c:423 / :511 take it.  The library's double log
 * costs ~150 instructions; the kernels' own table-driven one with its rounding-boundary guard (ns_core.h, ns_logf) */
template <bool NF = false> /* NF: the frames are the caller's floats (compceps_frames_kernel): Inf and NaN as libm gives them */
__device__ __forceinline__ float cc_logf(float v) { return ns_logf<NF>(v); }

template <bool SHARED, int T = kCcT>
struct CcGeom {
    /* SHARED: frames of one utterance, 80 samples apart, share their samples; word x of the span (x = 0 is
     * Data[-1] of the tile's first frame) sits at x + x / 80.  Otherwise: kCcT separate frames of 201 floats. */
    static constexpr int FS = SHARED ? 81 : 201;
    static constexpr int SPAN = SHARED ? 81 * (T - 1) + 204 : 201 * T;
};

template <bool SHARED, int T = kCcT>
struct __attribute__((aligned(16))) CcTileLds {
    float span[(CcGeom<SHARED, T>::SPAN + 3) & ~3];
    float work[512];                  /* the dual transform's work area; after the tile's last pair, its T x 14 output rows */
    float pw[2][SEA_CC_PWROW];        /* 129 power bins per frame, zeros behind (the mel taps read past 128) */
    float fb[T][24];
    float dctT[SEA_CC_NCHAN * 16];
};

struct CcTileConst {
    Fft2Regs fft;
    float win8[8];
    int qd[8], qm[8];                 /* word offsets of Data[idx], Data[idx-1] from the frame's base; qd < 0: idx >= 200 */
    int pwAB, pwCD;                   /* words from the pair's first power row: bins j (+ 64) and 64 - j (+ 64) of this lane's
                                         last-level item (rfft256_dual_keep_last), row of its transform */
    bool pairLane;                    /* the item with bins 0, 64, 128 | 32, 96 */
    int melBase, melFb;               /* this lane's (frame, band) of the mel pass: sea_tables.h, melLaneBase */
    float melW[SEA_CC_TAPS2];
    float floorFB, floorE;
};

template <bool SHARED>
__device__ __forceinline__ int cc_q(int x) /* word offset of Data[x-1] within its frame, x = 0..200 */
{
    return SHARED ? x + (x >= 80 ? 1 : 0) + (x >= 160 ? 1 : 0) : x;
}

template <bool SHARED, int T = kCcT>
__device__ __forceinline__ void load_cc_tile_const(CcTileConst &C, CcTileLds<SHARED, T> &L, const sea_cc_tables *t, int lane)
{
    load_fft2_regs<false>(C.fft, &t->fft, lane, nullptr);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        constexpr int kRev3[8] = {0, 4, 2, 6, 1, 5, 3, 7};
        const int idx = (lane & 31) + 32 * kRev3[k];
        C.win8[k] = t->win8[k][lane];
        C.qd[k] = (idx < SEA_WIN) ? cc_q<SHARED>(idx + 1) : -1;
        C.qm[k] = (idx < SEA_WIN) ? cc_q<SHARED>(idx) : 0;
    }
    {
        const unsigned item = t->fft.fft2Item[SEA_FFT_LSTAGES - 1][lane & 31];
        C.pairLane = (item >> 16) == SEA_BF_PAIR;
        const int ja = (int)(item & 255u), jc = C.pairLane ? (int)((item >> 8) & 255u) : ja; /* j, j | 0, 32 */
        C.pwAB = SEA_CC_PWROW * (lane >> 5) + ja;
        C.pwCD = SEA_CC_PWROW * (lane >> 5) + 64 - jc;
    }
    C.melBase = t->melLaneBase[lane];
    C.melFb = t->melLaneFb[lane];
#pragma unroll
    for (int i = 0; i < SEA_CC_TAPS2; ++i) C.melW[i] = t->melLaneW[i][lane];
    C.floorFB = t->floorFB;
    C.floorE = t->floorE;
    for (int i = lane; i < SEA_CC_NCHAN * 16; i += kLanes) L.dctT[i] = t->dctT[i >> 4][i & 15];
    for (int i = lane; i < 2 * SEA_CC_PWROW; i += kLanes) (&L.pw[0][0])[i] = 0.0f;
    wave_sync();
}

/* timing-only diagnostic (-DSEA_CC_TIMING, tools/cc_phases.py): shader clocks workgroup 0 of compceps_kernel spends per step of a tile */
#ifdef SEA_CC_TIMING
__device__ unsigned long long g_cc_ck[8];
extern "C" int sea_cc_timing(unsigned long long *out8, int reset)
{
    if (reset) {
        unsigned long long z[8] = {};
        return hipMemcpyToSymbol(HIP_SYMBOL(g_cc_ck), z, sizeof z) != hipSuccess;
    }
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_cc_ck), 8 * sizeof(unsigned long long)) != hipSuccess;
}
__device__ unsigned g_cc_wave[16384 * 4]; /* per wave of compceps_kernel: start, end (constant 100 MHz counter), HW_ID, XCC_ID */
extern "C" int sea_cc_waves(unsigned *out, int n) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cc_wave), (size_t)n * 4 * sizeof(unsigned)) != hipSuccess; }
#define CC_CK_START unsigned long long cck_ = clock64()
#define CC_CK(k) do { const unsigned long long c_ = clock64(); if (SHARED && blockIdx.x == 0 && threadIdx.x == 0) g_cc_ck[k] += c_ - cck_; cck_ = c_; } while (0)
#else
#define CC_CK_START
#define CC_CK(k)
#endif

/* the wideband mode's additions to a tile (cc_tile<.., WB = true>) */
struct __attribute__((aligned(16))) CcWbLds {
    float dec[kCcT][4];               /* GetBandsForDecoding16k's three sums per frame */
    float fbx[kCcT][4];               /* log band energies 23..25 (the frame's row of fb has 24 columns) */
    float dct26T[SEA_WB_NCHAN * 16];
};

/* the staged tile -> nv rows of 14 coefficients at dst.
 * WB: the wideband mode (CompCeps.c:392-402, :464-479, :488-530).  X = the additions' LDS; hpRows / codeRows = the tile's first
 * frame's rows of high-band energies (after the spectral subtraction) and code values: cepstral frame j of an utterance is
 * computed after NoiseSup output j + 2 and reads the heads of the three-deep queues hpBands / bufferCodeForBands16k, the
 * entries of output j (NoiseSup.c:1418-1428).  logE is taken after CorrectEnergy, not before. */
template <bool SHARED, int T = kCcT, bool WB = false, bool NF = false /* see cc_logf */>
__device__ __forceinline__ void cc_tile(CcTileLds<SHARED, T> &L, const CcTileConst &C, int nv, float *dst, int lane,
                                        CcWbLds *X = nullptr, const float *hpRows = nullptr, const float *codeRows = nullptr,
                                        const sea_wb_tables *wbt = nullptr)
{
    constexpr int FS = CcGeom<SHARED, T>::FS;
    /* logE (CompCeps.c:413-423): lane f sums the squares of frame f in sample order */
    float logE; /* three ranges of the walk, each with a constant pad */
    CC_CK_START;
    {
        const float *p = L.span + FS * (lane & (T - 1));
        float acc = 0.0f;
        if (lane < T) {
            if (SHARED) {
#pragma unroll 8
                for (int x = 1; x < 80; ++x) { const float v = p[x]; acc += v * v; }
#pragma unroll 8
                for (int x = 80; x < 160; ++x) { const float v = p[x + 1]; acc += v * v; }
#pragma unroll 8
                for (int x = 160; x < 201; ++x) { const float v = p[x + 2]; acc += v * v; }
            } else {
#pragma unroll 8
                for (int x = 1; x < 201; ++x) { const float v = p[x]; acc += v * v; }
            }
        }
        if (WB) logE = acc;
        else logE = (acc < C.floorE) ? (float)-50.0 : cc_logf<NF>(acc); /* a NaN goes INTO the log, as in the reference */
    }
    CC_CK(1);
    const int npair = (nv + 1) >> 1;
    for (int pr = 0; pr < npair; ++pr) {
        const int h = lane >> 5;
        const int f = 2 * pr + h;
        const bool act = f < nv;
        const float *p = L.span + FS * f;
        /* pre-emphasis in double (:427-429), symmetric Hamming (:115-125), zero padding (:439-440) */
        float e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = 0.0f;
            if (act && C.qd[k] >= 0) {
                const float d = p[C.qd[k]], dm1 = p[C.qm[k]];
                v = (float)((double)d - 0.90 * (double)dm1) * C.win8[k];
            }
            e[k] = v;
        }
        /* the transform's last level stays in registers: every lane holds four complete bins of its frame (one lane per frame
         * five), whose power -- products and sum in double (:451-459) -- goes straight to the frame's row */
        float o[8];
        bool nfPower = false;
        rfft256_dual_keep_last<false>(e, L.work, C.fft, o);
        {
            const bool pl = C.pairLane;
            const float ia = pl ? 0.0f : o[7], ib = pl ? o[3] : o[6], ic = pl ? o[7] : o[3], id = pl ? o[6] : o[2];
            auto power = [](float re, float im) { return (float)((double)re * (double)re + (double)im * (double)im); };
            float *rowAB = &L.pw[0][0] + C.pwAB, *rowCD = &L.pw[0][0] + C.pwCD;
            rowAB[0] = power(o[0], ia);   /* bin j | 0: (float)(re * re + 0.0) == (float)(re * re) */
            rowAB[64] = power(o[1], ib);  /* bin 64 + j | 64 */
            rowCD[0] = power(o[4], ic);   /* bin 64 - j | 32 */
            rowCD[64] = power(o[5], id);  /* bin 128 - j | 96 */
            if (pl) rowAB[128] = power(o[2], 0.0f); /* bin 128 */
            if constexpr (NF) /* (a separate statement: the lines above compile as they did without it) */
                nfPower = ns_nonfinite(power(o[0], ia)) || ns_nonfinite(power(o[1], ib)) || ns_nonfinite(power(o[4], ic)) ||
                          ns_nonfinite(power(o[5], id)) || (pl && ns_nonfinite(power(o[2], 0.0f)));
        }
        /* NF (the caller's floats): a power of this pair of frames is Inf or NaN (wave-uniform) */
        const bool skipZeroTaps = NF && __ballot(nfPower) != 0ull;
        wave_sync();
        if (WB && lane < 6) { /* GetBandsForDecoding16k (16kHzProcessing.c:317-336) from the power spectrum, before the mel pass */
            const int hh = lane / 3, b = lane - 3 * hh;
            if (2 * pr + hh < nv) {
                const float *row = &L.pw[hh][0];
                const int b0 = b == 0 ? 66 : (b == 1 ? 78 : 98), b1 = b == 0 ? 77 : (b == 1 ? 97 : 129);
                float sum = 0.0f;
                for (int i = b0; i < b1; ++i) sum += row[i];
                X->dec[2 * pr + hh][b] = sum * 0.5f; /* /= 2.0 */
            }
        }
        /* 23 mel triangles (DoMelFB, MelProc.c:82-104): lane = one (frame, band) of the pair, dealt so that the aligned
         * pairs the lanes of a group read lie on different banks (round 4: 3-way conflicts on every tap before) */
        if (C.melFb >= 0 && 2 * pr + (C.melFb >= 24 ? 1 : 0) < nv) {
            const float2 *q = reinterpret_cast<const float2 *>(&L.pw[0][0] + C.melBase);
            float acc = 0.0f;
            if (NF && skipZeroTaps) {
                /* Inf * 0 must not reach a band from a tap in front of or behind it, as it does not in the reference's loop over
                 * the band's own length: zero-weight taps are skipped (none lies INSIDE a band: sea_tables.c refuses such a table) */
#pragma unroll
                for (int i = 0; i < SEA_CC_TAPS2 / 2; ++i) {
                    const float2 v = q[i];
                    const float w0 = C.melW[2 * i], w1 = C.melW[2 * i + 1];
                    acc = (w0 == 0.0f) ? acc : acc + v.x * w0;
                    acc = (w1 == 0.0f) ? acc : acc + v.y * w1;
                }
            } else {
#pragma unroll
                for (int i = 0; i < SEA_CC_TAPS2 / 2; ++i) {
                    const float2 v = q[i];
                    acc = acc + v.x * C.melW[2 * i];
                    acc = acc + v.y * C.melW[2 * i + 1];
                }
            }
            (&L.fb[2 * pr][0])[C.melFb] = acc;
        }
        wave_sync();
    }
    CC_CK(2);
    /* natural log with floor (:509-513): lane = (frame, band) flattened */
    for (int idx = lane; idx < nv * SEA_CC_NCHAN; idx += kLanes) {
        const int f = idx / SEA_CC_NCHAN, b = idx - f * SEA_CC_NCHAN;
        const float v = L.fb[f][b];
        L.fb[f][b] = (v < C.floorFB) ? (float)-10.0 : cc_logf<NF>(v);
    }
    wave_sync();
    CC_CK(3);
    if (WB) { /* lane = frame: the high bands join (the promotions are the reference's: float unless a double constant enters) */
        if (lane < nv) {
            const int f = lane;
            const float *code = codeRows + f * 9, *hpr = hpRows + f * 3;
            const float cw[3] = {(float)0.1, (float)0.2, (float)0.7}; /* codeWeights, CompCeps.c:475-477 */
            float aux[3], hb[3], fbv[3];
            for (int j = 0; j < 3; ++j) { /* :468-473 */
                const float v = X->dec[f][j];
                aux[j] = (v > C.floorFB) ? cc_logf(v) : (float)-10.0;
            }
            for (int i = 0; i < 3; ++i) { /* DecodeBands16k, then the coded bands' pre-emphasis correction (:503-504) */
                float sum = 0.0f;
                for (int j = 0; j < 3; ++j) sum += cw[j] * (aux[j] - code[3 * i + j]);
                hb[i] = sum + wbt->preemLog;
            }
            for (int i = 0; i < 3; ++i) { /* the subtracted bands (:497-498), log with floor (:509-513) */
                const float v = (float)((1.0 + 0.90) * (double)hpr[i]);
                fbv[i] = (v < C.floorFB) ? (float)-10.0 : cc_logf(v);
            }
            const float percCoded = (float)0.7; /* MergeSSandCoded, 16kHzProcessing.c:106-125 */
            for (int i = 0; i < 3; ++i) fbv[i] = (float)((double)(percCoded * hb[i]) + (1.0 - (double)percCoded) * (double)fbv[i]);
            float f22 = L.fb[f][SEA_CC_NCHAN - 1];
            const float avg = (float)(0.5 * (double)f22 + 0.5 * (double)fbv[0]);
            f22 = (float)(0.6 * (double)f22 + 0.4 * (double)avg);
            fbv[0] = (float)(0.6 * (double)fbv[0] + 0.4 * (double)avg);
            L.fb[f][SEA_CC_NCHAN - 1] = f22;
            float energyHP = 0.0f; /* CorrectEnergy, :145-158 */
            for (int i = 0; i < 3; ++i) {
                X->fbx[f][i] = fbv[i];
                energyHP = (float)((double)energyHP + exp((double)(fbv[i] - wbt->preemLogF)));
            }
            logE += energyHP;
            logE = (logE < C.floorE) ? (float)-50.0 : cc_logf(logE); /* CompCeps.c:526-529 */
        }
        wave_sync();
    }
    /* DCT (:203-227): lane = (frame, coefficient) flattened; c = 12 is c0, logE goes to c = 13 */
    for (int idx = lane; idx < nv * 13; idx += kLanes) {
        const int f = idx / 13, c = idx - f * 13;
        float acc = 0.0f;
        if (WB) {
#pragma unroll
            for (int j = 0; j < SEA_CC_NCHAN; ++j) acc += L.fb[f][j] * X->dct26T[j * 16 + c];
#pragma unroll
            for (int j = 0; j < SEA_WB_NHP; ++j) acc += X->fbx[f][j] * X->dct26T[(SEA_CC_NCHAN + j) * 16 + c];
        } else {
#pragma unroll
            for (int j = 0; j < SEA_CC_NCHAN; ++j) acc += L.fb[f][j] * L.dctT[j * 16 + c];
        }
        L.work[f * SEA_CC_NCEP + c] = acc;
    }
    if (lane < nv) L.work[lane * SEA_CC_NCEP + 13] = logE;
    wave_sync();
    CC_CK(4);
    for (int idx = lane; idx < nv * SEA_CC_NCEP; idx += kLanes) dst[idx] = L.work[idx];
    wave_sync();
    CC_CK(5);
}

} // namespace

} // namespace sea
