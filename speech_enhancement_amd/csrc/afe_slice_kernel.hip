/*
 * afe_slice_kernel.hip -- the feature chain over one TIME SLICE of every utterance, both rates, gfx950 (MI355X)
 * (include/sea_mi355x.h, sea_afe_features_batch_slice / sea_wb_afe_features_batch_slice; the states' layouts: sea_kernels.h,
 * kAfeStateFloats / kWbAfeStateFloats).
 *
 * Both kernels of the one-launch chain have a form here that can start in the middle of an utterance: afe_ceps_kernel
 * (cc_kernel.hip) / afe_wb_ceps_kernel (afe_wb_kernel.hip), and afe_vad_kernel / afe_wb_vad_kernel (cc_kernel.hip).  Those
 * units stay as they are -- whatever joins them moves the register allocation of measured kernels.  One template <bool WB>
 * body serves each pair of rates here; the tile and WaveProc come from cc_tile.h / cc_waveproc.h, PostProc + VAD from afe_vad.h,
 * the span, the row staging and the carry from cc_slice.h (which also says what completes in a slice).  The rates differ in the
 * argument struct, the state's offsets, the frame's samples, where the float stream and a frame's flag byte lie, and the
 * wideband high-band and code rows: AfeSliceRate<WB> and `if constexpr (WB)` say where.
 *
 * What is carried, and who stores it.  The tile kernels stride over the slice's tiles with many workgroups per utterance, so
 * they only READ the state; the VAD kernels, one wave per utterance and the slice's last launch, read PostProc's and the VAD's
 * recursion, run the slice, and then write every part of the state for the next slice.
 */
#undef SEA_CC_TIMING /* the tile's timing diagnostic is compceps_kernel's (cc_kernel.hip) */
#include "cc_tile.h"
#include "cc_waveproc.h"
#include "cc_slice.h"
#include "afe_vad.h"

namespace sea {

namespace {
/* what a rate's slice form reads where: its arguments and its state's offsets (sea_kernels.h) */
template <bool WB> struct AfeSliceRate;
template <> struct AfeSliceRate<false> {
    using Args = AfeSliceArgs;
    static constexpr int kFloats = kAfeStateFloats, kF32 = kAf8StF32, kRing = kAf8StRing, kLane = kAf8StLane, kScal = kAf8StScal;
    static constexpr int kHop = SEA_HOP;
    static __device__ __forceinline__ const AfeArgs &afe(const Args &s) { return s.a; }
};
template <> struct AfeSliceRate<true> {
    using Args = WbAfeSliceArgs;
    static constexpr int kFloats = kWbAfeStateFloats, kF32 = kAfStF32, kRing = kAfStRing, kLane = kAfStLane, kScal = kAfStScal;
    static constexpr int kHp = kAfStHp, kCode = kAfStCode;
    static constexpr int kHop = SEA_WB_HOP;
    static __device__ __forceinline__ const AfeArgs &afe(const Args &s) { return s.w.a; }
};

template <bool WB>
__device__ __forceinline__ SliceSpan afe_slice_span(const typename AfeSliceRate<WB>::Args &s, int u)
{
    const AfeArgs &a = AfeSliceRate<WB>::afe(s);
    return slice_span(a.first_out[u], a.lengths[u] / AfeSliceRate<WB>::kHop, s.frame_base);
}

/* afe_ceps_kernel / afe_wb_ceps_kernel over the cepstral frames that complete in the slice: row r of the slice's feat_cc block
 * of utterance u is cepstral frame jLo + r.  Samples and rows from before the slice come from the state (zeros where
 * resume == 0); Data[-1] of the UTTERANCE's first cepstral frame is zero, whichever slice it falls into.  Rows behind the slice's
 * count are left alone: the capacity of a slice is its frames, not what the utterance may still produce. */
template <bool WB>
__device__ __forceinline__ void afe_ceps_slice_body(const typename AfeSliceRate<WB>::Args &s, CcTileLds<false, kAfeT> &L, WpLds &W,
                                                    CcWbLds *X = nullptr, float *hpS = nullptr, float *codeS = nullptr)
{
    using R = AfeSliceRate<WB>;
    const AfeArgs &a = R::afe(s);
    const int lane = threadIdx.x;
    const bool resume = s.resume != 0;
    CcTileConst C;
    load_cc_tile_const<false, kAfeT>(C, L, a.tables, lane);
    if constexpr (WB) {
        for (int i = lane; i < SEA_WB_NCHAN * 16; i += kLanes) X->dct26T[i] = s.w.wb->dct26T[i >> 4][i & 15];
        wave_sync();
    }
    const long long nslot = a.ceps_cum[a.n_utt] / kAfeT + a.n_utt; /* tile slots as in the one launch */
    for (long long sl = blockIdx.x; sl < nslot; sl += gridDim.x) {
        int lo = 0, hi = a.n_utt;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ceps_cum[mid] / kAfeT + mid <= sl) lo = mid; else hi = mid;
        }
        const int u = lo;
        const long long c0 = a.ceps_cum[u], cap = a.ceps_cum[u + 1] - c0;
        const long long j0 = (sl - (c0 / kAfeT + u)) * kAfeT; /* the tile's first row of the slice's block */
        if (j0 >= cap) continue;
        const SliceSpan p = afe_slice_span<WB>(s, u);
        const int nrow = (int)((cap - j0 < kAfeT) ? cap - j0 : kAfeT);
        const long long left = p.nc - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        if (nv <= 0) continue;
        const float *st = s.state + (size_t)u * R::kFloats;
        const long long jA = p.jLo + j0;                      /* the tile's first cepstral frame, absolute */
        const int r0 = (int)(p.f0 + jA - s.frame_base);       /* its frame within the slice: >= -2 */
        float *dst = a.feat_cc + (c0 + j0) * SEA_CC_NCEP;
        /* Data[-1..199] of the tile's frame f = the float stream from the slice's sample 80 (r0 + f) - 1 on, staged as in the
         * one launch; what lies before the slice's first sample is the state's last three frames */
        const float *cur0 = a.den_f32 + (WB ? a.offsets[u] / 2 : a.offsets[u]);
        const int s0 = r0 * SEA_HOP - 1;
        const bool first = jA == 0;
        constexpr int kAfeBatch = 13;
        constexpr int kIter = (kAfeT * 201 + kLanes - 1) / kLanes; /* 51 */
#pragma unroll 1
        for (int b0 = 0; b0 < kIter; b0 += kAfeBatch) {
            float sv[kAfeBatch];
#pragma unroll
            for (int k = 0; k < kAfeBatch; ++k) {
                const int i = lane + kLanes * (b0 + k);
                const int f = i / 201, x = i - f * 201;
                const int loc = s0 + SEA_HOP * f + x; /* -161 <= loc < 80 nfr */
                float v = 0.0f;
                if (i < nv * 201 && !(x == 0 && f == 0 && first)) v = slice_sample(cur0, st + R::kF32, loc, resume);
                sv[k] = v;
            }
#pragma unroll
            for (int k = 0; k < kAfeBatch; ++k) {
                const int i = lane + kLanes * (b0 + k);
                if (i < nv * 201) L.span[i] = sv[k];
            }
        }
        if constexpr (WB)
            stage_wb_rows(hpS, codeS, s.w.hp_rows, s.w.code_rows, (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP, r0, nv,
                          st + R::kHp, st + R::kCode, resume, lane);
        wave_sync();
        float energy = 0.0f; /* WaveProc.c:423-427, lane = frame */
        if (lane < nv) {
            const float *q = L.span + 201 * lane;
#pragma unroll 8
            for (int x = 1; x < 201; ++x) {
                const float v = q[x];
                energy += v * v;
            }
        }
        const unsigned long long pass = __ballot(lane < nv && (double)energy >= 100.0);
        for (int g = 0; g < nv; g += 4) { /* four frames at a time: their peak searches run side by side */
            const unsigned m4 = (unsigned)(pass >> g) & 0xfu;
            if (m4 == 0) continue;
            for (int r = 0; r < 4; ++r)
                if ((m4 >> r) & 1u) wp_smooth(W, r, L.span + 201 * (g + r) + 1, lane);
            wp_peaks4(W, m4, lane);
            for (int r = 0; r < 4; ++r)
                if ((m4 >> r) & 1u) wp_window(W, r, L.span + 201 * (g + r) + 1, lane);
        }
        wave_sync();
        if constexpr (WB)
            cc_tile<false, kAfeT, true>(L, C, nv, dst, lane, X, hpS, codeS, s.w.wb);
        else
            cc_tile<false, kAfeT>(L, C, nv, dst, lane);
    }
}

/* afe_vad_kernel / afe_wb_vad_kernel (cc_kernel.hip, afe_vad_body<WB>) over one slice: the null vectors of the slice's frames
 * before the onset, DoPostProc + DoVADProc on the cepstral frames that completed in it, DoVADFlush where the utterance ends with
 * it -- from where the previous slice left weightLMS, FeatureBuffer, the ring and the counters.  out / cc / pp are the slice's
 * blocks; the speech flag of cepstral frame j is the byte of frame f0 + j + 2, always a frame of this slice.  keep: kAfStKeep
 * floats, at the wideband rate kCarryRows more.  lane = feature index. */
template <bool WB>
__device__ __forceinline__ void afe_vad_slice_body(const typename AfeSliceRate<WB>::Args &s, float (&ring)[7][16], float *keep)
{
    using R = AfeSliceRate<WB>;
    const AfeArgs &a = R::afe(s);
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    float *st = s.state + (size_t)u * R::kFloats;
    const bool resume = s.resume != 0;
    const SliceSpan p = afe_slice_span<WB>(s, u);
    const long long fb = s.frame_base, nfr = p.nfr, nceps = p.nc;
    /* the slice's frames with an absolute index below the onset (a.onset: "frames so far" while there is none) */
    long long nnull = (long long)a.onset[u] - fb;
    nnull = nnull < 0 ? 0 : (nnull < nfr ? nnull : nfr);
    float *out = a.feat15 + a.feat_cum[u] * 15;
    const float *cc = a.feat_cc + a.ceps_cum[u] * SEA_CC_NCEP;
    float *pp = a.feat_pp ? a.feat_pp + a.ceps_cum[u] * SEA_CC_NCEP : nullptr;
    const long long row0 = WB ? (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP : 0; /* the utterance's first row of the slice's */
    constexpr int kFlagStep = WB ? 1 : 10; /* bytes between the flags of two frames */
    /* the flag of the slice's r-th completing frame: the slice's frame f0 + jLo + 2 - fb + r */
    const unsigned char *flg = a.flags + (WB ? row0 : a.offsets[u] / 8) + kFlagStep * (p.f0 >= 0 ? (long long)p.f0 + p.jLo + 2 - fb : 0);
    long long nemit = 0;

    for (long long k = 0; k < nnull; ++k) { /* null MFCC vectors, VAD = NON_SPEECH */
        if (lane < 15) out[nemit * 15 + lane] = 0.0f;
        nemit++;
    }
    if (lane < 16)
#pragma unroll
        for (int r = 0; r < 7; ++r) ring[r][lane] = resume ? st[R::kRing + r * 16 + lane] : 0.0f;
    wave_sync();

    AfeVad v;
    int nullsSoFar = 0, flushed = 0; /* running totals for the state's diagnostic words: nothing below reads them */
    if (resume) {
        if (lane < 16) {
            v.wLMS = st[R::kLane + lane];
            v.feat = st[R::kLane + 16 + lane];
        }
        v.focus = __float_as_int(st[R::kScal + 0]);
        v.hangOver = __float_as_int(st[R::kScal + 1]);
        v.hCount = __float_as_int(st[R::kScal + 2]);
        v.vCount = __float_as_int(st[R::kScal + 3]);
        v.frameCounter = __float_as_int(st[R::kScal + 4]);
        nullsSoFar = __float_as_int(st[R::kScal + 6]);
        flushed = __float_as_int(st[R::kScal + 7]);
        v.focus = (v.focus >= 0 && v.focus < 7) ? v.focus : 0; /* the ring's index, whatever the caller's state holds */
    }
    const float tgt = afe_postproc_target(lane);
    const float lambda = kPostProcLambda;

    auto decide = [&](int fc) { afe_vad_decide(v, ring, fc, lane); };

    /* rows and flag bytes are requested kAhead frames before use: the loop body is a few dozen
     * instructions, an HBM round trip a few thousand clocks */
    constexpr int kAhead = 8;
    float rowQ[kAhead];
    int bitQ[kAhead];
    auto fetch = [&](long long r, float &row, int &bits) {
        const long long rr = r < nceps ? r : (nceps > 0 ? nceps - 1 : 0);
        row = (lane < 14 && nceps > 0) ? cc[rr * SEA_CC_NCEP + lane] : 0.0f;
        bits = (nceps > 0) ? (int)flg[kFlagStep * rr] : 0;
    };
#pragma unroll
    for (int q = 0; q < kAhead; ++q) fetch(q, rowQ[q], bitQ[q]);
    for (long long q0 = 0; q0 < nceps; q0 += kAhead) {
#pragma unroll
      for (int q = 0; q < kAhead; ++q) {
        const long long r = q0 + q; /* row of the slice; cepstral frame jLo + r of the utterance */
        if (r >= nceps) break;
        /* PostProc on c1..c12; the weighting comes from logE = Coef[13] (Noc0 == 0) */
        const float c = rowQ[q];
        const int bits = bitQ[q];
        fetch(r + kAhead, rowQ[q], bitQ[q]);
        const float logE = __shfl(c, 13, 64);
        float wp = (logE * (float)64 - (float)211) / (float)64;
        wp = (wp < 0) ? 0.0f : ((wp > 1) ? lambda : wp * lambda);
        float x = c;
        if (lane < 12) {
            const float dif = ((c - v.wLMS) - tgt);
            x = c - v.wLMS;
            v.wLMS += dif * wp;
        }
        if (pp && lane < 14) pp[r * SEA_CC_NCEP + lane] = x;
        if (lane < 14) v.feat = x;
        /* DoVADProc */
        v.frameCounter = (int)(p.jLo + r) + 5; /* nbFrame[0] when NoiseSup output j+3 appears */
        v.focus = (v.focus + 1 == 7) ? 0 : v.focus + 1;
        if (lane < 14) ring[v.focus][lane] = v.feat;
        if (lane == 14) ring[v.focus][14] = bits ? 1.0f : 0.0f;
        wave_sync();
        if (v.frameCounter > 10) {
            decide(v.frameCounter);
            if (lane < 15) out[nemit * 15 + lane] = v.feat;
            nemit++;
        }
        wave_sync();
      }
    }
    /* FlushAdvProcess until DoVADFlush returns FALSE: only where the utterance ends with this slice */
    if (s.final && s.final[u]) {
        const int flushFocus = v.focus;
        for (;;) {
            int nf = v.focus + 1;
            nf = (nf == 7) ? 0 : nf;
            if (nf == flushFocus) break;
            v.focus = nf;
            v.frameCounter++;
            if (v.frameCounter > 10) decide(v.frameCounter);
            if (lane < 15) out[nemit * 15 + lane] = v.feat;
            nemit++;
        }
        flushed = 1;
    }
    if (lane == 0) {
        a.n_feat[u] = (int)nemit;
        if (a.n_ceps) a.n_ceps[u] = (int)nceps; /* here, not in the tile pass: a slice without a frame launches no tile */
    }

    /* the state for the next slice */
    carry_load(keep, a.den_f32 + (WB ? a.offsets[u] / 2 : a.offsets[u]), st + R::kF32, nfr, resume, lane);
    if constexpr (WB) carry_load_rows(keep, s.w.hp_rows, s.w.code_rows, row0, nfr, st + R::kHp, st + R::kCode, resume, lane);
    __syncthreads();
    carry_store(st + R::kF32, keep, lane);
    if constexpr (WB) carry_store_rows(st + R::kHp, st + R::kCode, keep, lane);
    if (lane < 16)
#pragma unroll
        for (int r = 0; r < 7; ++r) st[R::kRing + r * 16 + lane] = ring[r][lane];
    if (lane < 16) {
        st[R::kLane + lane] = v.wLMS;
        st[R::kLane + 16 + lane] = v.feat;
    }
    if (lane == 0) {
        st[R::kScal + 0] = __int_as_float(v.focus);
        st[R::kScal + 1] = __int_as_float(v.hangOver);
        st[R::kScal + 2] = __int_as_float(v.hCount);
        st[R::kScal + 3] = __int_as_float(v.vCount);
        st[R::kScal + 4] = __int_as_float(v.frameCounter);
        st[R::kScal + 5] = __int_as_float((int)(p.jLo + nceps));
        st[R::kScal + 6] = __int_as_float(nullsSoFar + (int)nnull);
        st[R::kScal + 7] = __int_as_float(flushed);
    }
}
} // namespace

/* LDS: the one launch's tile + WaveProc's -> two waves per SIMD as afe_wb_ceps_slice_kernel */
__global__ __launch_bounds__(64, 2) void afe_ceps_slice_kernel(AfeSliceArgs s)
{
    __shared__ CcTileLds<false, kAfeT> L;
    __shared__ WpLds W;
    afe_ceps_slice_body<false>(s, L, W);
}

/* LDS: the one launch's 19312 bytes + 384 for the tile's staged rows -> still eight waves in a CU's 160 KB */
__global__ __launch_bounds__(64, 2) void afe_wb_ceps_slice_kernel(WbAfeSliceArgs s)
{
    __shared__ CcTileLds<false, kAfeT> L;
    __shared__ WpLds W;
    __shared__ CcWbLds X;
    __shared__ float hpS[kAfeT * 3], codeS[kAfeT * 9];
    afe_ceps_slice_body<true>(s, L, W, &X, hpS, codeS);
}

__global__ __launch_bounds__(64) void afe_vad_slice_kernel(AfeSliceArgs s)
{
    __shared__ float ring[7][16];
    __shared__ float keep[kAfStKeep];
    afe_vad_slice_body<false>(s, ring, keep);
}

__global__ __launch_bounds__(64) void afe_wb_vad_slice_kernel(WbAfeSliceArgs s)
{
    __shared__ float ring[7][16];
    __shared__ float keep[kAfStKeep + kCarryRows];
    afe_vad_slice_body<true>(s, ring, keep);
}

} // namespace sea
