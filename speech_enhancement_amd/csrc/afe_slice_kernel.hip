/*
 * afe_slice_kernel.hip -- the 8 kHz feature chain over one TIME SLICE of every utterance, gfx950 (MI355X)
 * (include/sea_mi355x.h, sea_afe_features_batch_slice; the state's layout: sea_kernels.h, kAfeStateFloats).
 *
 * Both kernels of the one-launch chain (cc_kernel.hip: afe_ceps_kernel, afe_vad_kernel) have a form here that can start in the
 * middle of an utterance.  That unit stays as it is -- whatever joins it moves the register allocation of measured kernels -- so
 * the tile and WaveProc are shared through cc_tile.h / cc_waveproc.h and the PostProc + VAD body is restated here statement for
 * statement, as afe_wb_slice_kernel.hip does for the wideband chain.  tests/test_gpu_afe_slices.py holds the two texts together:
 * the slices of an utterance must give the bits of the one launch.
 *
 * What completes in a slice.  Cepstral frame j of an utterance whose first output is frame f0 reads the float stream from sample
 * 80 (f0 + j) - 1 for 201 values, and the VAD takes the speech flag of frame f0 + j + 2 with it: it completes when output frame
 * f0 + j + 2 exists.  A slice of the frames [fb, fb + n) completes j in [max(0, fb - f0 - 2), fb + n - f0 - 2); up to two
 * frames and one sample of the stream lie before the slice and come from the state.
 *
 * What is carried, and who stores it.  afe_ceps_slice_kernel strides over the slice's tiles with many workgroups per utterance,
 * so it only READS the state; afe_vad_slice_kernel, one wave per utterance and the slice's last launch, reads PostProc's and
 * the VAD's recursion, runs the slice, and then writes every part of the state for the next slice.
 */
#undef SEA_CC_TIMING /* the tile's timing diagnostic is compceps_kernel's (cc_kernel.hip) */
#include "cc_tile.h"
#include "cc_waveproc.h"

namespace sea {

namespace {
/* the cepstral frames of utterance u that complete in the slice: [jLo, jLo + nc) */
struct AfeSliceSpan {
    long long nfr, jLo, nc;
    int f0;
};
__device__ __forceinline__ AfeSliceSpan afe_slice_span(const AfeSliceArgs &s, int u)
{
    AfeSliceSpan p;
    p.f0 = s.a.first_out[u];
    p.nfr = s.a.lengths[u] / SEA_HOP;
    p.jLo = 0;
    p.nc = 0;
    if (p.f0 >= 0) {
        const long long fb = s.frame_base;
        p.jLo = fb - p.f0 - 2 > 0 ? fb - p.f0 - 2 : 0;
        const long long jHi = fb + p.nfr - p.f0 - 2;
        p.nc = jHi > p.jLo ? jHi - p.jLo : 0;
    }
    return p;
}
} // namespace

/* afe_ceps_kernel over the cepstral frames that complete in the slice: row r of the slice's feat_cc block of utterance u is
 * cepstral frame jLo + r.  Samples from before the slice come from the state (zeros where resume == 0); Data[-1] of the
 * UTTERANCE's first cepstral frame is zero, whichever slice it falls into.  Rows behind the slice's count are left alone: the
 * capacity of a slice is its frames, not what the utterance may still produce.
 * LDS: the one launch's tile + WaveProc's -> two waves per SIMD as afe_wb_ceps_slice_kernel. */
__global__ __launch_bounds__(64, 2) void afe_ceps_slice_kernel(AfeSliceArgs s)
{
    __shared__ CcTileLds<false, kAfeT> L;
    __shared__ WpLds W;
    const AfeArgs &a = s.a;
    const int lane = threadIdx.x;
    const bool resume = s.resume != 0;
    CcTileConst C;
    load_cc_tile_const<false, kAfeT>(C, L, a.tables, lane);
    const long long nslot = a.ceps_cum[a.n_utt] / kAfeT + a.n_utt; /* tile slots as in afe_ceps_kernel */
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
        const AfeSliceSpan p = afe_slice_span(s, u);
        const int nrow = (int)((cap - j0 < kAfeT) ? cap - j0 : kAfeT);
        const long long left = p.nc - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        if (nv <= 0) continue;
        const float *st = s.state + (size_t)u * kAfeStateFloats;
        const long long jA = p.jLo + j0;                      /* the tile's first cepstral frame, absolute */
        const int r0 = (int)(p.f0 + jA - s.frame_base);       /* its frame within the slice: >= -2 */
        float *dst = a.feat_cc + (c0 + j0) * SEA_CC_NCEP;
        /* Data[-1..199] of the tile's frame f = the float stream from the slice's sample 80 (r0 + f) - 1 on, staged as in
         * afe_ceps_kernel; what lies before the slice's first sample is the state's last three frames */
        const float *cur0 = a.den_f32 + a.offsets[u];
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
                if (i < nv * 201 && !(x == 0 && f == 0 && first)) {
                    if (loc >= 0) v = cur0[loc];
                    else if (resume) v = st[kAf8StF32 + kAfStKeep + loc];
                }
                sv[k] = v;
            }
#pragma unroll
            for (int k = 0; k < kAfeBatch; ++k) {
                const int i = lane + kLanes * (b0 + k);
                if (i < nv * 201) L.span[i] = sv[k];
            }
        }
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
        cc_tile<false, kAfeT>(L, C, nv, dst, lane);
    }
}

/* afe_vad_kernel (cc_kernel.hip, afe_vad_body<false>) over one slice: the null vectors of the slice's frames before the onset,
 * DoPostProc + DoVADProc on the cepstral frames that completed in it, DoVADFlush where the utterance ends with it -- from where
 * the previous slice left weightLMS, FeatureBuffer, the ring and the counters.  out / cc / pp are the slice's blocks; the speech
 * flag of cepstral frame j is the byte of frame f0 + j + 2, always a frame of this slice.  lane = feature index. */
__global__ __launch_bounds__(64) void afe_vad_slice_kernel(AfeSliceArgs s)
{
    __shared__ float ring[7][16];
    __shared__ float keep[kAfStKeep];
    const AfeArgs &a = s.a;
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    float *st = s.state + (size_t)u * kAfeStateFloats;
    const bool resume = s.resume != 0;
    const AfeSliceSpan p = afe_slice_span(s, u);
    const long long fb = s.frame_base, nfr = p.nfr, nceps = p.nc;
    const int f0 = p.f0;
    /* the slice's frames with an absolute index below the onset (a.onset: "frames so far" while there is none) */
    long long nnull = (long long)a.onset[u] - fb;
    nnull = nnull < 0 ? 0 : (nnull < nfr ? nnull : nfr);
    float *out = a.feat15 + a.feat_cum[u] * 15;
    const float *cc = a.feat_cc + a.ceps_cum[u] * SEA_CC_NCEP;
    float *pp = a.feat_pp ? a.feat_pp + a.ceps_cum[u] * SEA_CC_NCEP : nullptr;
    constexpr int kFlagStep = 10; /* bytes between the flags of two frames */
    /* the flag of the slice's r-th completing frame: the slice's frame f0 + jLo + 2 - fb + r */
    const unsigned char *flg = a.flags + a.offsets[u] / 8 + kFlagStep * (f0 >= 0 ? (long long)f0 + p.jLo + 2 - fb : 0);
    long long nemit = 0;

    for (long long k = 0; k < nnull; ++k) { /* null MFCC vectors, VAD = NON_SPEECH */
        if (lane < 15) out[nemit * 15 + lane] = 0.0f;
        nemit++;
    }
    if (lane < 16)
#pragma unroll
        for (int r = 0; r < 7; ++r) ring[r][lane] = resume ? st[kAf8StRing + r * 16 + lane] : 0.0f;
    wave_sync();

    static const float target[12] = {(float)-6.618909, (float)0.198269, (float)-0.740308, (float)0.055132,
                                     (float)-0.227086, (float)0.144280, (float)-0.112451, (float)-0.146940,
                                     (float)-0.327466, (float)0.134571, (float)0.027884,  (float)-0.114905};
    const float tgt = (lane < 12) ? target[lane] : 0.0f;
    const float lambda = (float)0.0087890625;
    float wLMS = 0.0f;   /* weightLMS[lane] */
    float feat = 0.0f;   /* FeatureBuffer[lane]: persists between calls like the reference's buffer */
    int focus = 0, hangOver = 23, hCount = 0, vCount = 0, frameCounter = 0;
    int nullsSoFar = 0, flushed = 0; /* running totals for the state's diagnostic words: nothing below reads them */
    if (resume) {
        if (lane < 16) {
            wLMS = st[kAf8StLane + lane];
            feat = st[kAf8StLane + 16 + lane];
        }
        focus = __float_as_int(st[kAf8StScal + 0]);
        hangOver = __float_as_int(st[kAf8StScal + 1]);
        hCount = __float_as_int(st[kAf8StScal + 2]);
        vCount = __float_as_int(st[kAf8StScal + 3]);
        frameCounter = __float_as_int(st[kAf8StScal + 4]);
        nullsSoFar = __float_as_int(st[kAf8StScal + 6]);
        flushed = __float_as_int(st[kAf8StScal + 7]);
        focus = (focus >= 0 && focus < 7) ? focus : 0; /* the ring's index, whatever the caller's state holds */
    }

    /* trigger = longest run of speech-flagged frames in the ring, scanned from focus+1 round to focus */
    auto decide = [&](int fc) {
        int sum = 0, trigger = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            int r = focus + i + 1;
            r = r > 6 ? r - 7 : r;
            if (ring[r][14] != 0.0f)
                sum++;
            else {
                trigger = sum > trigger ? sum : trigger;
                sum = 0;
            }
        }
        trigger = sum > trigger ? sum : trigger;
        if (trigger >= 4) {
            hCount = hangOver;
            if (fc <= 35) hangOver = 50;
        }
        if (hCount && trigger < 3) hCount--;
        if (trigger >= 3) vCount = 5;
        if (vCount && trigger < 3) vCount--;
        int r = focus + 1;
        r = r > 6 ? r - 7 : r;
        feat = (lane < 15) ? ring[r][lane] : 0.0f;
        if (lane == 14) feat = (vCount || hCount || trigger >= 3) ? 1.0f : 0.0f;
    };

    /* rows and flag bytes are requested kAhead frames before use, as in the one launch */
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
        float v = c;
        if (lane < 12) {
            const float dif = ((c - wLMS) - tgt);
            v = c - wLMS;
            wLMS += dif * wp;
        }
        if (pp && lane < 14) pp[r * SEA_CC_NCEP + lane] = v;
        if (lane < 14) feat = v;
        /* DoVADProc */
        frameCounter = (int)(p.jLo + r) + 5; /* nbFrame[0] when NoiseSup output j+3 appears */
        focus = (focus + 1 == 7) ? 0 : focus + 1;
        if (lane < 14) ring[focus][lane] = feat;
        if (lane == 14) ring[focus][14] = bits ? 1.0f : 0.0f;
        wave_sync();
        if (frameCounter > 10) {
            decide(frameCounter);
            if (lane < 15) out[nemit * 15 + lane] = feat;
            nemit++;
        }
        wave_sync();
      }
    }
    /* FlushAdvProcess until DoVADFlush returns FALSE: only where the utterance ends with this slice */
    if (s.final && s.final[u]) {
        const int flushFocus = focus;
        for (;;) {
            int nf = focus + 1;
            nf = (nf == 7) ? 0 : nf;
            if (nf == flushFocus) break;
            focus = nf;
            frameCounter++;
            if (frameCounter > 10) decide(frameCounter);
            if (lane < 15) out[nemit * 15 + lane] = feat;
            nemit++;
        }
        flushed = 1;
    }
    if (lane == 0) {
        a.n_feat[u] = (int)nemit;
        if (a.n_ceps) a.n_ceps[u] = (int)nceps; /* here, not in the tile pass: a slice without a frame launches no tile */
    }

    /* The state for the next slice.  Element i of the history of 240 is element i + m of (old history, the slice's m new
     * samples): everything is read into LDS first and stored after a barrier. */
    {
        const float *cur = a.den_f32 + a.offsets[u];
        const long long m8 = nfr * SEA_HOP;
        for (int i = lane; i < kAfStKeep; i += kLanes) {
            const long long j = i + m8;
            keep[i] = j >= kAfStKeep ? cur[j - kAfStKeep] : (resume ? st[kAf8StF32 + j] : 0.0f);
        }
    }
    __syncthreads();
    for (int i = lane; i < kAfStKeep; i += kLanes) st[kAf8StF32 + i] = keep[i];
    if (lane < 16)
#pragma unroll
        for (int r = 0; r < 7; ++r) st[kAf8StRing + r * 16 + lane] = ring[r][lane];
    if (lane < 16) {
        st[kAf8StLane + lane] = wLMS;
        st[kAf8StLane + 16 + lane] = feat;
    }
    if (lane == 0) {
        st[kAf8StScal + 0] = __int_as_float(focus);
        st[kAf8StScal + 1] = __int_as_float(hangOver);
        st[kAf8StScal + 2] = __int_as_float(hCount);
        st[kAf8StScal + 3] = __int_as_float(vCount);
        st[kAf8StScal + 4] = __int_as_float(frameCounter);
        st[kAf8StScal + 5] = __int_as_float((int)(p.jLo + nceps));
        st[kAf8StScal + 6] = __int_as_float(nullsSoFar + (int)nnull);
        st[kAf8StScal + 7] = __int_as_float(flushed);
    }
}

} // namespace sea
