/*
 * cc_slice_kernel.hip -- the plain CompCeps (DoCompCeps without WaveProc) over one TIME SLICE of every utterance, both rates,
 * gfx950 (MI355X) (include/sea_mi355x.h, sea_compceps_batch_slice / sea_wb_compceps_batch_slice; the state's layout:
 * sea_kernels.h, kCcStateFloats / kWbCcStateFloats).
 *
 * compceps_kernel and compceps_wb_kernel (cc_kernel.hip) stay as they are -- whatever joins that unit moves the register
 * allocation of measured kernels -- so the tile is shared through cc_tile.h and the staging is restated here with the one
 * difference a slice makes: words that lie before the slice's first sample come from the state.  The hot-path shape is the one
 * launch's: a wave owns 16 CONSECUTIVE cepstral frames sharing one span in LDS, and all of a tile's words are requested in
 * batches before the first store.  tests/test_gpu_ceps_slices.py holds the two texts together: the slices of an utterance must
 * give the bits of the one launch.
 *
 * What completes in a slice (afe_slice_kernel.hip's convention).  Cepstral frame j of an utterance whose first output is frame f0
 * reads the float stream from sample 80 (f0 + j) - 1 for 201 values and, in the wideband mode, the high-band and code rows of
 * frame f0 + j: it completes when output frame f0 + j + 2 exists.  A slice of the frames [fb, fb + n) completes j in
 * [max(0, fb - f0 - 2), fb + n - f0 - 2); up to two frames and one sample of the stream, and two rows of either kind, lie before
 * the slice and come from the state.
 *
 * What is carried, and who stores it.  The tile kernels run many workgroups per utterance, so they only READ the state;
 * compceps_carry_slice_kernel, one wave per utterance and a launch of its own after them on the same stream, writes the slice's
 * counts and then the state for the next slice.  It runs for every slice, also one without a whole frame.
 */
#undef SEA_CC_TIMING /* the tile's timing diagnostic is compceps_kernel's (cc_kernel.hip) */
#include "cc_tile.h"

namespace sea {

namespace {
/* the cepstral frames of utterance u that complete in the slice: [jLo, jLo + nc) */
struct CcSliceSpan {
    long long nfr, jLo, nc;
    int f0;
};
template <bool WB>
__device__ __forceinline__ CcSliceSpan cc_slice_span(const CcSliceArgs &s, int u)
{
    CcSliceSpan p;
    p.f0 = s.c.first_out[u];
    p.nfr = s.c.lengths[u] / (WB ? SEA_WB_HOP : SEA_HOP);
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

/* compceps_body (cc_kernel.hip) over the cepstral frames that complete in the slice: row r of the slice's block of utterance u
 * is cepstral frame jLo + r.  Data[-1] of the UTTERANCE's first cepstral frame is zero, whichever slice it falls into.  Rows
 * behind the slice's count are left alone: the capacity of a slice is its frames, not what the utterance may still produce. */
template <bool WB>
__device__ __forceinline__ void compceps_slice_body(const CcSliceArgs &s, CcTileLds<true> &L, CcWbLds *X = nullptr,
                                                    float *hpS = nullptr, float *codeS = nullptr)
{
    const CepsArgs &a = s.c;
    const int lane = threadIdx.x;
    const bool resume = s.resume != 0;
    CcTileConst C;
    load_cc_tile_const<true>(C, L, a.tables, lane);
    if (WB) {
        for (int i = lane; i < SEA_WB_NCHAN * 16; i += kLanes) X->dct26T[i] = s.wb->dct26T[i >> 4][i & 15];
        wave_sync();
    }
    const long long nslot = a.ceps_cum[a.n_utt] / kCcT + a.n_utt; /* tile slots as in compceps_kernel */
    for (long long sl = blockIdx.x; sl < nslot; sl += gridDim.x) {
        int lo = 0, hi = a.n_utt; /* largest u with base(u) <= sl */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ceps_cum[mid] / kCcT + mid <= sl) lo = mid; else hi = mid;
        }
        const int u = lo;
        const long long c0 = a.ceps_cum[u], cap = a.ceps_cum[u + 1] - c0;
        const long long j0 = (sl - (c0 / kCcT + u)) * kCcT; /* the tile's first row of the slice's block */
        if (j0 >= cap) continue; /* spare slot */
        const CcSliceSpan p = cc_slice_span<WB>(s, u);
        const int nrow = (int)((cap - j0 < kCcT) ? cap - j0 : kCcT);
        const long long left = p.nc - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        if (nv <= 0) continue;
        const float *st = s.state + (size_t)u * s.stride;
        const long long jA = p.jLo + j0;                /* the tile's first cepstral frame, absolute */
        const int r0 = (int)(p.f0 + jA - s.frame_base); /* its frame within the slice: >= -2 */
        float *dst = a.ceps + (c0 + j0) * SEA_CC_NCEP;
        /* span word x = Data[x-1] of the tile's first frame = the slice's sample s0 + x, -161 <= s0 + x < 80 nfr (the tile's last
         * frame ends with sample 39 of the slice's frame r0 + nv + 1 < nfr); what lies before the slice's first sample is the
         * state's last three frames */
        const float *cur0 = a.den_f32 + (WB ? a.offsets[u] / 2 : a.offsets[u]);
        const int s0 = r0 * SEA_HOP - 1;
        const bool first = jA == 0;
        const int nword = SEA_HOP * (nv - 1) + SEA_WIN + 1;
        /* all of the tile's words are requested before the first is stored, in two equal batches as in compceps_kernel */
        constexpr int kReq = (SEA_HOP * (kCcT - 1) + SEA_WIN + 1 + kLanes - 1) / kLanes; /* 22 */
        constexpr int kCcStageBatch = 11;
#pragma unroll 1
        for (int b0 = 0; b0 < kReq; b0 += kCcStageBatch) {
            float sv[kCcStageBatch];
#pragma unroll
            for (int k = 0; k < kCcStageBatch; ++k) {
                const int x = lane + kLanes * (b0 + k);
                const int loc = s0 + x;
                float v = 0.0f;
                if (x < nword && !(x == 0 && first)) {
                    if (loc >= 0) v = cur0[loc];
                    else if (resume) v = st[kCcStF32 + kAfStKeep + loc];
                }
                sv[k] = v;
            }
#pragma unroll
            for (int k = 0; k < kCcStageBatch; ++k) {
                const int x = lane + kLanes * (b0 + k);
                if (x < nword) L.span[x + x / SEA_HOP] = sv[k];
            }
        }
        if (WB) { /* the tile's rows of high-band energies and code values: frame r0 + f of the slice, the state's two before it */
            const long long row0 = (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP;
            for (int i = lane; i < nv * 9; i += kLanes) {
                const int r = r0 + i / 9, c = i % 9;
                codeS[i] = r >= 0 ? s.code_rows[(row0 + r) * 9 + c] : (resume ? st[kCcStCode + (2 + r) * 9 + c] : 0.0f);
            }
            if (lane < nv * 3) {
                const int r = r0 + lane / 3, c = lane % 3;
                hpS[lane] = r >= 0 ? s.hp_rows[(row0 + r) * 3 + c] : (resume ? st[kCcStHp + (2 + r) * 3 + c] : 0.0f);
            }
        }
        wave_sync();
        if (WB)
            cc_tile<true, kCcT, true>(L, C, nv, dst, lane, X, hpS, codeS, s.wb);
        else
            cc_tile<true>(L, C, nv, dst, lane);
    }
}
} // namespace

/* three waves per SIMD as compceps_kernel (LDS allows twelve waves per CU) */
__global__ __launch_bounds__(64, 3) void compceps_slice_kernel(CcSliceArgs s)
{
    __shared__ CcTileLds<true> L;
    compceps_slice_body<false>(s, L);
}

/* the wideband mode's, on the outputs of sea_wb_denoise_batch_slice; two waves per SIMD as compceps_wb_kernel */
__global__ __launch_bounds__(64, 2) void compceps_wb_slice_kernel(CcSliceArgs s)
{
    __shared__ CcTileLds<true> L;
    __shared__ CcWbLds X;
    __shared__ float hpS[kCcT * 3], codeS[kCcT * 9];
    compceps_slice_body<true>(s, L, &X, hpS, codeS);
}

/* One wave per utterance, after the tile pass: the slice's count, then the state for the next slice.  Element i of a history of
 * n is element i + m of (old history, the slice's m new ones): everything is read into LDS first and stored after a barrier.  A
 * slice without a whole frame (a ragged tail alone) reports 0 and stores back what it read. */
__global__ __launch_bounds__(64) void compceps_carry_slice_kernel(CcSliceArgs s)
{
    __shared__ float keep[kAfStKeep + 8 + 24];
    const CepsArgs &a = s.c;
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const bool wb = s.hp_rows != nullptr;
    const bool resume = s.resume != 0;
    float *st = s.state + (size_t)u * s.stride;
    const CcSliceSpan p = wb ? cc_slice_span<true>(s, u) : cc_slice_span<false>(s, u);
    if (lane == 0) a.n_ceps[u] = (int)p.nc; /* here, not in the tile pass: a slice without a frame launches no tile */
    {
        const float *cur = a.den_f32 + (wb ? a.offsets[u] / 2 : a.offsets[u]);
        const long long m8 = p.nfr * SEA_HOP;
        for (int i = lane; i < kAfStKeep; i += kLanes) {
            const long long j = i + m8;
            keep[i] = j >= kAfStKeep ? cur[j - kAfStKeep] : (resume ? st[kCcStF32 + j] : 0.0f);
        }
        if (wb && lane < 24) {
            const long long row0 = (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP;
            const float *rows = lane < 6 ? s.hp_rows : s.code_rows;
            const int wd = lane < 6 ? 3 : 9, i = lane < 6 ? lane : lane - 6, base = lane < 6 ? kCcStHp : kCcStCode;
            const long long r = i / wd + p.nfr; /* row of (the state's two, the slice's nfr) */
            keep[kAfStKeep + (lane < 6 ? 0 : 8) + i] =
                r >= 2 ? rows[(row0 + r - 2) * wd + i % wd] : (resume ? st[base + r * wd + i % wd] : 0.0f);
        }
    }
    __syncthreads();
    for (int i = lane; i < kAfStKeep; i += kLanes) st[kCcStF32 + i] = keep[i];
    if (wb) {
        if (lane < 8) st[kCcStHp + lane] = lane < 6 ? keep[kAfStKeep + lane] : 0.0f;
        if (lane < 24) st[kCcStCode + lane] = lane < 18 ? keep[kAfStKeep + 8 + lane] : 0.0f;
    }
}

} // namespace sea
