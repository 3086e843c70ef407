/*
 * cc_slice_kernel.hip -- the plain CompCeps (DoCompCeps without WaveProc) over one TIME SLICE of every utterance, both rates,
 * gfx950 (MI355X) (include/sea_mi355x.h, sea_compceps_batch_slice / sea_wb_compceps_batch_slice; the state's layout:
 * sea_kernels.h, kCcStateFloats / kWbCcStateFloats).
 *
 * compceps_kernel and compceps_wb_kernel (cc_kernel.hip) stay as they are -- whatever joins that unit moves the register
 * allocation of measured kernels -- so the tile is shared through cc_tile.h, and the staging loop has a form of its own here with
 * the one difference a slice makes: words that lie before the slice's first sample come from the state.  The hot-path shape is
 * the one launch's: a wave owns 16 CONSECUTIVE cepstral frames sharing one span in LDS, and all of a tile's words are requested
 * in batches before the first store.  tests/test_gpu_ceps_slices.py holds the two together: the slices of an utterance must give
 * the bits of the one launch.
 *
 * What completes in a slice, the staging of the wideband rows and the carry of the history are cc_slice.h's, shared with the
 * feature chain's slice form (afe_slice_kernel.hip).
 *
 * What is carried, and who stores it.  The tile kernels run many workgroups per utterance, so they only READ the state;
 * compceps_carry_slice_kernel, one wave per utterance and a launch of its own after them on the same stream, writes the slice's
 * counts and then the state for the next slice.  It runs for every slice, also one without a whole frame.
 */
#undef SEA_CC_TIMING /* the tile's timing diagnostic is compceps_kernel's (cc_kernel.hip) */
#include "cc_tile.h"
#include "cc_slice.h"

namespace sea {

namespace {
template <bool WB>
__device__ __forceinline__ SliceSpan cc_slice_span(const CcSliceArgs &s, int u)
{
    return slice_span(s.c.first_out[u], s.c.lengths[u] / (WB ? SEA_WB_HOP : SEA_HOP), s.frame_base);
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
        const SliceSpan p = cc_slice_span<WB>(s, u);
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
                if (x < nword && !(x == 0 && first)) v = slice_sample(cur0, st + kCcStF32, loc, resume);
                sv[k] = v;
            }
#pragma unroll
            for (int k = 0; k < kCcStageBatch; ++k) {
                const int x = lane + kLanes * (b0 + k);
                if (x < nword) L.span[x + x / SEA_HOP] = sv[k];
            }
        }
        if (WB)
            stage_wb_rows(hpS, codeS, s.hp_rows, s.code_rows, (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP, r0, nv, st + kCcStHp,
                          st + kCcStCode, resume, lane);
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

/* One wave per utterance, after the tile pass: the slice's count, then the state for the next slice (cc_slice.h's carry).  A
 * slice without a whole frame (a ragged tail alone) reports 0 and stores back what it read. */
__global__ __launch_bounds__(64) void compceps_carry_slice_kernel(CcSliceArgs s)
{
    __shared__ float keep[kAfStKeep + kCarryRows];
    const CepsArgs &a = s.c;
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const bool wb = s.hp_rows != nullptr;
    const bool resume = s.resume != 0;
    float *st = s.state + (size_t)u * s.stride;
    const SliceSpan p = wb ? cc_slice_span<true>(s, u) : cc_slice_span<false>(s, u);
    if (lane == 0) a.n_ceps[u] = (int)p.nc; /* here, not in the tile pass: a slice without a frame launches no tile */
    carry_load(keep, a.den_f32 + (wb ? a.offsets[u] / 2 : a.offsets[u]), st + kCcStF32, p.nfr, resume, lane);
    if (wb)
        carry_load_rows(keep, s.hp_rows, s.code_rows, (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP, p.nfr, st + kCcStHp,
                        st + kCcStCode, resume, lane);
    __syncthreads();
    carry_store(st + kCcStF32, keep, lane);
    if (wb) carry_store_rows(st + kCcStHp, st + kCcStCode, keep, lane);
}

} // namespace sea
