/*
 * afe_wb_kernel.hip -- the wideband (16 kHz) feature chain's WaveProc + CompCeps pass, gfx950 (MI355X).
 *
 * A unit of its own: whatever joins cc_kernel.hip's unit moves the register allocation of the 8 kHz kernels there (afe_ceps_kernel
 * came out with 233 or 251 instead of 255 VGPRs), and those are to stay as measured.  The tile and WaveProc are shared with them
 * through cc_tile.h / cc_waveproc.h; the PostProc + VAD pass of the chain is afe_wb_vad_kernel in cc_kernel.hip (its registers and
 * decision: afe_vad.h).  The time-slice forms of both passes, for both rates, are one text in afe_slice_kernel.hip.
 */
#undef SEA_CC_TIMING /* the tile's timing diagnostic is compceps_kernel's (cc_kernel.hip) */
#include "cc_tile.h"
#include "cc_waveproc.h"

namespace sea {

/* The wideband chain's WaveProc + CompCeps on the outputs of sea_wb_denoise_batch_fd, tiled like afe_ceps_kernel: WaveProc is
 * mode-independent (WaveProc.c never reads Do16kHzProc) and reshapes the low band's 200-sample frame before CompCeps sums its
 * energy; the tile then takes the frames' rows of high-band energies and code values as compceps_wb_kernel's does.  The float
 * stream and first_out are at the 8 kHz rate (offsets[u] / 2, frames of 160 input samples).
 * LDS: 19312 bytes per wave (the 8 kHz tile's 17136 + dec / fbx / the 26-band DCT) -> eight waves in a CU's 160 KB; 253 VGPRs, no
 * scratch -> two waves per SIMD of 512 registers = the same eight.  Left at one wave per SIMD the allocator takes 256 + 2 AGPRs
 * = four per CU. */
__global__ __launch_bounds__(64, 2) void afe_wb_ceps_kernel(WbAfeArgs w)
{
    __shared__ CcTileLds<false, kAfeT> L;
    __shared__ WpLds W;
    __shared__ CcWbLds X;
    const AfeArgs &a = w.a;
    const int lane = threadIdx.x;
    CcTileConst C;
    load_cc_tile_const<false, kAfeT>(C, L, a.tables, lane);
    for (int i = lane; i < SEA_WB_NCHAN * 16; i += kLanes) X.dct26T[i] = w.wb->dct26T[i >> 4][i & 15];
    wave_sync();
    const long long nslot = a.ceps_cum[a.n_utt] / kAfeT + a.n_utt; /* tile slots as in compceps_kernel */
    for (long long s = blockIdx.x; s < nslot; s += gridDim.x) {
        int lo = 0, hi = a.n_utt;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ceps_cum[mid] / kAfeT + mid <= s) lo = mid; else hi = mid;
        }
        const int u = lo;
        const long long c0 = a.ceps_cum[u], cap = a.ceps_cum[u + 1] - c0;
        const long long j0 = (s - (c0 / kAfeT + u)) * kAfeT;
        if (j0 >= cap) continue;
        const int f0 = a.first_out[u];
        const long long nfr = a.lengths[u] / SEA_WB_HOP;
        const long long nout = (f0 >= 0) ? nfr - f0 : 0;
        const long long nceps = (nout >= 3) ? nout - 2 : 0;
        if (j0 == 0 && lane == 0 && a.n_ceps) a.n_ceps[u] = (int)nceps;
        const int nrow = (int)((cap - j0 < kAfeT) ? cap - j0 : kAfeT);
        long long left = nceps - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        float *dst = a.feat_cc + (c0 + j0) * SEA_CC_NCEP;
        if (nv > 0) {
            /* Data[-1..199] of cepstral frame j = the low band's float stream from sample 80 (f0 + j) - 1 on, staged as in
             * afe_ceps_kernel: requests in batches before their stores, the outer loop kept rolled */
            const float *cur0 = a.den_f32 + a.offsets[u] / 2 + (f0 + j0) * SEA_HOP;
            constexpr int kAfeBatch = 13; /* 17 as in afe_ceps_kernel spills two registers here; 13-17 measured alike there */
            constexpr int kIter = (kAfeT * 201 + kLanes - 1) / kLanes; /* 51 */
#pragma unroll 1
            for (int b0 = 0; b0 < kIter; b0 += kAfeBatch) {
                float sv[kAfeBatch];
#pragma unroll
                for (int k = 0; k < kAfeBatch; ++k) {
                    const int i = lane + kLanes * (b0 + k);
                    const int f = i / 201, x = i - f * 201;
                    sv[k] = (i < nv * 201 && !(x == 0 && f == 0 && j0 == 0)) ? cur0[SEA_HOP * f + x - 1] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < kAfeBatch; ++k) {
                    const int i = lane + kLanes * (b0 + k);
                    if (i < nv * 201) L.span[i] = sv[k];
                }
            }
            wave_sync();
            float energy = 0.0f; /* WaveProc.c:413-417, lane = frame */
            if (lane < nv) {
                const float *p = L.span + 201 * lane;
#pragma unroll 8
                for (int x = 1; x < 201; ++x) {
                    const float v = p[x];
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
            const long long row = (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP + f0 + j0; /* sea_kernels.h, WbHbArgs */
            cc_tile<false, kAfeT, true>(L, C, nv, dst, lane, &X, w.hp_rows + row * 3, w.code_rows + row * 9, w.wb);
        }
        for (int idx = nv * SEA_CC_NCEP + lane; idx < nrow * SEA_CC_NCEP; idx += kLanes) dst[idx] = 0.0f;
    }
}

} // namespace sea
