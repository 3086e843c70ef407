/*
 * cc_kernel.hip -- batched rfft and the CompCeps cepstral front-end, gfx950 (MI355X).
 *
 * Both are recursion-free per frame: a wave takes two frames (rfft) or a tile of 16 frames (CompCeps) at a time.
 *   rfft256_kernel           etsi/cpp/rfft.c:45-180 on [nframes][256] floats, in place or not
 *   compceps_frames_kernel   DoCompCeps (etsi/cpp/CompCeps.c:309-318 -> WI8CompCeps :368-549) on
 *                            caller-supplied frames of 201 floats (Data[-1..199])
 *   compceps_kernel          the same, reading frames straight out of the float NoiseSup stream:
 *                            frame j of an utterance = denoised[80j-1 .. 80j+199], available once 3
 *                            NoiseSup outputs exist (the commented-out driver block
 *                            etsi/cpp/ParmInterface.c:275-293)
 * The tile (cc_tile.h) and DoWaveProc (cc_waveproc.h) are shared with afe_wb_kernel.hip.
 */
#include "cc_tile.h"
#include "cc_waveproc.h"
#include "afe_vad.h"

namespace sea {

/* Streaming form: a wave transforms TWO frames at a time (lanes 0..31 / 32..63, the dual transform of
 * sea_device.h: swizzled work area, five LDS round trips), 2 KB in + 2 KB out per pass.  Budget per frame at the
 * HBM rate: ~240 clk per CU, i.e. ~960 SIMD-clk and ~240 LDS-array clk; the dual transform needs ~180 vector
 * issue slots and ~144 LDS clk per frame (the one-frame-per-wave form: ~300 and ~320 -- LDS-bound).  Each lane
 * gathers its eight inputs n0 + 32 bitrev3(j) straight from global memory (per instruction the 32 lanes of a frame
 * read one contiguous 128-byte line), one pair ahead; results leave as one float4 per lane and frame.
 * The butterflies' operand addresses stay in VGPRs (4.45 TB/s; in LDS -- 76 VGPRs, five waves per SIMD -- 4.04); loads and stores are
 * non-temporal: every frame is touched once. */
constexpr int kRfftWaves = 4; /* waves per SIMD the register allocation leaves room for */
__global__ __launch_bounds__(64, kRfftWaves) void rfft256_kernel(const float *in, float *out, long long nframes,
                                                                     const sea_fft_tables *t)
{
    __shared__ __attribute__((aligned(16))) float work[512];
    const int lane = threadIdx.x;
    Fft2Regs R;
    load_fft2_regs<false>(R, t, lane, nullptr);
    wave_sync();
    const int n0 = lane & 31, h = lane >> 5;
    unsigned oa[4]; /* where elements 4l..4l+3 of the reference's order sit in a (swizzled) work area */
#pragma unroll
    for (int q = 0; q < 4; ++q) oa[q] = fft_swz(4u * (unsigned)lane + (unsigned)q);
    const long long npair = (nframes + 1) >> 1;
    auto load = [&](long long p, float(&e)[8]) {
        const long long f = 2 * p + h;
        const float *x = in + (f < nframes ? f : 0) * 256 + n0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            constexpr int kRev3[8] = {0, 4, 2, 6, 1, 5, 3, 7};
            const float v = __builtin_nontemporal_load(x + 32 * kRev3[k]);
            e[k] = (f < nframes) ? v : 0.0f;
        }
    };
    float cur[8], nxt[8];
    long long p = blockIdx.x;
    if (p < npair) load(p, cur);
    for (; p < npair; p += gridDim.x) {
        const long long pn = p + gridDim.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) nxt[k] = 0.0f;
        if (pn < npair) load(pn, nxt);
        rfft256_dual(cur, work, R);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const long long f = 2 * p + hh;
            if (f < nframes) {
                const float *w = work + 256 * hh;
                float4 v;
                v.x = fft_at(w, oa[0]);
                v.y = fft_at(w, oa[1]);
                v.z = fft_at(w, oa[2]);
                v.w = fft_at(w, oa[3]);
                typedef float v4f __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f *>(out + f * 256 + 4 * lane));
            }
        }
        wave_sync();
#pragma unroll
        for (int k = 0; k < 8; ++k) cur[k] = nxt[k];
    }
}

/* rfft (x, n, m) for every size the reference's routine takes (etsi/cpp/rfft.c:45-180): ONE workgroup per transform walks
 * the schedule sea_rfft_schedule() unrolled on the host -- digit reversal, the length-two butterflies, then level by
 * level the plain, pi/4 and twiddled butterflies of all blocks, which touch disjoint elements within a level -- with the
 * frame in LDS (n floats, dynamic).  A convenience path behind the drop-in symbol (the hot path's only size, (256, 8),
 * keeps rfft256_kernel; the 16 k-native variant's (512, 8) keeps its own schedule in ns16k_pipe_kernel.hip): written
 * for exactness -- the reference's operations in the reference's order per butterfly -- not for speed. */
__global__ __launch_bounds__(256) void rfft_any_kernel(float *x, const unsigned *sched, long long nframes)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int n = (int)sched[0], m = (int)sched[1];
    const unsigned *rev = sched + sched[2], *len2 = sched + sched[3];
    const int nlen2 = (int)sched[4], tid = threadIdx.x;
    for (long long f = blockIdx.x; f < nframes; f += gridDim.x) {
        float *xf = x + f * n;
        for (int i = tid; i < n; i += 256) xs[rev[i]] = xf[i];
        __syncthreads();
        for (int w = tid; w < nlen2; w += 256) { /* :82-96 */
            const int i0 = (int)len2[w];
            const float a0 = xs[i0], a1 = xs[i0 + 1];
            xs[i0] = a0 + a1;
            xs[i0 + 1] = a0 - a1;
        }
        __syncthreads();
        int n2 = 2;
        for (int k = 1; k < m; ++k) {
            n2 <<= 1;
            const int n4 = n2 >> 2, n8 = n2 >> 3, per = n8 > 0 ? n8 : 1;
            const unsigned *blk = sched + sched[5 + 3 * k];
            const float *tw = reinterpret_cast<const float *>(sched + sched[7 + 3 * k]);
            const int items = (int)sched[6 + 3 * k] * per;
            for (int w = tid; w < items; w += 256) {
                const int i = (int)blk[w / per], j = w % per;
                if (j == 0) {
                    { /* :108-115 */
                        const int i1 = i, i3 = i1 + 2 * n4, i4 = i3 + n4;
                        const float x1 = xs[i1], x3 = xs[i3], x4 = xs[i4];
                        const float t1 = x4 + x3;
                        xs[i4] = x4 - x3;
                        xs[i3] = x1 - t1;
                        xs[i1] = x1 + t1;
                    }
                    if (n4 != 1) { /* :117-128; the division by sqrt 2 in double == this multiplication for every float
                                      (sea_device.h, swept over all 2^32 by sea_selftest_pi4) */
                        const int i1 = i + n8, i2 = i1 + n4, i3 = i2 + n4, i4 = i3 + n4;
                        const float x1 = xs[i1], x2 = xs[i2], x3 = xs[i3], x4 = xs[i4];
                        const float t1 = (float)((double)(x3 + x4) * 0.70710678118654752440);
                        const float t2 = (float)((double)(x3 - x4) * 0.70710678118654752440);
                        xs[i4] = x2 - t1;
                        xs[i3] = -x2 - t1;
                        xs[i2] = x1 - t2;
                        xs[i1] = x1 + t2;
                    }
                } else { /* :145-174 */
                    const float cc1 = tw[4 * j], ss1 = tw[4 * j + 1], cc3 = tw[4 * j + 2], ss3 = tw[4 * j + 3];
                    const int i1 = i + j, i2 = i1 + n4, i3 = i2 + n4, i4 = i3 + n4;
                    const int i5 = i + n4 - j, i6 = i5 + n4, i7 = i6 + n4, i8 = i7 + n4;
                    const float x1 = xs[i1], x2 = xs[i2], x3 = xs[i3], x4 = xs[i4], x5 = xs[i5], x6 = xs[i6], x7 = xs[i7], x8 = xs[i8];
                    float t1 = x3 * cc1 + x7 * ss1;
                    float t2 = x7 * cc1 - x3 * ss1;
                    float t3 = x4 * cc3 + x8 * ss3;
                    float t4 = x8 * cc3 - x4 * ss3;
                    const float t5 = t1 + t3, t6 = t2 + t4;
                    t3 = t1 - t3;
                    t4 = t2 - t4;
                    xs[i3] = t6 - x6;
                    xs[i8] = x6 + t6;
                    xs[i7] = -x2 - t3;
                    xs[i4] = x2 - t3;
                    xs[i6] = x1 - t5;
                    xs[i1] = x1 + t5;
                    xs[i5] = x5 - t4;
                    xs[i2] = x5 + t4;
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < n; i += 256) xf[i] = xs[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void compceps_frames_kernel(const float *data201, float *coef14,
                                                             long long nframes, const sea_cc_tables *t)
{
    __shared__ CcTileLds<false> L;
    const int lane = threadIdx.x;
    CcTileConst C;
    load_cc_tile_const<false>(C, L, t, lane);
    const long long ntile = (nframes + kCcT - 1) / kCcT;
    for (long long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const long long f0 = tile * kCcT;
        const int nv = (int)((nframes - f0 < kCcT) ? nframes - f0 : kCcT);
        const float *src = data201 + f0 * 201;
        constexpr int kBatch = 13, kIter = (kCcT * 201 + kLanes - 1) / kLanes;
        for (int b0 = 0; b0 < kIter; b0 += kBatch) { /* requests in batches before their stores (see compceps_kernel) */
            float sv[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int i = lane + kLanes * (b0 + k);
                sv[k] = (i < nv * 201) ? src[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int i = lane + kLanes * (b0 + k);
                if (i < nv * 201) L.span[i] = sv[k];
            }
        }
        wave_sync();
        cc_tile<false, kCcT, false, true>(L, C, nv, coef14 + f0 * SEA_CC_NCEP, lane); /* the caller's floats: NF */
    }
}

namespace {
/* WB: the wideband mode -- the float stream and first_out are at the 8 kHz rate (offsets[u] / 2, frames of 160 input samples) */
template <bool WB>
__device__ __forceinline__ void compceps_body(const CepsArgs &a, CcTileLds<true> &L, CcWbLds *X = nullptr, const float *hpRows = nullptr,
                                              const float *codeRows = nullptr, const sea_wb_tables *wbt = nullptr)
{
    const int lane = threadIdx.x;
#ifdef SEA_CC_TIMING
    if (lane == 0 && blockIdx.x < 16384) {
        g_cc_wave[4 * blockIdx.x] = (unsigned)wall_clock64();
        g_cc_wave[4 * blockIdx.x + 2] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
        g_cc_wave[4 * blockIdx.x + 3] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);
    }
#endif
    CcTileConst C;
    load_cc_tile_const<true>(C, L, a.tables, lane);
    if (WB) {
        for (int i = lane; i < SEA_WB_NCHAN * 16; i += kLanes) X->dct26T[i] = wbt->dct26T[i >> 4][i & 15];
        wave_sync();
    }
    /* tile slots: utterance u owns slots [ceps_cum[u] / T + u, ceps_cum[u+1] / T + u + 1), at least
     * ceil(capacity / T) of them; slot k of an utterance covers its cepstral frames kT .. kT + T - 1 */
    const long long nslot = a.ceps_cum[a.n_utt] / kCcT + a.n_utt;
    for (long long s = blockIdx.x; s < nslot; s += gridDim.x) {
        int lo = 0, hi = a.n_utt; /* largest u with base(u) <= s */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ceps_cum[mid] / kCcT + mid <= s) lo = mid; else hi = mid;
        }
        const int u = lo;
        const long long c0 = a.ceps_cum[u], cap = a.ceps_cum[u + 1] - c0;
        const long long j0 = (s - (c0 / kCcT + u)) * kCcT;
        if (j0 >= cap) continue; /* spare slot */
        const int f0 = a.first_out[u];
        const long long nfr = a.lengths[u] / (WB ? SEA_WB_HOP : SEA_HOP);
        const long long nout = (f0 >= 0) ? nfr - f0 : 0;
        const long long nceps = (nout >= 3) ? nout - 2 : 0;
        if (j0 == 0 && lane == 0 && a.n_ceps) a.n_ceps[u] = (int)nceps;
        const int nrow = (int)((cap - j0 < kCcT) ? cap - j0 : kCcT);
        long long left = nceps - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        float *dst = a.ceps + (c0 + j0) * SEA_CC_NCEP;
        if (nv > 0) {
#ifdef SEA_CC_TIMING
            constexpr bool SHARED = true; /* (CC_CK's switch) */
#endif
            CC_CK_START;
            /* span word x = Data[x-1] of frame j0: the float NoiseSup stream from sample 80 (f0 + j0) - 1 on;
             * Data[-1] of the utterance's very first cepstral frame is the zero before the first output */
            const float *cur0 = a.den_f32 + (WB ? a.offsets[u] / 2 : a.offsets[u]) + (f0 + j0) * SEA_HOP;
            const int nword = SEA_HOP * (nv - 1) + SEA_WIN + 1;
            /* all of the tile's words are requested before the first is stored: written as a load-store loop the
             * compiler waits for each of the 22 requests in turn -- ~22 HBM latencies per tile, most of the kernel's time */
            constexpr int kReq = (SEA_HOP * (kCcT - 1) + SEA_WIN + 1 + kLanes - 1) / kLanes; /* 22 */
            /* round 3: 22 at once two waves per SIMD 0.77 ms, 8: three waves 0.71; round 4 (three waves per SIMD forced, 168 VGPRs
             * either way): 8 0.610 ms, 11 = two equal batches 0.58-0.60, 12 0.60, 22 (32 spilled registers) not run */
            constexpr int kCcStageBatch = 11;
#pragma unroll 1
            for (int b0 = 0; b0 < kReq; b0 += kCcStageBatch) {
                float sv[kCcStageBatch];
#pragma unroll
                for (int k = 0; k < kCcStageBatch; ++k) {
                    const int x = lane + kLanes * (b0 + k);
                    sv[k] = (x < nword && !(x == 0 && j0 == 0)) ? cur0[x - 1] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < kCcStageBatch; ++k) {
                    const int x = lane + kLanes * (b0 + k);
                    if (x < nword) L.span[x + x / SEA_HOP] = sv[k];
                }
            }
            wave_sync();
            CC_CK(0);
#ifdef SEA_CC_TIMING
            if (blockIdx.x == 0 && lane == 0) g_cc_ck[7] += 1;
#endif
            if (WB) {
                const long long row = (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP + f0 + j0; /* sea_kernels.h, WbHbArgs */
                cc_tile<true, kCcT, true>(L, C, nv, dst, lane, X, hpRows + row * 3, codeRows + row * 9, wbt);
            } else
                cc_tile<true>(L, C, nv, dst, lane);
        }
        for (int idx = nv * SEA_CC_NCEP + lane; idx < nrow * SEA_CC_NCEP; idx += kLanes) dst[idx] = 0.0f;
    }
#ifdef SEA_CC_TIMING
    if (lane == 0 && blockIdx.x < 16384) g_cc_wave[4 * blockIdx.x + 1] = (unsigned)wall_clock64();
#endif
}
} // namespace

/* three waves per SIMD (LDS allows twelve waves per CU): 168 VGPRs, no spilled vector register; left to itself the allocator takes
 * 193 = two waves per SIMD */
__global__ __launch_bounds__(64, 3) void compceps_kernel(CepsArgs a)
{
    __shared__ CcTileLds<true> L;
    compceps_body<false>(a, L);
}

/* the wideband mode's CompCeps on the outputs of sea_wb_denoise_batch */
__global__ __launch_bounds__(64, 2) void compceps_wb_kernel(WbCepsArgs a)
{
    __shared__ CcTileLds<true> L;
    __shared__ CcWbLds X;
    compceps_body<true>(a.c, L, &X, a.hp_rows, a.code_rows, a.wb);
}

/* ==================================================================================================
 * the chain after NoiseSup that the reference has commented out
 * (etsi/cpp/ParmInterface.c:274-311): WaveProc -> CompCeps -> PostProc -> VAD, FlushAdvProcess.
 * WaveProc and CompCeps depend on the frame only -> one wave per cepstral frame (afe_ceps_kernel);
 * PostProc (an LMS recurrence over frames) and the frame-dropping VAD (a 7-frame ring and two
 * hangover counters) are serial per utterance and tiny -> one wave per utterance (afe_vad_kernel).
 * ================================================================================================ */

/* WaveProc + CompCeps of the restored feature chain, tiled like compceps_kernel: a wave owns 16 consecutive
 * cepstral frames of one utterance as SEPARATE 201-float frames in LDS (WaveProc reshapes each frame in place, so
 * they cannot share samples).  The low-energy check's in-order sum of squares runs lane = frame; the frames that
 * pass go through DoWaveProc one after the other (wave-wide peak search), then the tile through cc_tile(). */

/* timing-only diagnostic (-DSEA_AFE_TIMING, tools/afe_phases.py): shader clocks workgroup 0 spends per step of a tile */
#ifdef SEA_AFE_TIMING
__device__ unsigned long long g_afe_ck[8];
extern "C" int sea_afe_timing(unsigned long long *out8, int reset)
{
    if (reset) {
        unsigned long long z[8] = {};
        return hipMemcpyToSymbol(HIP_SYMBOL(g_afe_ck), z, sizeof z) != hipSuccess;
    }
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_afe_ck), 8 * sizeof(unsigned long long)) != hipSuccess;
}
#define AFE_CK_START unsigned long long ck_ = clock64()
#define AFE_CK(k) do { const unsigned long long c_ = clock64(); if (blockIdx.x == 0 && threadIdx.x == 0) g_afe_ck[k] += c_ - ck_; ck_ = c_; } while (0)
#else
#define AFE_CK_START
#define AFE_CK(k)
#endif

__global__ __launch_bounds__(64, 1) void afe_ceps_kernel(AfeArgs a)
{
    __shared__ CcTileLds<false, kAfeT> L;
    __shared__ WpLds W;
    const int lane = threadIdx.x;
    CcTileConst C;
    load_cc_tile_const<false, kAfeT>(C, L, a.tables, lane);
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
        const long long nfr = a.lengths[u] / SEA_HOP;
        const long long nout = (f0 >= 0) ? nfr - f0 : 0;
        const long long nceps = (nout >= 3) ? nout - 2 : 0;
        if (j0 == 0 && lane == 0 && a.n_ceps) a.n_ceps[u] = (int)nceps;
        const int nrow = (int)((cap - j0 < kAfeT) ? cap - j0 : kAfeT);
        long long left = nceps - j0;
        const int nv = (int)(left < 0 ? 0 : (left > nrow ? nrow : left));
        float *dst = a.feat_cc + (c0 + j0) * SEA_CC_NCEP;
        AFE_CK_START;
        if (nv > 0) {
            /* frameBuf of ParmInterface.c:281 for cepstral frame j: Data[-1..199] = the float NoiseSup stream from
             * sample 80 (f0 + j) - 1 on; Data[-1] of the utterance's first cepstral frame is 0 */
            const float *cur0 = a.den_f32 + a.offsets[u] + (f0 + j0) * SEA_HOP;
            constexpr int kAfeBatch = 17; /* 1: 4.03 ms for the feature pass, 6: 3.78, 13-17: 3.66 (outer loop kept rolled) */
            /* requests in batches before their stores, the outer loop kept rolled (fully unrolled the allocator went to
             * 256 VGPRs + 95 AGPRs, one wave per SIMD: 3.96 -> 5.9 ms) */
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
            AFE_CK(0);
            float energy = 0.0f; /* WaveProc.c:423-427, lane = frame */
            if (lane < nv) {
                const float *p = L.span + 201 * lane;
#pragma unroll 8
                for (int x = 1; x < 201; ++x) {
                    const float v = p[x];
                    energy += v * v;
                }
            }
            const unsigned long long pass = __ballot(lane < nv && (double)energy >= 100.0);
            AFE_CK(1);
            for (int g = 0; g < nv; g += 4) { /* four frames at a time: their peak searches run side by side */
                const unsigned m4 = (unsigned)(pass >> g) & 0xfu;
                if (m4 == 0) continue;
                for (int r = 0; r < 4; ++r)
                    if ((m4 >> r) & 1u) wp_smooth(W, r, L.span + 201 * (g + r) + 1, lane);
                AFE_CK(2);
                wp_peaks4(W, m4, lane);
                AFE_CK(3);
                for (int r = 0; r < 4; ++r)
                    if ((m4 >> r) & 1u) wp_window(W, r, L.span + 201 * (g + r) + 1, lane);
                AFE_CK(4);
            }
            wave_sync();
            cc_tile<false, kAfeT>(L, C, nv, dst, lane);
            AFE_CK(5);
#ifdef SEA_AFE_TIMING
            if (blockIdx.x == 0 && threadIdx.x == 0) g_afe_ck[7] += 1;
#endif
        }
        for (int idx = nv * SEA_CC_NCEP + lane; idx < nrow * SEA_CC_NCEP; idx += kLanes) dst[idx] = 0.0f;
    }
}

/* DoPostProc (PostProc.c:123-149), DoVADProc (VAD.c:219-317), DoVADFlush (:342-433) and the null
 * feature frames of the all-zero lead (ParmInterface.c:314-329), in emission order.  lane = feature
 * index (0..13 cepstra/energies, 14 the VAD flag). */
namespace {
/* WB: frames of 160 input samples, the speech flags one byte per per-frame row (ns_denoise_pipe_wb_fd_kernel); the null vectors
 * follow the wideband gate, which works on the 160 raw samples (ParmInterface.c:244-251): a.onset is that gate's.  The
 * arithmetic is the same: PostProc.c and VAD.c read no wideband state.  The registers, PostProc's table and the decision are
 * afe_vad.h's, shared with the slice form (afe_slice_kernel.hip); the row loop and the flush loop are written out here and there:
 * why, afe_vad.h says. */
template <bool WB>
__device__ __forceinline__ void afe_vad_body(const AfeArgs &a, float (&ring)[7][16])
{
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const int f0 = a.first_out[u];
    const long long nfr = a.lengths[u] / (WB ? SEA_WB_HOP : SEA_HOP);
    const long long nout = (f0 >= 0) ? nfr - f0 : 0;
    const long long nceps = (nout >= 3) ? nout - 2 : 0;
    long long nnull = a.onset[u];
    nnull = nnull < nfr ? nnull : nfr;
    float *out = a.feat15 + a.feat_cum[u] * 15;
    const float *cc = a.feat_cc + a.ceps_cum[u] * SEA_CC_NCEP;
    float *pp = a.feat_pp ? a.feat_pp + a.ceps_cum[u] * SEA_CC_NCEP : nullptr;
    const unsigned char *flg = a.flags + (WB ? (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP : a.offsets[u] / 8);
    constexpr int kFlagStep = WB ? 1 : 10; /* bytes between the flags of two frames */
    long long nemit = 0;

    for (long long k = 0; k < nnull; ++k) { /* null MFCC vectors, VAD = NON_SPEECH */
        if (lane < 15) out[nemit * 15 + lane] = 0.0f;
        nemit++;
    }
    if (lane < 16)
#pragma unroll
        for (int r = 0; r < 7; ++r) ring[r][lane] = 0.0f;
    wave_sync();

    const float tgt = afe_postproc_target(lane);
    const float lambda = kPostProcLambda;
    AfeVad v;

    auto decide = [&](int fc) { afe_vad_decide(v, ring, fc, lane); };

    /* rows and flag bytes are requested kAhead frames before use: the loop body is a few dozen
     * instructions, an HBM round trip a few thousand clocks */
    constexpr int kAhead = 8;
    float rowQ[kAhead];
    int bitQ[kAhead];
    auto fetch = [&](long long j, float &row, int &bits) {
        const long long jj = j < nceps ? j : (nceps > 0 ? nceps - 1 : 0);
        row = (lane < 14 && nceps > 0) ? cc[jj * SEA_CC_NCEP + lane] : 0.0f;
        bits = (nceps > 0) ? (int)flg[kFlagStep * (f0 + jj + 2)] : 0;
    };
#pragma unroll
    for (int q = 0; q < kAhead; ++q) fetch(q, rowQ[q], bitQ[q]);
    for (long long j0 = 0; j0 < nceps; j0 += kAhead) {
#pragma unroll
      for (int q = 0; q < kAhead; ++q) {
        const long long j = j0 + q;
        if (j >= nceps) break;
        /* PostProc on c1..c12; the weighting comes from logE = Coef[13] (Noc0 == 0) */
        const float c = rowQ[q];
        const int bits = bitQ[q];
        fetch(j + kAhead, rowQ[q], bitQ[q]);
        const float logE = __shfl(c, 13, 64);
        float wp = (logE * (float)64 - (float)211) / (float)64;
        wp = (wp < 0) ? 0.0f : ((wp > 1) ? lambda : wp * lambda);
        float x = c;
        if (lane < 12) {
            const float dif = ((c - v.wLMS) - tgt);
            x = c - v.wLMS;
            v.wLMS += dif * wp;
        }
        if (pp && lane < 14) pp[j * SEA_CC_NCEP + lane] = x;
        if (lane < 14) v.feat = x;
        /* DoVADProc */
        v.frameCounter = (int)j + 5; /* nbFrame[0] when NoiseSup output j+3 appears */
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
    /* FlushAdvProcess until DoVADFlush returns FALSE */
    {
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
    }
    if (lane == 0) a.n_feat[u] = (int)nemit;
}
} // namespace

__global__ __launch_bounds__(64) void afe_vad_kernel(AfeArgs a)
{
    __shared__ float ring[7][16];
    afe_vad_body<false>(a, ring);
}

/* the same pass over the wideband chain's cepstra (afe_wb_kernel.hip) */
__global__ __launch_bounds__(64) void afe_wb_vad_kernel(AfeArgs a)
{
    __shared__ float ring[7][16];
    afe_vad_body<true>(a, ring);
}

} // namespace sea
