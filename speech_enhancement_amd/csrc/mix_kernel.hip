/*
 * mix_kernel.hip -- the training-set builder: addnoise() (enhancement_extract_subband_linux/cpp/extractwav.cpp:6-35) on the
 * device, the pipeline mix -> subbband() x2/x3 -> make_single_IBM's IRM on one stream, and the same from host buffers in
 * chunks (the loop of enhancement_extract_subband_linux/cpp/main.cpp:91-274).  DESIGN.md section 5.10.
 *
 * addnoise per utterance, as g++ on x86-64 compiles it:
 *   sums    float puresum = 0, noisesum = 0; for every sample IN ORDER  sum = (float)((double)sum + (double)(x * x)), x * x in
 *           int.  The double sum is exact (a float below 2^47 plus an integer up to 2^30 fits 53 bits), so every step is
 *           one correctly rounded float addition of an integer a float cannot hold: done here as f64 add + conversion.  A
 *           tree reduction gives other sums and, from 4 800 samples up, other samples.
 *   gain    sqrt ((puresum / noisesum) / (float)pow (10.0, db / 10.0)), both divisions in float.  The reference's sqrt may
 *           be the double one; rounded to float that is the correctly rounded float square root (53 >= 2 * 24 + 2), which
 *           is what sqrtf is in this build (hipcc's default; the Makefile passes no fast-math flag), as `/` is IEEE.
 *   scaled  (short)((float)noise[i] * gain).  C leaves the out-of-range conversion undefined; defined here as the x86-64
 *           build behaves (cvttss2si + low half): int32 truncating toward zero, low 16 bits kept; NaN or |product| >= 2^31
 *           give 0.  v_cvt_i32_f32 saturates instead, hence the explicit range test.
 *   noisy   low 16 bits of clean[i] + scaled[i].
 * Silent noise (gain inf, products NaN or inf -> 0, noisy = clean) and silent clean (gain 0) fall out of these rules.
 *
 * Two launches:
 *   mix_sums_kernel   one wave per kMixGroup utterances.  The two chains of an utterance are serial and independent, so
 *                     lane r < kMixGroup walks the clean samples of group member r and lane kMixGroup + r its noise
 *                     stretch.  Global memory is read by all 64 lanes, lane-consecutive, one tile of kMixTile samples per
 *                     row at a time into registers while the previous tile is walked out of LDS (row pitch odd in dwords:
 *                     the 16 walking lanes hit 16 banks).  Samples past an utterance's end are staged as 0, which leaves a
 *                     sum as it is, so no lane needs a length test in the walk.
 *   mix_scale_kernel  over all samples, 8 per thread: gain from the sums, the noise stretch (any alignment) staged through
 *                     LDS with lane-consecutive loads, clean / scaled / noisy as 16-byte vectors.  The pad samples up to the
 *                     next multiple of 8 are written as 0, the packed layout's convention.
 */
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "capi_internal.h"

using namespace sea_capi;

namespace {

constexpr int kMixGroup = 8;             /* utterances per wave */
constexpr int kMixRows = 2 * kMixGroup;  /* chains per wave: clean and noise of each */
constexpr int kMixTile = 256;            /* samples per row and tile */
constexpr int kMixPitch = kMixTile / 2 + 1; /* dwords; odd, so rows r and r + 1 start one bank apart */
constexpr int kMixQ = kMixTile / 64;     /* loads per lane, row and tile */
constexpr int kScaleThreads = 256, kScalePer = 8, kScaleChunk = kScaleThreads * kScalePer, kScaleBlocksX = 16;

struct MixArgs {
    const int16_t *clean;
    const long long *offsets, *lengths;
    const int16_t *noise_src;
    const long long *noise_start;
    const float *snr_lin;
    int16_t *noise_scaled, *noisy;
    float *sums; /* [n_utt][2]: pure, noise */
    float *gain; /* [n_utt] or NULL */
    const int *order;
    int n_utt;
};

/* one step of `sum += x * x * 1.0` with a float sum */
__device__ __forceinline__ float mix_acc(float acc, int x) { return (float)((double)acc + (double)(x * x)); }

__global__ __launch_bounds__(64) void mix_sums_kernel(MixArgs a)
{
    __shared__ uint32_t tile[kMixRows][kMixPitch];
    const int lane = threadIdx.x;
    const int first = blockIdx.x * kMixGroup;
    /* wave-uniform description of the rows */
    const int16_t *src[kMixRows];
    long long len[kMixRows], maxL = 0;
#pragma unroll
    for (int r = 0; r < kMixGroup; ++r) {
        const int k = first + r;
        long long L = 0, off = 0, ns = 0;
        if (k < a.n_utt) {
            const int u = a.order ? a.order[k] : k;
            L = std::max(a.lengths[u], 0LL);
            off = a.offsets[u];
            ns = a.noise_start[u];
        }
        src[r] = a.clean + off;
        src[kMixGroup + r] = a.noise_src + ns;
        len[r] = len[kMixGroup + r] = L;
        maxL = std::max(maxL, L);
    }
    const long long ntile = (maxL + kMixTile - 1) / kMixTile;
    int16_t st[kMixRows][kMixQ];
    auto fetch = [&](long long j) {
#pragma unroll
        for (int r = 0; r < kMixRows; ++r)
#pragma unroll
            for (int q = 0; q < kMixQ; ++q) {
                const long long i = j * kMixTile + q * 64 + lane;
                st[r][q] = i < len[r] ? src[r][i] : (int16_t)0;
            }
    };
    const int row = lane & (kMixRows - 1); /* lanes past the rows walk one again and write nothing */
    float acc = 0.0f;
    if (ntile > 0) fetch(0);
    for (long long j = 0; j < ntile; ++j) {
        __syncthreads(); /* the walk of tile j - 1 is over */
#pragma unroll
        for (int r = 0; r < kMixRows; ++r)
#pragma unroll
            for (int q = 0; q < kMixQ; ++q) reinterpret_cast<int16_t *>(tile[r])[q * 64 + lane] = st[r][q];
        __syncthreads();
        if (j + 1 < ntile) fetch(j + 1); /* in flight during the walk */
#pragma unroll 8
        for (int k = 0; k < kMixTile / 2; ++k) {
            const uint32_t w = tile[row][k];
            acc = mix_acc(acc, (int)(int16_t)(w & 0xffffu));
            acc = mix_acc(acc, (int)(int16_t)(w >> 16));
        }
    }
    if (lane < kMixRows) {
        const int k = first + (lane & (kMixGroup - 1));
        if (k < a.n_utt) {
            const int u = a.order ? a.order[k] : k;
            a.sums[2 * (long long)u + (lane >= kMixGroup)] = acc;
        }
    }
}

__device__ __forceinline__ int16_t mix_to_short(float p)
{
    /* cvttss2si's "integer indefinite" 0x80000000 has a zero low half */
    const int v = fabsf(p) < 2147483648.0f ? (int)p : 0;
    return (int16_t)(uint16_t)((uint32_t)v & 0xffffu);
}

struct alignas(16) Short8 {
    int16_t v[8];
};

__global__ __launch_bounds__(kScaleThreads) void mix_scale_kernel(MixArgs a)
{
    __shared__ __attribute__((aligned(16))) int16_t ns[kScaleChunk];
    const int u = blockIdx.y, tid = threadIdx.x;
    const long long L = std::max(a.lengths[u], 0LL), off = a.offsets[u];
    const long long Lp = (L + 7) & ~7LL;
    const float pure = a.sums[2 * (long long)u], noise = a.sums[2 * (long long)u + 1];
    /* both divisions and the square root correctly rounded (see the head of this file) */
    const float gain = sqrtf((pure / noise) / a.snr_lin[u]);
    if (a.gain && blockIdx.x == 0 && tid == 0) a.gain[u] = gain;
    const int16_t *nsrc = a.noise_src + a.noise_start[u];
    for (long long c0 = (long long)blockIdx.x * kScaleChunk; c0 < Lp; c0 += (long long)gridDim.x * kScaleChunk) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kScalePer; ++k) {
            const long long i = c0 + k * kScaleThreads + tid;
            ns[k * kScaleThreads + tid] = i < L ? nsrc[i] : (int16_t)0;
        }
        __syncthreads();
        const long long i0 = c0 + (long long)tid * kScalePer;
        if (i0 < Lp) {
            const Short8 x = *reinterpret_cast<const Short8 *>(a.clean + off + i0);
            const Short8 n = *reinterpret_cast<const Short8 *>(&ns[tid * kScalePer]);
            Short8 s, y;
#pragma unroll
            for (int k = 0; k < kScalePer; ++k) {
                const bool in = i0 + k < L;
                const int16_t sc = in ? mix_to_short((float)n.v[k] * gain) : (int16_t)0;
                s.v[k] = sc;
                y.v[k] = in ? (int16_t)(uint16_t)(((int)x.v[k] + (int)sc) & 0xffff) : (int16_t)0;
            }
            *reinterpret_cast<Short8 *>(a.noise_scaled + off + i0) = s;
            *reinterpret_cast<Short8 *>(a.noisy + off + i0) = y;
        }
    }
}

/* the sums of a call that passes d_sums == NULL: grow-only, per host thread and device.  Two such calls of one thread share it:
 * they must not overlap on the device (one stream, or d_sums given); include/sea_mi355x.h says so */
struct SumsScratch {
    float *p = nullptr;
    size_t cap = 0;
    int device = -1;
    ~SumsScratch() { if (p) (void)hipFree(p); }
    int ensure(size_t n, float **out)
    {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (dev != device || n > cap) {
            if (p) HIP_TRY(hipFree(p)); /* waits for the launches that still use it */
            p = nullptr;
            cap = 0;
            HIP_TRY(hipMalloc(&p, n * sizeof(float)));
            cap = n;
            device = dev;
        }
        *out = p;
        return 0;
    }
};
thread_local SumsScratch t_sums;

int mix_launch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
               const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy, float *d_sums,
               float *d_gain, const int *d_order, int n_utt, hipStream_t stream)
{
    if (n_utt <= 0) return 0;
    if (!d_clean || !d_offsets || !d_lengths || !d_noise_src || !d_noise_start || !d_snr_lin || !d_noise_scaled || !d_noisy)
        return fail("addnoise: a required pointer is NULL");
    MixArgs a;
    a.clean = d_clean;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.noise_src = d_noise_src;
    a.noise_start = d_noise_start;
    a.snr_lin = d_snr_lin;
    a.noise_scaled = d_noise_scaled;
    a.noisy = d_noisy;
    a.sums = d_sums;
    a.gain = d_gain;
    a.order = d_order;
    a.n_utt = n_utt;
    if (!a.sums && t_sums.ensure(2 * (size_t)n_utt, &a.sums)) return 1;
    hipLaunchKernelGGL(mix_sums_kernel, dim3((unsigned)((n_utt + kMixGroup - 1) / kMixGroup)), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    /* grid.y is limited to 65535 */
    for (int u0 = 0; u0 < n_utt; u0 += 65535) {
        MixArgs b = a;
        const int n = std::min(n_utt - u0, 65535);
        b.offsets += u0;
        b.lengths += u0;
        b.noise_start += u0;
        b.snr_lin += u0;
        b.sums += 2 * (size_t)u0;
        if (b.gain) b.gain += u0;
        hipLaunchKernelGGL(mix_scale_kernel, dim3(kScaleBlocksX, (unsigned)n), dim3(kScaleThreads), 0, stream, b);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int trainset_launch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
                    const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy,
                    float *d_sums, float *d_gain, short *d_sub_clean, short *d_sub_noise, short *d_sub_noisy,
                    const long long *d_row_offsets, float *d_irm, int window, const int *d_order, int n_utt, void *stream)
{
    if (mix_launch(d_clean, d_offsets, d_lengths, d_noise_src, d_noise_start, d_snr_lin, d_noise_scaled, d_noisy, d_sums,
                   d_gain, d_order, n_utt, (hipStream_t)stream))
        return 1;
    if (sea_subband64_batch(d_clean, d_sub_clean, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    if (sea_subband64_batch(d_noise_scaled, d_sub_noise, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    if (d_sub_noisy && sea_subband64_batch(d_noisy, d_sub_noisy, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    return sea_irm_target_batch(d_sub_clean, d_sub_noise, d_offsets, d_lengths, d_row_offsets, d_irm, window, n_utt, stream);
}

float snr_lin_of(int db) { return (float)pow(10.0, db / 10.0); }

thread_local int t_last_chunks = 0;

} // namespace

extern "C" {

int sea_addnoise_batch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
                       const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy,
                       float *d_sums, float *d_gain, int n_utt, void *stream)
{
    return mix_launch(d_clean, d_offsets, d_lengths, d_noise_src, d_noise_start, d_snr_lin, d_noise_scaled, d_noisy, d_sums,
                      d_gain, nullptr, n_utt, (hipStream_t)stream);
}

int sea_addnoise(const short *clean, const short *noise, long L, int db, short *noise_scaled, short *noisy, float *sums2,
                 float *gain)
{
    if (L <= 0) return fail("addnoise: L=%ld", L);
    const long long Lp = align8(L);
    DevBuf<short> dc, dn, ds, dy;
    DevBuf<long long> dmeta;
    DevBuf<float> df;
    HIP_TRY(dc.alloc((size_t)Lp));
    HIP_TRY(dn.alloc((size_t)Lp));
    HIP_TRY(ds.alloc((size_t)Lp));
    HIP_TRY(dy.alloc((size_t)Lp));
    HIP_TRY(dmeta.alloc(3));
    HIP_TRY(df.alloc(4));
    const long long meta[3] = {0, L, 0};
    float f[4] = {snr_lin_of(db), 0, 0, 0};
    HIP_TRY(hipMemset(dc.p, 0, (size_t)Lp * sizeof(short)));
    HIP_TRY(hipMemcpy(dc.p, clean, (size_t)L * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dn.p, noise, (size_t)L * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmeta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(df.p, f, sizeof f, hipMemcpyHostToDevice));
    if (sea_addnoise_batch(dc.p, dmeta.p, dmeta.p + 1, dn.p, dmeta.p + 2, df.p, ds.p, dy.p, df.p + 1, df.p + 3, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    if (noise_scaled) HIP_TRY(hipMemcpy(noise_scaled, ds.p, (size_t)L * sizeof(short), hipMemcpyDeviceToHost));
    if (noisy) HIP_TRY(hipMemcpy(noisy, dy.p, (size_t)L * sizeof(short), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f, df.p, sizeof f, hipMemcpyDeviceToHost));
    if (sums2) sums2[0] = f[1], sums2[1] = f[2];
    if (gain) *gain = f[3];
    return 0;
}

int sea_trainset_batch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
                       const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy,
                       float *d_sums, float *d_gain, short *d_sub_clean, short *d_sub_noise, short *d_sub_noisy,
                       const long long *d_row_offsets, float *d_irm, int window, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (window < 0 || window > 2) return fail("trainset: window %d (0 rectangular, 1 Hamming, 2 Hanning)", window);
    if (!d_sub_clean || !d_sub_noise || !d_row_offsets || !d_irm || !d_lengths)
        return fail("trainset: a required pointer is NULL");
    /* make_single_IBM's frame count (L - 320) / 160 + 1 needs one frame: the lengths come back before anything is launched.
     * A capturing stream cannot be synchronised, and trying to would invalidate the caller's capture: refuse first, with the
     * capture left intact (the query is legal during capture) */
    if (stream) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &capturing));
        if (capturing != hipStreamCaptureStatusNone)
            return fail("trainset: the call reads the lengths back before it launches and cannot be captured in a graph "
                        "(capture sea_addnoise_batch, sea_subband64_batch and sea_irm_target_batch instead)");
    }
    std::vector<long long> lens((size_t)n_utt);
    HIP_TRY(hipMemcpyAsync(lens.data(), d_lengths, (size_t)n_utt * sizeof(long long), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int u = 0; u < n_utt; ++u)
        if (lens[u] < 320) return fail("trainset: utterance %d has %lld samples (shorter than one 320-sample frame)", u, lens[u]);
    return trainset_launch(d_clean, d_offsets, d_lengths, d_noise_src, d_noise_start, d_snr_lin, d_noise_scaled, d_noisy, d_sums,
                           d_gain, d_sub_clean, d_sub_noise, d_sub_noisy, d_row_offsets, d_irm, window, d_order, n_utt, stream);
}

int sea_trainset_last_chunks(void) { return t_last_chunks; }

/* Device footprint of a chunk: per padded sample 2 B each of clean, scaled noise and noisy plus 128 B per subband set
 * (two or three), per mask row 256 B, per utterance its metadata.  The budget (SEA_TRAINSET_SCRATCH_MB) is read after the
 * noise recordings went up.  The reference handles one utterance at a time; results do not depend on the cut. */
int sea_trainset_utterances(const short *const *clean, const long *lengths, int n_utt, const short *const *noises,
                            const long *noise_lengths, int n_noise, const int *rec, const long *off, const int *db, int window,
                            short *const *noisy, float *const *irm, short *const *noise_scaled, short *const *sub_clean,
                            short *const *sub_noise, short *const *sub_noisy)
{
    t_last_chunks = 0;
    if (n_utt <= 0) return 0;
    if (!clean || !lengths || !noises || !noise_lengths || !rec || !off || !db || !noisy || !irm)
        return fail("trainset: a required argument is NULL");
    if (window < 0 || window > 2) return fail("trainset: window %d (0 rectangular, 1 Hamming, 2 Hanning)", window);
    for (int r = 0; r < n_noise; ++r)
        if (noise_lengths[r] < 0 || (noise_lengths[r] > 0 && !noises[r])) return fail("trainset: noise recording %d is unusable", r);
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 320)
            return fail("trainset: utterance %d has %ld samples (shorter than one 320-sample frame)", u, lengths[u]);
        if (rec[u] < 0 || rec[u] >= n_noise) return fail("trainset: utterance %d names noise recording %d of %d", u, rec[u], n_noise);
        if (off[u] < 0 || off[u] > noise_lengths[rec[u]] - lengths[u])
            return fail("trainset: utterance %d (%ld samples) at offset %ld does not fit noise recording %d (%ld samples)", u,
                        lengths[u], off[u], rec[u], noise_lengths[rec[u]]);
        if (!clean[u] || !noisy[u] || !irm[u]) return fail("trainset: utterance %d has a NULL buffer", u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    const int nsets = sub_noisy ? 3 : 2;
    std::vector<long long> nbase((size_t)n_noise + 1, 0);
    for (int r = 0; r < n_noise; ++r) nbase[r + 1] = nbase[r] + noise_lengths[r];
    DevBuf<short> d_noise;
    HIP_TRY(d_noise.alloc((size_t)std::max(nbase[n_noise], 1LL)));
    for (int r = 0; r < n_noise; ++r)
        if (noise_lengths[r])
            HIP_TRY(hipMemcpy(d_noise.p + nbase[r], noises[r], (size_t)noise_lengths[r] * sizeof(short), hipMemcpyHostToDevice));

    long long budget;
    if (scratch_budget("SEA_TRAINSET_SCRATCH_MB", &budget)) return 1;
    auto rows_of = [](long L) -> long long { return (L - 320) / 160 + 1; };
    enum { S, R }; /* of an utterance: padded samples, rows, bytes */
    auto of = [&](int u) -> Totals<3> {
        const long long s = align8(lengths[u]), r = rows_of(lengths[u]);
        return {s, r, s * (6 + 128LL * nsets) + r * 256 + 64};
    };
    const ChunkPlan<3> plan = plan_chunks<3>(n_utt, budget, of);
    const size_t max_s = (size_t)plan.max[S], max_n = (size_t)plan.max_n;
    Staged<short> b_clean, b_noisy; /* b_noisy.h brings the scaled noise back as well */
    DevBuf<short> d_scaled, d_sub[3];
    Staged<float> b_irm, b_snr;
    DevBuf<float> d_sums;
    Staged<long long> b_meta; /* offsets, lengths, noise starts, row offsets */
    Staged<int> b_order;
    HIP_TRY(b_clean.alloc(max_s));
    HIP_TRY(d_scaled.alloc(max_s));
    HIP_TRY(b_noisy.alloc(max_s));
    for (int s = 0; s < nsets; ++s) HIP_TRY(d_sub[s].alloc(max_s * 64));
    HIP_TRY(b_irm.alloc((size_t)plan.max[R] * 64));
    HIP_TRY(b_snr.alloc(max_n));
    HIP_TRY(d_sums.alloc(2 * max_n));
    HIP_TRY(b_meta.alloc(4 * max_n));
    HIP_TRY(b_order.alloc(max_n));
    const long long *d_meta = b_meta.d.p;
    std::vector<short> &h_out = b_noisy.h;

    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *offs = b_meta.h.data(), *lens = offs + n, *nst = lens + n, *roff = nst + n;
        long long s = 0, r = 0;
        for (int j = 0; j < n; ++j) {
            const int u = u0 + j;
            offs[j] = s;
            lens[j] = lengths[u];
            nst[j] = nbase[rec[u]] + off[u];
            roff[j] = r;
            b_snr.h[j] = snr_lin_of(db[u]);
            s += pack_padded(b_clean.h.data() + s, clean[u], lens[j]);
            r += rows_of(lengths[u]);
        }
        launch_order(lens, n, dc->n_cu, b_order.h.data());
        HIP_TRY(hipMemcpy(b_clean.d.p, b_clean.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_meta.d.p, b_meta.h.data(), 4 * (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_snr.d.p, b_snr.h.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_order.d.p, b_order.h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        if (trainset_launch(b_clean.d.p, d_meta, d_meta + n, d_noise.p, d_meta + 2 * n, b_snr.d.p, d_scaled.p, b_noisy.d.p, d_sums.p,
                            nullptr, d_sub[0].p, d_sub[1].p, sub_noisy ? d_sub[2].p : nullptr, d_meta + 3 * n, b_irm.d.p, window,
                            b_order.d.p, n, nullptr))
            return 1;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out.data(), b_noisy.d.p, (size_t)s * sizeof(short), hipMemcpyDeviceToHost));
        for (int j = 0; j < n; ++j) memcpy(noisy[u0 + j], h_out.data() + offs[j], (size_t)lens[j] * sizeof(short));
        HIP_TRY(hipMemcpy(b_irm.h.data(), b_irm.d.p, (size_t)r * 64 * sizeof(float), hipMemcpyDeviceToHost));
        for (int j = 0; j < n; ++j)
            memcpy(irm[u0 + j], b_irm.h.data() + roff[j] * 64, (size_t)rows_of((long)lens[j]) * 64 * sizeof(float));
        if (noise_scaled) {
            HIP_TRY(hipMemcpy(h_out.data(), d_scaled.p, (size_t)s * sizeof(short), hipMemcpyDeviceToHost));
            for (int j = 0; j < n; ++j)
                if (noise_scaled[u0 + j]) memcpy(noise_scaled[u0 + j], h_out.data() + offs[j], (size_t)lens[j] * sizeof(short));
        }
        short *const *sets[3] = {sub_clean, sub_noise, sub_noisy};
        for (int t = 0; t < 3; ++t)
            if (sets[t])
                for (int j = 0; j < n; ++j)
                    if (sets[t][u0 + j]) {
                        const size_t L = (size_t)lens[j], Lp = (size_t)align8(lens[j]);
                        HIP_TRY(hipMemcpy2D(sets[t][u0 + j], L * sizeof(short), d_sub[t].p + offs[j] * 64, Lp * sizeof(short),
                                            L * sizeof(short), 64, hipMemcpyDeviceToHost));
                    }
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
