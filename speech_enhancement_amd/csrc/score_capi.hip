/*
 * score_capi.hip -- the C ABI of the objective scores (include/sea_mi355x.h): lists of utterances from
 * host memory, staged in chunks of whole utterances that fit the device, scored by the kernels of score_kernel.hip.  Host
 * pointers only.
 */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "score_kernels.h"

using namespace sea_capi;

namespace {

thread_local int t_last_chunks = 0;
constexpr int kStages = SEA_SCORE_STAGE_COUNT;
thread_local double t_stage_ms[kStages] = {};

struct Events {
    hipEvent_t e[3] = {};
    ~Events()
    {
        for (hipEvent_t ev : e)
            if (ev) (void)hipEventDestroy(ev);
    }
    int create()
    {
        for (hipEvent_t &ev : e) HIP_TRY(hipEventCreate(&ev));
        return 0;
    }
};

/* 60 % of the HBM that is free now, as sea_dnn_enhance_utterances; SEA_SCORE_SCRATCH_MB overrides it */
int score_budget(long long *budget)
{
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = (long long)(free_b / 10 * 6);
    if (const char *e = getenv("SEA_SCORE_SCRATCH_MB")) *budget = atoll(e) * (1LL << 20);
    return 0;
}

/* whole utterances in list order, cut where the next one would pass the budget; an utterance larger than the budget forms a
 * chunk of its own and hipMalloc reports what does not fit */
template <typename Bytes>
std::vector<int> cut_list(int n_utt, long long budget, Bytes bytes_of)
{
    std::vector<int> cuts(1, 0);
    long long run = 0;
    for (int u = 0; u < n_utt; ++u) {
        const long long b = bytes_of(u);
        if (u > cuts.back() && run + b > budget) {
            cuts.push_back(u);
            run = 0;
        }
        run += b;
    }
    cuts.push_back(n_utt);
    return cuts;
}

long long halves_of(long long L, int hop) { return L / hop; }
long long frames_of(long long L, int hop) { return L < 2 * hop ? 0 : (L - 2 * hop) / hop + 1; }
long long tiles_of(long long n, int per) { return (n + per - 1) / per; }

} // namespace

extern "C" {

int sea_score_last_chunks(void) { return t_last_chunks; }

double sea_score_last_stage_ms(int stage) { return stage >= 0 && stage < kStages ? t_stage_ms[stage] : -1.0; }

/* Device footprint of a chunk: per padded sample 4 B of audio (ref and est), per frame 4 B of frame_db, per 252 half-frames
 * four wave partials of 24 B, per utterance four table entries and its results */
int sea_score_utterances(const short *const *ref, const short *const *est, const long *lengths, int n_utt, int hop, long long *sums,
                         double *seg_sum, int *seg_frames, float *const *frame_db)
{
    t_last_chunks = 0;
    if (n_utt < 0) return fail("score: n_utt = %d", n_utt);
    if (hop != 80 && hop != 160) return fail("score: hop = %d (80 at 8 kHz, 160 at 16 kHz)", hop);
    if (n_utt == 0) return 0;
    if (!ref || !est || !lengths || !sums || !seg_sum || !seg_frames) return fail("score: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0 || (long long)lengths[u] > 0x7fffffffLL) return fail("score: utterance %d has %ld samples (0 .. 2^31 - 1)", u, lengths[u]);
        if (lengths[u] > 0 && (!ref[u] || !est[u])) return fail("score: utterance %d has a NULL buffer", u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    long long budget;
    if (score_budget(&budget)) return 1;
    const std::vector<int> cuts = cut_list(n_utt, budget, [&](int u) -> long long {
        const long long L = lengths[u];
        return align8(L) * 4 + frames_of(L, hop) * 4 + tiles_of(halves_of(L, hop), sea::kScoreTileHalves) * sea::kScoreWaves * 24 + 96;
    });
    const int nchunk = (int)cuts.size() - 1;
    long long max_s = 0, max_f = 0, max_t = 0;
    int max_n = 0;
    for (int k = 0; k < nchunk; ++k) {
        long long s = 0, f = 0, t = 0;
        for (int u = cuts[k]; u < cuts[k + 1]; ++u) {
            s += align8(lengths[u]), f += frames_of(lengths[u], hop);
            t += tiles_of(halves_of(lengths[u], hop), sea::kScoreTileHalves);
        }
        max_s = std::max(max_s, s), max_f = std::max(max_f, f), max_t = std::max(max_t, t);
        max_n = std::max(max_n, cuts[k + 1] - cuts[k]);
    }
    if (max_t > 0x7fffffffLL) return fail("score: %lld tiles in one launch", max_t);
    DevBuf<short> d_ref, d_est;
    DevBuf<float> d_db;
    DevBuf<long long> d_meta, d_part, d_sums; /* meta: offsets [n], lengths [n], frame offsets [n + 1], tile prefix [n + 1] */
    DevBuf<double> d_seg;
    DevBuf<int> d_used;
    HIP_TRY(d_ref.alloc((size_t)max_s));
    HIP_TRY(d_est.alloc((size_t)max_s));
    HIP_TRY(d_db.alloc((size_t)max_f));
    HIP_TRY(d_part.alloc((size_t)max_t * sea::kScoreWaves * 3));
    HIP_TRY(d_meta.alloc(4 * (size_t)max_n + 2));
    HIP_TRY(d_sums.alloc(3 * (size_t)max_n));
    HIP_TRY(d_seg.alloc((size_t)max_n));
    HIP_TRY(d_used.alloc((size_t)max_n));
    std::vector<short> h_ref((size_t)max_s), h_est((size_t)max_s);
    std::vector<float> h_db(frame_db ? (size_t)max_f : 0);
    std::vector<long long> h_meta(4 * (size_t)max_n + 2);
    hipStream_t stream = nullptr;
    Events ev;
    if (ev.create()) return 1;
    t_stage_ms[SEA_SCORE_STAGE_FRAMES] = t_stage_ms[SEA_SCORE_STAGE_FINISH] = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const int u0 = cuts[k], n = cuts[k + 1] - u0;
        long long *offs = h_meta.data(), *lens = offs + n, *foff = lens + n, *tcum = foff + n + 1;
        long long s = 0, f = 0, t = 0;
        for (int j = 0; j < n; ++j) {
            const long long L = lengths[u0 + j], Lp = align8(L);
            offs[j] = s, lens[j] = L, foff[j] = f, tcum[j] = t;
            if (L > 0) {
                memcpy(h_ref.data() + s, ref[u0 + j], (size_t)L * sizeof(short));
                memcpy(h_est.data() + s, est[u0 + j], (size_t)L * sizeof(short));
            }
            if (Lp > L) {
                memset(h_ref.data() + s + L, 0, (size_t)(Lp - L) * sizeof(short));
                memset(h_est.data() + s + L, 0, (size_t)(Lp - L) * sizeof(short));
            }
            s += Lp, f += frames_of(L, hop), t += tiles_of(halves_of(L, hop), sea::kScoreTileHalves);
        }
        foff[n] = f, tcum[n] = t;
        if (s > 0) {
            HIP_TRY(hipMemcpyAsync(d_ref.p, h_ref.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_est.p, h_est.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipMemcpyAsync(d_meta.p, h_meta.data(), (4 * (size_t)n + 2) * sizeof(long long), hipMemcpyHostToDevice, stream));
        sea::ScoreArgs a;
        a.ref = d_ref.p, a.est = d_est.p;
        a.offsets = d_meta.p, a.lengths = d_meta.p + n, a.frame_offsets = d_meta.p + 2 * n, a.tile_cum = d_meta.p + 3 * n + 1;
        a.frame_db = d_db.p, a.partials = d_part.p;
        a.sums = d_sums.p, a.seg_sum = d_seg.p, a.seg_frames = d_used.p;
        a.n_utt = n, a.hop = hop;
        HIP_TRY(hipEventRecord(ev.e[0], stream));
        if (t > 0) { /* the grid is the work: one workgroup per (utterance, tile of 252 half-frames) */
            if (hop == 160) hipLaunchKernelGGL(sea::score_frames_kernel<160>, dim3((unsigned)t), dim3(256), 0, stream, a);
            else hipLaunchKernelGGL(sea::score_frames_kernel<80>, dim3((unsigned)t), dim3(256), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev.e[1], stream));
        hipLaunchKernelGGL(sea::score_finish_kernel, dim3((unsigned)n), dim3(64), 0, stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[2], stream));
        HIP_TRY(hipMemcpyAsync(sums + 3 * (size_t)u0, d_sums.p, 3 * (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(seg_sum + u0, d_seg.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(seg_frames + u0, d_used.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (frame_db && f > 0) HIP_TRY(hipMemcpyAsync(h_db.data(), d_db.p, (size_t)f * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int st = 0; st < 2; ++st) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.e[st], ev.e[st + 1]));
            t_stage_ms[st] += ms;
        }
        if (frame_db)
            for (int j = 0; j < n; ++j)
                if (frame_db[u0 + j] && foff[j + 1] > foff[j])
                    memcpy(frame_db[u0 + j], h_db.data() + foff[j], (size_t)(foff[j + 1] - foff[j]) * sizeof(float));
        t_last_chunks = k + 1;
    }
    return 0;
}

/* Device footprint of a chunk: per row 512 B of masks, per utterance two table entries and four counts */
int sea_mask_score_utterances(const float *const *est, const float *const *ideal, const int *n_rows, int n_utt, float t_est,
                              float t_ideal, long long *counts)
{
    t_last_chunks = 0;
    if (n_utt < 0) return fail("mask_score: n_utt = %d", n_utt);
    if (!std::isfinite(t_est) || !std::isfinite(t_ideal)) return fail("mask_score: a threshold is not finite");
    if (n_utt == 0) return 0;
    if (!est || !ideal || !n_rows || !counts) return fail("mask_score: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (n_rows[u] < 0) return fail("mask_score: utterance %d has %d rows", u, n_rows[u]);
        if (n_rows[u] > 0 && (!est[u] || !ideal[u])) return fail("mask_score: utterance %d has a NULL buffer", u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    long long budget;
    if (score_budget(&budget)) return 1;
    const std::vector<int> cuts = cut_list(n_utt, budget, [&](int u) -> long long { return n_rows[u] * 512LL + 48; });
    const int nchunk = (int)cuts.size() - 1;
    long long max_r = 0, max_t = 0;
    int max_n = 0;
    for (int k = 0; k < nchunk; ++k) {
        long long r = 0, t = 0;
        for (int u = cuts[k]; u < cuts[k + 1]; ++u) r += n_rows[u], t += tiles_of(n_rows[u], sea::kMaskTileRows);
        max_r = std::max(max_r, r), max_t = std::max(max_t, t), max_n = std::max(max_n, cuts[k + 1] - cuts[k]);
    }
    if (max_t > 0x7fffffffLL) return fail("mask_score: %lld tiles in one launch", max_t);
    DevBuf<float> d_est, d_ideal;
    DevBuf<long long> d_meta; /* row offsets [n + 1], tile prefix [n + 1] */
    DevBuf<unsigned long long> d_counts;
    HIP_TRY(d_est.alloc((size_t)max_r * 64));
    HIP_TRY(d_ideal.alloc((size_t)max_r * 64));
    HIP_TRY(d_meta.alloc(2 * (size_t)max_n + 2));
    HIP_TRY(d_counts.alloc(4 * (size_t)max_n));
    std::vector<float> h_est((size_t)max_r * 64), h_ideal((size_t)max_r * 64);
    std::vector<long long> h_meta(2 * (size_t)max_n + 2);
    hipStream_t stream = nullptr;
    Events ev;
    if (ev.create()) return 1;
    t_stage_ms[SEA_SCORE_STAGE_MASK] = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const int u0 = cuts[k], n = cuts[k + 1] - u0;
        long long *roff = h_meta.data(), *tcum = roff + n + 1;
        long long r = 0, t = 0;
        for (int j = 0; j < n; ++j) {
            const long long rows = n_rows[u0 + j];
            roff[j] = r, tcum[j] = t;
            if (rows > 0) {
                memcpy(h_est.data() + r * 64, est[u0 + j], (size_t)rows * 64 * sizeof(float));
                memcpy(h_ideal.data() + r * 64, ideal[u0 + j], (size_t)rows * 64 * sizeof(float));
            }
            r += rows, t += tiles_of(rows, sea::kMaskTileRows);
        }
        roff[n] = r, tcum[n] = t;
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, 4 * (size_t)n * sizeof(unsigned long long), stream));
        if (t > 0) {
            HIP_TRY(hipMemcpyAsync(d_est.p, h_est.data(), (size_t)r * 64 * sizeof(float), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_ideal.p, h_ideal.data(), (size_t)r * 64 * sizeof(float), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_meta.p, h_meta.data(), (2 * (size_t)n + 2) * sizeof(long long), hipMemcpyHostToDevice, stream));
            sea::MaskScoreArgs a;
            a.est = d_est.p, a.ideal = d_ideal.p;
            a.row_offsets = d_meta.p, a.tile_cum = d_meta.p + n + 1;
            a.counts = d_counts.p;
            a.t_est = t_est, a.t_ideal = t_ideal;
            a.n_utt = n;
            HIP_TRY(hipEventRecord(ev.e[0], stream));
            hipLaunchKernelGGL(sea::mask_score_kernel, dim3((unsigned)t), dim3(256), 0, stream, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev.e[1], stream));
        }
        static_assert(sizeof(long long) == sizeof(unsigned long long), "counts are copied as they are");
        HIP_TRY(hipMemcpyAsync(counts + 4 * (size_t)u0, d_counts.p, 4 * (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (t > 0) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
            t_stage_ms[SEA_SCORE_STAGE_MASK] += ms;
        }
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
