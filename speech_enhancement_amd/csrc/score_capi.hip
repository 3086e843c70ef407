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

long long halves_of(long long L, int hop) { return L / hop; }
long long frames_of(long long L, int hop) { return L < 2 * hop ? 0 : (L - 2 * hop) / hop + 1; }

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
    if (scratch_budget("SEA_SCORE_SCRATCH_MB", &budget)) return 1;
    enum { S, F, T }; /* of an utterance: padded samples, frames, tiles, bytes */
    auto of = [&](int u) -> Totals<4> {
        const long long L = lengths[u], s = align8(L), f = frames_of(L, hop), t = tiles_of(halves_of(L, hop), sea::kScoreTileHalves);
        return {s, f, t, s * 4 + f * 4 + t * sea::kScoreWaves * 24 + 96};
    };
    const ChunkPlan<4> plan = plan_chunks<4>(n_utt, budget, of);
    const size_t max_n = (size_t)plan.max_n;
    if (plan.max[T] > 0x7fffffffLL) return fail("score: %lld tiles in one launch", plan.max[T]);
    Staged<short> b_ref, b_est;
    Staged<float> b_db;
    Staged<long long> b_meta; /* offsets [n], lengths [n], frame offsets [n + 1], tile prefix [n + 1] */
    DevBuf<long long> d_part, d_sums;
    DevBuf<double> d_seg;
    DevBuf<int> d_used;
    HIP_TRY(b_ref.alloc((size_t)plan.max[S]));
    HIP_TRY(b_est.alloc((size_t)plan.max[S]));
    HIP_TRY(b_db.alloc((size_t)plan.max[F], frame_db != nullptr));
    HIP_TRY(d_part.alloc((size_t)plan.max[T] * sea::kScoreWaves * 3));
    HIP_TRY(b_meta.alloc(4 * max_n + 2));
    HIP_TRY(d_sums.alloc(3 * max_n));
    HIP_TRY(d_seg.alloc(max_n));
    HIP_TRY(d_used.alloc(max_n));
    const long long *d_meta = b_meta.d.p;
    hipStream_t stream = nullptr;
    EventSet<3> ev;
    if (ev.create()) return 1;
    t_stage_ms[SEA_SCORE_STAGE_FRAMES] = t_stage_ms[SEA_SCORE_STAGE_FINISH] = 0.0;
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *offs = b_meta.h.data(), *lens = offs + n, *foff = lens + n, *tcum = foff + n + 1;
        long long s = 0, f = 0, t = 0;
        for (int j = 0; j < n; ++j) {
            const Totals<4> q = of(u0 + j);
            offs[j] = s, lens[j] = lengths[u0 + j], foff[j] = f, tcum[j] = t;
            pack_padded(b_ref.h.data() + s, ref[u0 + j], lens[j]);
            pack_padded(b_est.h.data() + s, est[u0 + j], lens[j]);
            s += q[S], f += q[F], t += q[T];
        }
        foff[n] = f, tcum[n] = t;
        if (s > 0) {
            HIP_TRY(hipMemcpyAsync(b_ref.d.p, b_ref.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(b_est.d.p, b_est.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipMemcpyAsync(b_meta.d.p, b_meta.h.data(), (4 * (size_t)n + 2) * sizeof(long long), hipMemcpyHostToDevice, stream));
        sea::ScoreArgs a;
        a.ref = b_ref.d.p, a.est = b_est.d.p;
        a.offsets = d_meta, a.lengths = d_meta + n, a.frame_offsets = d_meta + 2 * n, a.tile_cum = d_meta + 3 * n + 1;
        a.frame_db = b_db.d.p, a.partials = d_part.p;
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
        if (frame_db && f > 0) HIP_TRY(hipMemcpyAsync(b_db.h.data(), b_db.d.p, (size_t)f * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int st = 0; st < 2; ++st)
            if (ev.add_ms(st, st + 1, &t_stage_ms[st])) return 1;
        if (frame_db)
            for (int j = 0; j < n; ++j)
                if (frame_db[u0 + j] && foff[j + 1] > foff[j])
                    memcpy(frame_db[u0 + j], b_db.h.data() + foff[j], (size_t)(foff[j + 1] - foff[j]) * sizeof(float));
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
    if (scratch_budget("SEA_SCORE_SCRATCH_MB", &budget)) return 1;
    enum { R, T }; /* of an utterance: rows, tiles, bytes */
    auto of = [&](int u) -> Totals<3> { return {n_rows[u], tiles_of(n_rows[u], sea::kMaskTileRows), n_rows[u] * 512LL + 48}; };
    const ChunkPlan<3> plan = plan_chunks<3>(n_utt, budget, of);
    if (plan.max[T] > 0x7fffffffLL) return fail("mask_score: %lld tiles in one launch", plan.max[T]);
    Staged<float> b_est, b_ideal;
    Staged<long long> b_meta; /* row offsets [n + 1], tile prefix [n + 1] */
    DevBuf<unsigned long long> d_counts;
    HIP_TRY(b_est.alloc((size_t)plan.max[R] * 64));
    HIP_TRY(b_ideal.alloc((size_t)plan.max[R] * 64));
    HIP_TRY(b_meta.alloc(2 * (size_t)plan.max_n + 2));
    HIP_TRY(d_counts.alloc(4 * (size_t)plan.max_n));
    hipStream_t stream = nullptr;
    EventSet<2> ev;
    if (ev.create()) return 1;
    t_stage_ms[SEA_SCORE_STAGE_MASK] = 0.0;
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *roff = b_meta.h.data(), *tcum = roff + n + 1;
        long long r = 0, t = 0;
        for (int j = 0; j < n; ++j) {
            const Totals<3> q = of(u0 + j);
            roff[j] = r, tcum[j] = t;
            if (q[R] > 0) {
                memcpy(b_est.h.data() + r * 64, est[u0 + j], (size_t)q[R] * 64 * sizeof(float));
                memcpy(b_ideal.h.data() + r * 64, ideal[u0 + j], (size_t)q[R] * 64 * sizeof(float));
            }
            r += q[R], t += q[T];
        }
        roff[n] = r, tcum[n] = t;
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, 4 * (size_t)n * sizeof(unsigned long long), stream));
        if (t > 0) {
            HIP_TRY(hipMemcpyAsync(b_est.d.p, b_est.h.data(), (size_t)r * 64 * sizeof(float), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(b_ideal.d.p, b_ideal.h.data(), (size_t)r * 64 * sizeof(float), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(b_meta.d.p, b_meta.h.data(), (2 * (size_t)n + 2) * sizeof(long long), hipMemcpyHostToDevice, stream));
            sea::MaskScoreArgs a;
            a.est = b_est.d.p, a.ideal = b_ideal.d.p;
            a.row_offsets = b_meta.d.p, a.tile_cum = b_meta.d.p + n + 1;
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
        if (t > 0 && ev.add_ms(0, 1, &t_stage_ms[SEA_SCORE_STAGE_MASK])) return 1;
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
