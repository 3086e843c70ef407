/*
 * hw64_resynth_capi.hip -- the C ABI of the Hu-Wang resynthesis at 16 kHz on the 64-channel bank (hw64_resynth_kernel.hip):
 * sea_hw64_resynth_tables_host, the single-utterance forms sea_hw64_resynth and sea_hw64_enhance, the forms that take lists of
 * utterances in host memory, sea_hw64_resynth_utterances and sea_hw64_enhance_utterances, with the plan that cuts a list into
 * chunks that fit HBM (sea_hw64_enhance_plan, sea_hw64_enhance_last_chunks, sea_hw64_enhance_last_resynth_ms).  Every exported
 * call takes host pointers.  The batch launches on device pointers and a stream are the shared ones of hw_bank.h on the
 * 64-channel bank, resynth_launch and enhance_launch: each chunk of a list is one launch group of them, and a single utterance
 * is a list of one.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hw_bank.h"

using namespace sea_capi;

namespace {

constexpr int kCh = SEA_HW64_NCHAN;

thread_local int t_last_chunks = 0;
thread_local double t_last_resynth_ms = 0.0;

long long rows_of(long L) { return L > 0 ? L / SEA_HW64_HOP : 0; }

/* Device footprint of a chunk of n utterances with s padded samples and r mask rows in all: what the launch group works in --
 * the estimator's scratch, or for the resynthesis alone the three [64][pitch] planes hOut, hEv and gOut -- and its I/O buffers:
 * 10 B per padded sample (float in, float out, int16 out), 260 B per row (mask, pitch), 32 B per utterance (offsets, lengths,
 * row offsets, launch order, status). */
long long work_bytes(long long s, long long r, int n, int resynth_only)
{
    return resynth_only ? 3 * s * kCh * 4 : sea_hw64_ibm_scratch_bytes(s, r, n);
}
long long chunk_bytes(long long s, long long r, int n, int resynth_only)
{
    return work_bytes(s, r, n, resynth_only) + 10 * s + 260 * r + 32LL * n;
}

enum { S, R }; /* of an utterance: padded samples, mask rows */

/* the cut of chunk_plan.h over a footprint that is a function of the chunk's totals, not a sum over its utterances */
ChunkPlan<2> plan(const long *lengths, int n_utt, long long budget, int resynth_only)
{
    return plan_chunks<2>(
        n_utt, budget, [&](int u) -> Totals<2> { return {align8(lengths[u]), rows_of(lengths[u])}; },
        [&](const Totals<2> &c, int n) { return chunk_bytes(c[S], c[R], n, resynth_only); });
}

/* What both list forms share: the cut, the device and host buffers sized once for the largest chunk, and a chunk's way up
 * (samples zero-padded to a multiple of 8, offsets | lengths | row offsets, the LPT launch order) and down (float and int16
 * audio scattered to the callers' buffers). */
struct List {
    const float *const *in;
    const long *lengths;
    int n_utt, n_cu = 256;
    ChunkPlan<2> p;
    long long max_s = 0, max_r = 0, max_work = 0;
    int max_n = 0;
    Staged<float> f32, mask; /* f32: the input on the way up, the float output on the way down */
    DevBuf<float> d_out;
    Staged<short> i16;
    Staged<long long> meta;
    Staged<int> order;
    /* the chunk in hand */
    int u0 = 0, n = 0;
    long long s = 0, r = 0;
    const long long *offs = nullptr, *lens = nullptr, *roff = nullptr;

    int setup(const char *what, const float *const *in_, const long *lengths_, int n_utt_, float *const *out_f32, short *const *out_i16,
              int resynth_only)
    {
        in = in_;
        lengths = lengths_;
        n_utt = n_utt_;
        if (!in || !lengths) return fail("%s: null pointer", what);
        if (!out_f32 && !out_i16) return fail("%s: no output (out_f32 and out_i16 are both null)", what);
        for (int u = 0; u < n_utt; ++u) {
            if (lengths[u] < 0) return fail("%s: utterance %d has length %ld", what, u, lengths[u]);
            if (lengths[u] > 0 && (!in[u] || (out_f32 && !out_f32[u]) || (out_i16 && !out_i16[u])))
                return fail("%s: utterance %d has a null buffer", what, u);
        }
        DeviceCtx *dc;
        if (ctx(&dc)) return 1;
        n_cu = dc->n_cu;
        long long budget = 0;
        if (scratch_budget("SEA_HW64_ENHANCE_SCRATCH_MB", &budget)) return 1;
        p = plan(lengths, n_utt, budget, resynth_only);
        max_s = p.max[S], max_r = p.max[R], max_n = p.max_n;
        for (int k = 0; k < p.chunks(); ++k)
            max_work = std::max(max_work, work_bytes(p.sum[k][S], p.sum[k][R], p.cuts[k + 1] - p.cuts[k], resynth_only));
        HIP_TRY(f32.alloc((size_t)max_s));
        if (out_f32) HIP_TRY(d_out.alloc((size_t)max_s));
        if (out_i16) HIP_TRY(i16.alloc((size_t)max_s));
        HIP_TRY(mask.alloc((size_t)(max_r + 1) * kCh));
        HIP_TRY(meta.alloc(3 * (size_t)max_n));
        HIP_TRY(order.alloc((size_t)max_n));
        return 0;
    }

    int chunks() const { return p.chunks(); }

    int upload(int k)
    {
        u0 = p.cuts[k];
        n = p.cuts[k + 1] - u0;
        long long *o = meta.h.data(), *l = o + n, *ro = l + n;
        s = r = 0;
        for (int j = 0; j < n; ++j) {
            const long L = lengths[u0 + j];
            o[j] = s;
            l[j] = L;
            ro[j] = r;
            s += pack_padded(f32.h.data() + s, in[u0 + j], L);
            r += rows_of(L);
        }
        launch_order(l, n, n_cu, order.h.data());
        if (s > 0) HIP_TRY(hipMemcpy(f32.d.p, f32.h.data(), (size_t)s * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(meta.d.p, meta.h.data(), 3 * (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(order.d.p, order.h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        offs = meta.d.p;
        lens = offs + n;
        roff = offs + 2 * n;
        return 0;
    }

    int audio_back(float *const *out_f32, short *const *out_i16)
    {
        const long long *o = meta.h.data(), *l = o + n;
        if (out_f32 && s > 0) {
            HIP_TRY(hipMemcpy(f32.h.data(), d_out.p, (size_t)s * sizeof(float), hipMemcpyDeviceToHost));
            for (int j = 0; j < n; ++j)
                if (l[j] > 0) memcpy(out_f32[u0 + j], f32.h.data() + o[j], (size_t)l[j] * sizeof(float));
        }
        if (out_i16 && s > 0) {
            HIP_TRY(hipMemcpy(i16.h.data(), i16.d.p, (size_t)s * sizeof(short), hipMemcpyDeviceToHost));
            for (int j = 0; j < n; ++j)
                if (l[j] > 0) memcpy(out_i16[u0 + j], i16.h.data() + o[j], (size_t)l[j] * sizeof(short));
        }
        return 0;
    }
};

/* periphery with gOut, then the resynthesis of the callers' masks: one launch group per chunk */
int resynth_list(const float *const *in, const long *lengths, const float *const *masks, float threshold, float *const *out_f32,
                 short *const *out_i16, int n_utt, int *chunks)
{
    const char *what = "hw64_resynth_utterances";
    List q;
    if (q.setup(what, in, lengths, n_utt, out_f32, out_i16, 1)) return 1;
    for (int u = 0; u < n_utt; ++u)
        if (rows_of(lengths[u]) > 0 && (!masks || !masks[u])) return fail("%s: utterance %d has no mask", what, u);
    const size_t plane = (size_t)q.max_s * kCh;
    DevBuf<float> d_planes; /* hout | hev | gout */
    HIP_TRY(d_planes.alloc(3 * plane));
    EventSet<2> timer; /* around the resynthesis launch, which is not exported: sea_hw64_enhance_last_resynth_ms */
    if (timer.create()) return 1;
    for (int k = 0; k < q.chunks(); ++k) {
        if (q.upload(k)) return 1;
        if (q.s > 0) {
            const long long *ro = q.meta.h.data() + 2 * q.n;
            for (int j = 0; j < q.n; ++j) {
                const size_t units = (size_t)rows_of(lengths[q.u0 + j]) * kCh;
                if (units) memcpy(q.mask.h.data() + ro[j] * kCh, masks[q.u0 + j], units * sizeof(float));
            }
            if (q.r > 0) HIP_TRY(hipMemcpy(q.mask.d.p, q.mask.h.data(), (size_t)q.r * kCh * sizeof(float), hipMemcpyHostToDevice));
            float *gout = d_planes.p + 2 * plane;
            if (sea_hw64_periphery_batch(q.f32.d.p, d_planes.p, d_planes.p + plane, gout, q.offs, q.lens, q.order.d.p, q.n, nullptr))
                return 1;
            HIP_TRY(hipEventRecord(timer.e[0], nullptr));
            if (resynth_launch<Bank64>(gout, q.mask.d.p, q.offs, q.lens, q.roff, threshold, q.d_out.p, q.i16.d.p, q.order.d.p, q.n, nullptr))
                return 1;
            HIP_TRY(hipEventRecord(timer.e[1], nullptr));
            HIP_TRY(hipDeviceSynchronize());
            if (timer.add_ms(0, 1, &t_last_resynth_ms)) return 1;
            if (q.audio_back(out_f32, out_i16)) return 1;
        }
        *chunks = k + 1;
    }
    return 0;
}

/* sea_hw64_ibm_batch, then the resynthesis of its own mask from the gOut it keeps in its scratch: one launch group per chunk */
int enhance_list(const float *const *in, const long *lengths, int n_utt, float *const *out_f32, short *const *out_i16,
                 float *const *masks, int *const *pitch, int *status, int *chunks)
{
    const char *what = "hw64_enhance_utterances";
    if (!status) return fail("%s: null pointer", what);
    List q;
    if (q.setup(what, in, lengths, n_utt, out_f32, out_i16, 0)) return 1;
    DevBuf<int> d_int; /* pitch | status */
    DevBuf<char> d_scr;
    HIP_TRY(d_int.alloc((size_t)(q.max_r + 1) + (size_t)q.max_n));
    HIP_TRY(d_scr.alloc((size_t)q.max_work));
    std::vector<int> h_int((size_t)(q.max_r + 1) + (size_t)q.max_n);
    int *d_pitch = d_int.p, *d_status = d_int.p + q.max_r + 1;
    EventSet<2> timer; /* around the resynthesis launch, which is not exported: sea_hw64_enhance_last_resynth_ms */
    if (timer.create()) return 1;
    for (int k = 0; k < q.chunks(); ++k) {
        if (q.upload(k)) return 1;
        if (q.s == 0) { /* no sample in the whole chunk: nothing to compute */
            for (int j = 0; j < q.n; ++j) status[q.u0 + j] = 0;
            *chunks = k + 1;
            continue;
        }
        if (enhance_launch<Bank64>(q.f32.d.p, q.offs, q.lens, q.roff, q.d_out.p, q.i16.d.p, q.mask.d.p, d_pitch, d_status, d_scr.p, q.s, q.r,
                                q.order.d.p, q.n, nullptr, timer.e[0], timer.e[1]))
            return 1;
        HIP_TRY(hipDeviceSynchronize());
        if (timer.add_ms(0, 1, &t_last_resynth_ms)) return 1;
        HIP_TRY(hipMemcpy(status + q.u0, d_status, (size_t)q.n * sizeof(int), hipMemcpyDeviceToHost));
        if (q.audio_back(out_f32, out_i16)) return 1;
        const long long *ro = q.meta.h.data() + 2 * q.n;
        if (masks && q.r > 0) {
            HIP_TRY(hipMemcpy(q.mask.h.data(), q.mask.d.p, (size_t)q.r * kCh * sizeof(float), hipMemcpyDeviceToHost));
            for (int j = 0; j < q.n; ++j) {
                const size_t units = (size_t)rows_of(lengths[q.u0 + j]) * kCh;
                if (units && masks[q.u0 + j]) memcpy(masks[q.u0 + j], q.mask.h.data() + ro[j] * kCh, units * sizeof(float));
            }
        }
        if (pitch && q.r > 0) {
            HIP_TRY(hipMemcpy(h_int.data(), d_pitch, (size_t)q.r * sizeof(int), hipMemcpyDeviceToHost));
            for (int j = 0; j < q.n; ++j) {
                const size_t rows = (size_t)rows_of(lengths[q.u0 + j]);
                if (rows && pitch[q.u0 + j]) memcpy(pitch[q.u0 + j], h_int.data() + ro[j], rows * sizeof(int));
            }
        }
        *chunks = k + 1;
    }
    return 0;
}

} // namespace

int sea_hw64_resynth_tables_host(float *w640, double *up160, double *down160)
{
    sea_hw64_ola_tables(w640, up160, down160);
    return 0;
}

int sea_hw64_enhance_plan(const long *lengths, int n_utt, long long budget_bytes, int resynth_only, int *cuts)
{
    if (n_utt <= 0) return 0;
    if (!lengths) return fail("hw64_enhance_plan: null pointer"), -1;
    for (int u = 0; u < n_utt; ++u)
        if (lengths[u] < 0) return fail("hw64_enhance_plan: utterance %d has length %ld", u, lengths[u]), -1;
    const ChunkPlan<2> p = plan(lengths, n_utt, budget_bytes, resynth_only);
    if (cuts) std::copy(p.cuts.begin(), p.cuts.end(), cuts);
    return p.chunks();
}

int sea_hw64_enhance_last_chunks(void) { return t_last_chunks; }

double sea_hw64_enhance_last_resynth_ms(void) { return t_last_resynth_ms; }

int sea_hw64_resynth_utterances(const float *const *in, const long *lengths, const float *const *masks, float threshold,
                                float *const *out_f32, short *const *out_i16, int n_utt)
{
    t_last_chunks = 0;
    t_last_resynth_ms = 0.0;
    if (n_utt <= 0) return 0;
    return resynth_list(in, lengths, masks, threshold, out_f32, out_i16, n_utt, &t_last_chunks);
}

int sea_hw64_enhance_utterances(const float *const *in, const long *lengths, int n_utt, float *const *out_f32, short *const *out_i16,
                                float *const *masks, int *const *pitch, int *status)
{
    t_last_chunks = 0;
    t_last_resynth_ms = 0.0;
    if (n_utt <= 0) return 0;
    return enhance_list(in, lengths, n_utt, out_f32, out_i16, masks, pitch, status, &t_last_chunks);
}

int sea_hw64_resynth(const float *x, long L, const float *mask, long F, float threshold, float *out_f32)
{
    if (L < 0) return fail("hw64_resynth: L=%ld", L);
    if (L == 0) return 0;
    if (!x || !out_f32) return fail("hw64_resynth: null pointer");
    if (F != (long)sea_hw64_frames(L)) return fail("hw64_resynth: F=%ld, not L / 160 = %lld", F, sea_hw64_frames(L));
    if (F > 0 && !mask) return fail("hw64_resynth: null pointer");
    int chunks = 0;
    return resynth_list(&x, &L, &mask, threshold, &out_f32, nullptr, 1, &chunks);
}

int sea_hw64_enhance(const float *x, long L, float *out_f32, float *mask, int *pitch, int *status)
{
    if (L < 0) return fail("hw64_enhance: L=%ld", L);
    if (!status || (L > 0 && (!x || !out_f32))) return fail("hw64_enhance: null pointer");
    if (L == 0) { /* no sample: nothing to compute */
        *status = 0;
        return 0;
    }
    int chunks = 0;
    return enhance_list(&x, &L, 1, &out_f32, nullptr, mask ? &mask : nullptr, pitch ? &pitch : nullptr, status, &chunks);
}
