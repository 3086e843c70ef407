/*
 * dnn_capi.hip -- the C ABI of the DNN mask estimator (include/sea_mi355x.h): the model object, the
 * cochleagram and the network from host memory, and the chain noisy audio -> subbands -> cochleagram -> network ->
 * resynthesis, which stays on the device on one stream.  Host pointers only; the launches on device pointers are internal
 * (sea_capi::cochleagram64_launch, sea_capi::dnn_forward_launch).
 */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "dnn_kernels.h"

using namespace sea_capi;

namespace sea_capi {

int cochleagram64_launch(const short *d_sub64, const long long *d_offsets, const long long *d_lengths,
                         const long long *d_row_offsets, float *d_feats, int n_utt, hipStream_t stream)
{
    if (n_utt <= 0) return 0;
    if (n_utt > (1 << 25)) return fail("cochleagram: %d utterances in one launch", n_utt);
    sea::CochleagramArgs a;
    a.sub = d_sub64;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.feats = d_feats;
    a.n_utt = n_utt;
    hipLaunchKernelGGL(sea::cochleagram64_kernel, dim3((unsigned)n_utt * 64u), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dnn_forward_launch(const sea_dnn *m, const float *d_feats, const long long *d_row_offsets, int n_utt, long long rows,
                       float *d_act0, float *d_act1, float *d_out, hipStream_t stream, const hipEvent_t *marks)
{
    if (rows <= 0 || n_utt <= 0) return 0;
    if (rows > 0x7fffffffLL) return fail("dnn: %lld rows in one launch", rows);
    sea::DnnSpliceArgs s;
    s.feats = d_feats;
    s.row_offsets = d_row_offsets;
    s.shift = m->d_shift;
    s.scale = m->d_scale;
    s.x0 = d_act0;
    s.ldx = m->ld;
    s.context = m->context;
    s.n_utt = n_utt;
    hipLaunchKernelGGL(sea::dnn_splice_kernel, dim3((unsigned)rows), dim3(256), 0, stream, s);
    HIP_TRY(hipGetLastError());
    if (marks) HIP_TRY(hipEventRecord(marks[0], stream));
    float *buf[2] = {d_act0, d_act1};
    for (int l = 0; l < m->n_layers; ++l) {
        const bool last = l == m->n_layers - 1;
        sea::DnnLayerArgs a;
        a.x = buf[l & 1];
        a.w = m->d_w[l];
        a.b = m->d_b[l];
        a.y = last ? d_out : buf[(l + 1) & 1];
        a.M = rows;
        a.K = m->dims[l];
        a.N = m->dims[l + 1];
        a.Kp = (a.K + sea::kDnnTileK - 1) / sea::kDnnTileK * sea::kDnnTileK;
        a.ldx = m->ld;
        a.ldy = last ? a.N : m->ld;
        a.act = m->act[l];
        const dim3 grid((unsigned)((rows + sea::kDnnTileM - 1) / sea::kDnnTileM), (unsigned)((a.N + sea::kDnnTileN - 1) / sea::kDnnTileN));
        hipLaunchKernelGGL(sea::dnn_layer_kernel, grid, dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        if (marks) HIP_TRY(hipEventRecord(marks[1 + l], stream));
    }
    return 0;
}

} // namespace sea_capi

namespace {

thread_local int t_last_chunks = 0;

/* the device time of the stages of this thread's last sea_dnn_enhance_utterances, summed over its chunks, between events on
 * its stream: SEA_DNN_STAGE_* of the header */
constexpr int kStages = SEA_DNN_STAGE_COUNT;
thread_local double t_stage_ms[kStages] = {};

long long rows_of(long L) { return (L - 320) / 160 + 1; }

enum { S, R }; /* of an utterance of audio: padded samples, rows, bytes */

int on_models_device(const sea_dnn *m, const char *who)
{
    if (!m) return fail("%s: the model is NULL", who);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != m->device) return fail("%s: the model's weights are on device %d, the current device is %d", who, m->device, dev);
    return 0;
}

bool all_finite(const float *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

template <typename T>
int upload(T **d, const T *h, size_t n)
{
    HIP_TRY(hipMalloc(d, n * sizeof(T)));
    HIP_TRY(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int dnn_fill(sea_dnn *m, const float *shift, const float *scale, const float *const *W, const float *const *b)
{
    HIP_TRY(hipGetDevice(&m->device));
    const size_t K0 = (size_t)m->dims[0];
    if (upload(&m->d_shift, shift, K0) || upload(&m->d_scale, scale, K0)) return 1;
    std::vector<float> wp;
    for (int l = 0; l < m->n_layers; ++l) {
        const size_t K = (size_t)m->dims[l], N = (size_t)m->dims[l + 1];
        const size_t Kp = (K + sea::kDnnTileK - 1) / sea::kDnnTileK * sea::kDnnTileK;
        const size_t Np = (N + sea::kDnnTileN - 1) / sea::kDnnTileN * sea::kDnnTileN;
        wp.assign(Np * Kp, 0.0f); /* the K padding and the rows beyond N are zeros: fma (0, 0, acc) is acc */
        for (size_t j = 0; j < N; ++j) memcpy(&wp[j * Kp], W[l] + j * K, K * sizeof(float));
        if (upload(&m->d_w[l], wp.data(), wp.size()) || upload(&m->d_b[l], b[l], N)) return 1;
    }
    return 0;
}

} // namespace

extern "C" {

sea_dnn *sea_dnn_create(int context, const float *shift, const float *scale, int n_layers, const int *dims, const float *const *W,
                        const float *const *b, const int *act)
{
    if (context < 0 || context > 15) return fail("dnn_create: context %d (0..15)", context), nullptr;
    if (n_layers < 1 || n_layers > 8) return fail("dnn_create: %d layers (1..8)", n_layers), nullptr;
    if (!shift || !scale || !dims || !W || !b || !act) return fail("dnn_create: a required argument is NULL"), nullptr;
    const int K0 = 64 * (2 * context + 1);
    if (dims[0] != K0) return fail("dnn_create: dims[0] = %d, the input of context %d has %d values", dims[0], context, K0), nullptr;
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1 || dims[l] > 4096) return fail("dnn_create: dims[%d] = %d (1..4096)", l, dims[l]), nullptr;
    if (!all_finite(shift, (size_t)K0) || !all_finite(scale, (size_t)K0))
        return fail("dnn_create: shift or scale holds a value that is not finite"), nullptr;
    for (int l = 0; l < n_layers; ++l) {
        if (act[l] < 0 || act[l] > 2) return fail("dnn_create: act[%d] = %d (0 identity, 1 sigmoid, 2 ReLU)", l, act[l]), nullptr;
        if (!W[l] || !b[l]) return fail("dnn_create: layer %d has a NULL array", l), nullptr;
        if (!all_finite(W[l], (size_t)dims[l] * dims[l + 1]) || !all_finite(b[l], (size_t)dims[l + 1]))
            return fail("dnn_create: layer %d holds a weight or bias that is not finite", l), nullptr;
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return nullptr;
    sea_dnn *m = new sea_dnn;
    m->context = context;
    m->n_layers = n_layers;
    int max_dim = 0;
    for (int l = 0; l <= n_layers; ++l) m->dims[l] = dims[l], max_dim = std::max(max_dim, dims[l]);
    for (int l = 0; l < n_layers; ++l) m->act[l] = act[l];
    m->ld = (max_dim + 3) & ~3;
    if (dnn_fill(m, shift, scale, W, b)) {
        sea_dnn_destroy(m);
        return nullptr;
    }
    return m;
}

void sea_dnn_destroy(sea_dnn *m)
{
    if (!m) return;
    (void)hipFree(m->d_shift);
    (void)hipFree(m->d_scale);
    for (int l = 0; l < 8; ++l) (void)hipFree(m->d_w[l]), (void)hipFree(m->d_b[l]);
    delete m;
}

int sea_dnn_last_chunks(void) { return t_last_chunks; }

double sea_dnn_last_stage_ms(int stage) { return stage >= 0 && stage < kStages ? t_stage_ms[stage] : -1.0; }

int sea_cochleagram64(const short *sub64, long L, float *feats)
{
    if (!sub64 || !feats) return fail("cochleagram64: a required argument is NULL");
    if (L < 320) return fail("cochleagram64: L=%ld is shorter than one 320-sample frame", L);
    const long long Lp = align8(L), F = rows_of(L);
    DevBuf<short> ds;
    DevBuf<float> df;
    DevBuf<long long> dmeta;
    HIP_TRY(ds.alloc((size_t)Lp * 64));
    HIP_TRY(df.alloc((size_t)F * 64));
    HIP_TRY(dmeta.alloc(3));
    const long long meta[3] = {0, L, 0};
    /* the padding of a channel row is no part of any frame: SEA_DNN_PAD_FILL puts a value of the caller's there so that a test
     * can show it (tests/test_gpu_dnn.py) */
    const char *fill = getenv("SEA_DNN_PAD_FILL");
    std::vector<short> staged((size_t)Lp * 64, (short)(fill ? atoi(fill) : 0));
    for (int c = 0; c < 64; ++c) memcpy(&staged[(size_t)c * Lp], sub64 + (size_t)c * L, (size_t)L * sizeof(short));
    HIP_TRY(hipMemcpy(ds.p, staged.data(), staged.size() * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmeta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    if (cochleagram64_launch(ds.p, dmeta.p, dmeta.p + 1, dmeta.p + 2, df.p, 1, nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(feats, df.p, (size_t)F * 64 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

/* Device footprint of a chunk: per padded sample 2 B of audio and 128 B of subbands, per row 256 B of features */
int sea_cochleagram_utterances(const short *const *in, const long *lengths, int n_utt, float *const *feats)
{
    t_last_chunks = 0;
    if (n_utt <= 0) return 0;
    if (!in || !lengths || !feats) return fail("cochleagram: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 320)
            return fail("cochleagram: utterance %d has %ld samples (shorter than one 320-sample frame)", u, lengths[u]);
        if (!in[u] || !feats[u]) return fail("cochleagram: utterance %d has a NULL buffer", u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    long long budget;
    if (scratch_budget("SEA_DNN_SCRATCH_MB", &budget)) return 1;
    auto of = [&](int u) -> Totals<3> {
        const long long s = align8(lengths[u]), r = rows_of(lengths[u]);
        return {s, r, s * 130 + r * 256 + 64};
    };
    const ChunkPlan<3> plan = plan_chunks<3>(n_utt, budget, of);
    Staged<short> b_in;
    DevBuf<short> d_sub;
    Staged<float> b_feats;
    Staged<long long> b_meta; /* offsets, lengths, row offsets */
    Staged<int> b_order;
    HIP_TRY(b_in.alloc((size_t)plan.max[S]));
    HIP_TRY(d_sub.alloc((size_t)plan.max[S] * 64));
    HIP_TRY(b_feats.alloc((size_t)plan.max[R] * 64));
    HIP_TRY(b_meta.alloc(3 * (size_t)plan.max_n));
    HIP_TRY(b_order.alloc((size_t)plan.max_n));
    const long long *d_meta = b_meta.d.p;
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *offs = b_meta.h.data(), *lens = offs + n, *roff = lens + n;
        long long s = 0, r = 0;
        for (int j = 0; j < n; ++j) {
            offs[j] = s, lens[j] = lengths[u0 + j], roff[j] = r;
            s += pack_padded(b_in.h.data() + s, in[u0 + j], lens[j]);
            r += rows_of(lengths[u0 + j]);
        }
        launch_order(lens, n, dc->n_cu, b_order.h.data());
        HIP_TRY(hipMemcpy(b_in.d.p, b_in.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_meta.d.p, b_meta.h.data(), 3 * (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b_order.d.p, b_order.h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        if (sea_subband64_batch(b_in.d.p, d_sub.p, d_meta, d_meta + n, b_order.d.p, n, nullptr)) return 1;
        if (cochleagram64_launch(d_sub.p, d_meta, d_meta + n, d_meta + 2 * n, b_feats.d.p, n, nullptr)) return 1;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(b_feats.h.data(), b_feats.d.p, (size_t)r * 64 * sizeof(float), hipMemcpyDeviceToHost));
        for (int j = 0; j < n; ++j)
            memcpy(feats[u0 + j], b_feats.h.data() + roff[j] * 64, (size_t)rows_of((long)lens[j]) * 64 * sizeof(float));
        t_last_chunks = k + 1;
    }
    return 0;
}

/* Device footprint of a chunk: per row 256 B of features, the output row and two activation rows */
int sea_dnn_forward(const sea_dnn *m, const float *const *feats, const int *n_rows, int n_utt, float *const *out)
{
    t_last_chunks = 0;
    if (on_models_device(m, "dnn_forward")) return 1;
    if (n_utt <= 0) return 0;
    if (!feats || !n_rows || !out) return fail("dnn_forward: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (n_rows[u] < 0) return fail("dnn_forward: utterance %d has %d rows", u, n_rows[u]);
        if (n_rows[u] > 0 && (!feats[u] || !out[u])) return fail("dnn_forward: utterance %d has a NULL buffer", u);
    }
    const int n_out = m->dims[m->n_layers];
    long long budget;
    if (scratch_budget("SEA_DNN_SCRATCH_MB", &budget)) return 1;
    const long long row_bytes = 256 + 4LL * n_out + 8LL * m->ld;
    const ChunkPlan<2> plan =
        plan_chunks<2>(n_utt, budget, [&](int u) -> Totals<2> { return {n_rows[u], n_rows[u] * row_bytes + 8}; }); /* rows, bytes */
    const size_t max_r = (size_t)plan.max[0];
    if (max_r == 0) return 0;
    Staged<float> b_feats, b_out;
    DevBuf<float> d_act[2];
    Staged<long long> b_roff;
    HIP_TRY(b_feats.alloc(max_r * 64));
    HIP_TRY(d_act[0].alloc(max_r * m->ld));
    HIP_TRY(d_act[1].alloc(max_r * m->ld));
    HIP_TRY(b_out.alloc(max_r * n_out));
    HIP_TRY(b_roff.alloc((size_t)plan.max_n + 1));
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long r = 0;
        for (int j = 0; j < n; ++j) {
            b_roff.h[j] = r;
            if (n_rows[u0 + j]) memcpy(b_feats.h.data() + r * 64, feats[u0 + j], (size_t)n_rows[u0 + j] * 64 * sizeof(float));
            r += n_rows[u0 + j];
        }
        b_roff.h[n] = r;
        if (r > 0) {
            HIP_TRY(hipMemcpy(b_feats.d.p, b_feats.h.data(), (size_t)r * 64 * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(b_roff.d.p, b_roff.h.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice));
            if (dnn_forward_launch(m, b_feats.d.p, b_roff.d.p, n, r, d_act[0].p, d_act[1].p, b_out.d.p, nullptr)) return 1;
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(b_out.h.data(), b_out.d.p, (size_t)r * n_out * sizeof(float), hipMemcpyDeviceToHost));
            for (int j = 0; j < n; ++j)
                if (n_rows[u0 + j])
                    memcpy(out[u0 + j], b_out.h.data() + b_roff.h[j] * n_out, (size_t)n_rows[u0 + j] * n_out * sizeof(float));
        }
        t_last_chunks = k + 1;
    }
    return 0;
}

/* Device footprint of a chunk: per padded sample 4 B of audio (in and out), 128 B of subbands and the resynthesis scratch
 * (256 B, plus eight time steps per utterance); per row 256 B of features, 256 B of mask and two activation rows.  The
 * network's output is the resynthesis kernel's d_mask: nothing but the audio (and the mask, on request) leaves the device. */
int sea_dnn_enhance_utterances(const sea_dnn *m, const short *const *in, const long *lengths, int n_utt, int binary,
                               short *const *out, float *const *masks)
{
    t_last_chunks = 0;
    if (!m) return fail("dnn_enhance: the model is NULL");
    if (m->dims[m->n_layers] != 64) return fail("dnn_enhance: the network has %d outputs, a mask row has 64", m->dims[m->n_layers]);
    if (binary & ~1)
        return fail("dnn_enhance: binary = %d (bit 1 selects L / 160 mask rows; the cochleagram has (L - 320) / 160 + 1)", binary);
    if (n_utt <= 0) return 0;
    if (!in || !lengths || !out) return fail("dnn_enhance: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 320)
            return fail("dnn_enhance: utterance %d has %ld samples (shorter than one 320-sample frame)", u, lengths[u]);
        if (!in[u] || !out[u]) return fail("dnn_enhance: utterance %d has a NULL buffer", u);
    }
    if (on_models_device(m, "dnn_enhance")) return 1;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    long long budget;
    if (scratch_budget("SEA_DNN_SCRATCH_MB", &budget)) return 1;
    const long long row_bytes = 512 + 8LL * m->ld;
    auto of = [&](int u) -> Totals<3> {
        const long long s = align8(lengths[u]), r = rows_of(lengths[u]);
        return {s, r, s * 132 + sea_resynth_scratch_bytes(s, 1) + r * row_bytes + 64};
    };
    const ChunkPlan<3> plan = plan_chunks<3>(n_utt, budget, of);
    const size_t max_s = (size_t)plan.max[S], max_r = (size_t)plan.max[R], max_n = (size_t)plan.max_n;
    Staged<short> b_audio; /* in on the way up, out on the way down */
    DevBuf<short> d_out, d_sub;
    DevBuf<float> d_feats, d_act[2], d_inter;
    Staged<float> b_mask;
    Staged<long long> b_meta; /* offsets, lengths, row offsets [n + 1] */
    Staged<int> b_order;
    HIP_TRY(b_audio.alloc(max_s));
    HIP_TRY(d_out.alloc(max_s));
    HIP_TRY(d_sub.alloc(max_s * 64));
    HIP_TRY(d_inter.alloc((size_t)sea_resynth_scratch_bytes(plan.max[S], plan.max_n) / sizeof(float)));
    HIP_TRY(d_feats.alloc(max_r * 64));
    HIP_TRY(b_mask.alloc(max_r * 64, masks != nullptr));
    HIP_TRY(d_act[0].alloc(max_r * m->ld));
    HIP_TRY(d_act[1].alloc(max_r * m->ld));
    HIP_TRY(b_meta.alloc(3 * max_n + 1));
    HIP_TRY(b_order.alloc(max_n));
    short *d_in = b_audio.d.p;
    float *d_mask = b_mask.d.p;
    hipStream_t stream = nullptr;
    EventSet<kStages + 1> ev; /* e[0] before the subbands, e[1 + s] after stage s */
    if (ev.create()) return 1;
    for (double &t : t_stage_ms) t = 0.0;
    const int nl = m->n_layers;
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *offs = b_meta.h.data(), *lens = offs + n, *roff = lens + n;
        long long s = 0, r = 0;
        for (int j = 0; j < n; ++j) {
            offs[j] = s, lens[j] = lengths[u0 + j], roff[j] = r;
            s += pack_padded(b_audio.h.data() + s, in[u0 + j], lens[j]);
            r += rows_of(lengths[u0 + j]);
        }
        roff[n] = r;
        launch_order(lens, n, dc->n_cu, b_order.h.data());
        HIP_TRY(hipMemcpyAsync(d_in, b_audio.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(b_meta.d.p, b_meta.h.data(), (3 * (size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(b_order.d.p, b_order.h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
        const long long *d_offs = b_meta.d.p, *d_lens = d_offs + n, *d_roff = d_offs + 2 * n;
        HIP_TRY(hipEventRecord(ev.e[0], stream));
        if (sea_subband64_batch(d_in, d_sub.p, d_offs, d_lens, b_order.d.p, n, stream)) return 1;
        HIP_TRY(hipEventRecord(ev.e[1 + SEA_DNN_STAGE_SUBBAND], stream));
        if (cochleagram64_launch(d_sub.p, d_offs, d_lens, d_roff, d_feats.p, n, stream)) return 1;
        HIP_TRY(hipEventRecord(ev.e[1 + SEA_DNN_STAGE_COCHLEAGRAM], stream));
        if (dnn_forward_launch(m, d_feats.p, d_roff, n, r, d_act[0].p, d_act[1].p, d_mask, stream, &ev.e[1 + SEA_DNN_STAGE_SPLICE]))
            return 1;
        if (sea_resynth64_batch(d_in, d_out.p, d_offs, d_lens, d_mask, d_roff, d_inter.p, b_order.d.p, n, binary, stream)) return 1;
        HIP_TRY(hipEventRecord(ev.e[1 + SEA_DNN_STAGE_RESYNTH], stream));
        HIP_TRY(hipMemcpyAsync(b_audio.h.data(), d_out.p, (size_t)s * sizeof(short), hipMemcpyDeviceToHost, stream));
        if (masks) HIP_TRY(hipMemcpyAsync(b_mask.h.data(), d_mask, (size_t)r * 64 * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        {   /* stage s lasts from the event before it to its own; the stages 3 + n_layers .. 10 do not exist */
            int before = 0;
            for (int st = 0; st <= SEA_DNN_STAGE_RESYNTH; ++st) {
                if (st >= SEA_DNN_STAGE_LAYER0 + nl && st < SEA_DNN_STAGE_RESYNTH) continue;
                if (ev.add_ms(before, 1 + st, &t_stage_ms[st])) return 1;
                before = 1 + st;
            }
            if (ev.add_ms(0, 1 + SEA_DNN_STAGE_RESYNTH, &t_stage_ms[SEA_DNN_STAGE_ALL])) return 1;
        }
        for (int j = 0; j < n; ++j) {
            memcpy(out[u0 + j], b_audio.h.data() + offs[j], (size_t)lens[j] * sizeof(short));
            if (masks && masks[u0 + j])
                memcpy(masks[u0 + j], b_mask.h.data() + roff[j] * 64, (size_t)(roff[j + 1] - roff[j]) * 64 * sizeof(float));
        }
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
