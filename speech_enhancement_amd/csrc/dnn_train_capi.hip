/*
 * dnn_train_capi.hip -- the C ABI of the DNN mask estimator's trainer (include/sea_mi355x.h): the
 * training set resident on the device, minibatch SGD steps back to back on one internal stream, in place in the sea_dnn's
 * weights.  Host pointers only.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "dnn_train_kernels.h"

using namespace sea_capi;

struct sea_dnn_trainer {
    sea_dnn *m = nullptr;
    int n_utt = 0, max_batch = 0, last_batch = 0;
    long long rows = 0;
    hipStream_t stream = nullptr;
    float *d_feats = nullptr, *d_targets = nullptr;
    long long *d_roff = nullptr;
    float *d_a[9] = {};     /* a_0 .. a_n, [max_batch][m->ld] */
    float *d_delta[9] = {}; /* delta_1 .. delta_n at [1] .. [n], [max_batch][m->ld] */
    float *d_G[8] = {}, *d_g[8] = {}, *d_vw[8] = {}, *d_vb[8] = {};
    float *d_r = nullptr;
    long long *d_order = nullptr;
    double *d_losses = nullptr;
    long long cap_order = 0, cap_losses = 0;
    hipEvent_t ev[SEA_DNN_TRAIN_STAGE_COUNT + 1] = {};
    double stage_ms[SEA_DNN_TRAIN_STAGE_COUNT] = {};
};

namespace {

int on_device(const sea_dnn *m, const char *who)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != m->device) return fail("%s: the model's weights are on device %d, the current device is %d", who, m->device, dev);
    return 0;
}

int kp_of(int K) { return (K + sea::kDnnTileK - 1) / sea::kDnnTileK * sea::kDnnTileK; }

template <typename T>
int dev_alloc(T **p, size_t n, bool zero = false)
{
    HIP_TRY(hipMalloc(p, std::max<size_t>(n, 1) * sizeof(T) + 16));
    if (zero) HIP_TRY(hipMemset(*p, 0, std::max<size_t>(n, 1) * sizeof(T)));
    return 0;
}

int trainer_fill(sea_dnn_trainer *t, const float *const *feats, const float *const *targets, const int *n_rows)
{
    const sea_dnn *m = t->m;
    const int n = m->n_layers, n_out = m->dims[n];
    const size_t mb = (size_t)t->max_batch, ld = (size_t)m->ld;
    size_t bytes = (size_t)t->rows * (64 + (size_t)n_out) * 4 + ((size_t)t->n_utt + 1) * 8 + (2 * (size_t)n + 1) * mb * ld * 4;
    for (int l = 0; l < n; ++l) bytes += 2 * ((size_t)m->dims[l] + 1) * (size_t)m->dims[l + 1] * 4;
    long long limit;
    if (scratch_budget(nullptr, &limit)) return 1;
    if (bytes > (size_t)limit)
        return fail("dnn_trainer_create: the training set and the step's buffers take %zu bytes, 60 %% of the free device memory is "
                    "%zu (a set larger than the device is out of scope)", bytes, (size_t)limit);
    HIP_TRY(hipStreamCreate(&t->stream));
    for (hipEvent_t &e : t->ev) HIP_TRY(hipEventCreate(&e));
    if (dev_alloc(&t->d_feats, (size_t)t->rows * 64) || dev_alloc(&t->d_targets, (size_t)t->rows * n_out) ||
        dev_alloc(&t->d_roff, (size_t)t->n_utt + 1) || dev_alloc(&t->d_r, mb))
        return 1;
    std::vector<long long> roff((size_t)t->n_utt + 1);
    long long r = 0;
    for (int u = 0; u < t->n_utt; ++u) {
        roff[u] = r;
        if (n_rows[u]) {
            HIP_TRY(hipMemcpy(t->d_feats + r * 64, feats[u], (size_t)n_rows[u] * 64 * sizeof(float), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t->d_targets + r * n_out, targets[u], (size_t)n_rows[u] * n_out * sizeof(float), hipMemcpyHostToDevice));
        }
        r += n_rows[u];
    }
    roff[t->n_utt] = r;
    HIP_TRY(hipMemcpy(t->d_roff, roff.data(), roff.size() * sizeof(long long), hipMemcpyHostToDevice));
    for (int l = 0; l <= n; ++l) {
        if (dev_alloc(&t->d_a[l], mb * ld, true)) return 1;
        if (l > 0 && dev_alloc(&t->d_delta[l], mb * ld, true)) return 1;
    }
    for (int l = 0; l < n; ++l) {
        const size_t K = (size_t)m->dims[l], N = (size_t)m->dims[l + 1];
        if (dev_alloc(&t->d_G[l], N * K, true) || dev_alloc(&t->d_g[l], N, true) || dev_alloc(&t->d_vw[l], N * K, true) ||
            dev_alloc(&t->d_vb[l], N, true))
            return 1;
    }
    return 0;
}

/* one step on the minibatch idx[0 .. B - 1]; marks: record the stage events (the run's last step) */
int trainer_step(sea_dnn_trainer *t, const long long *d_idx, int B, float eta, float mu, int update, double *d_loss, bool marks)
{
    const sea_dnn *m = t->m;
    const int n = m->n_layers, ld = m->ld;
    hipStream_t s = t->stream;
    auto mark = [&](int stage) -> int {
        if (marks) HIP_TRY(hipEventRecord(t->ev[1 + stage], s));
        return 0;
    };
    if (marks) HIP_TRY(hipEventRecord(t->ev[0], s));
    sea::DnnGatherArgs ga;
    ga.feats = t->d_feats, ga.row_offsets = t->d_roff, ga.idx = d_idx, ga.shift = m->d_shift, ga.scale = m->d_scale;
    ga.x0 = t->d_a[0], ga.ldx = ld, ga.context = m->context, ga.n_utt = t->n_utt;
    hipLaunchKernelGGL(sea::dnn_gather_splice_kernel, dim3((unsigned)B), dim3(256), 0, s, ga);
    HIP_TRY(hipGetLastError());
    if (mark(SEA_DNN_TRAIN_STAGE_GATHER)) return 1;
    for (int l = 0; l < n; ++l) { /* the inference contract: dnn_layer_kernel as it is */
        sea::DnnLayerArgs a;
        a.x = t->d_a[l], a.w = m->d_w[l], a.b = m->d_b[l], a.y = t->d_a[l + 1];
        a.M = B, a.K = m->dims[l], a.N = m->dims[l + 1], a.Kp = kp_of(a.K), a.ldx = ld, a.ldy = ld, a.act = m->act[l];
        const dim3 grid((unsigned)((B + sea::kDnnTileM - 1) / sea::kDnnTileM), (unsigned)((a.N + sea::kDnnTileN - 1) / sea::kDnnTileN));
        hipLaunchKernelGGL(sea::dnn_layer_kernel, grid, dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        if (mark(SEA_DNN_TRAIN_STAGE_FORWARD0 + l)) return 1;
    }
    sea::DnnDeltaOutArgs da;
    da.y = t->d_a[n], da.targets = t->d_targets, da.idx = d_idx, da.delta = update ? t->d_delta[n] : nullptr, da.r = t->d_r;
    da.B = B, da.N = m->dims[n], da.ldy = ld, da.ldd = ld, da.act = m->act[n - 1];
    hipLaunchKernelGGL(sea::dnn_delta_out_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, da);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sea::dnn_loss_kernel, dim3(1), dim3(64), 0, s, t->d_r, B, d_loss);
    HIP_TRY(hipGetLastError());
    if (mark(SEA_DNN_TRAIN_STAGE_DELTA)) return 1;
    if (!update) return 0;
    const int T = sea::kDnnTrainTile;
    for (int l = n; l >= 1; --l) { /* layer l: dims[l - 1] -> dims[l], weights m->d_w[l - 1] as they were before this step */
        const int K = m->dims[l - 1], N = m->dims[l];
        sea::DnnWgradArgs wa;
        wa.delta = t->d_delta[l], wa.a_prev = t->d_a[l - 1], wa.G = t->d_G[l - 1], wa.g = t->d_g[l - 1];
        wa.M = B, wa.N = N, wa.K = K, wa.ldd = ld, wa.lda = ld;
        hipLaunchKernelGGL(sea::dnn_wgrad_kernel, dim3((unsigned)((N + T - 1) / T), (unsigned)((K + 1 + T - 1) / T)), dim3(256), 0, s, wa);
        HIP_TRY(hipGetLastError());
        if (mark(SEA_DNN_TRAIN_STAGE_WGRAD0 + l - 1)) return 1;
        if (l > 1) { /* nothing is propagated into x0 */
            sea::DnnDgradArgs ea;
            ea.delta = t->d_delta[l], ea.w = m->d_w[l - 1], ea.a_prev = t->d_a[l - 1], ea.out = t->d_delta[l - 1];
            ea.M = B, ea.N = N, ea.K = K, ea.Kp = kp_of(K), ea.ldd = ld, ea.lda = ld, ea.ldo = ld, ea.act = m->act[l - 2];
            hipLaunchKernelGGL(sea::dnn_dgrad_kernel, dim3((unsigned)((B + T - 1) / T), (unsigned)((K + T - 1) / T)), dim3(256), 0, s, ea);
            HIP_TRY(hipGetLastError());
            if (mark(SEA_DNN_TRAIN_STAGE_DGRAD0 + l - 1)) return 1;
        }
    }
    for (int l = 0; l < n; ++l) {
        sea::DnnSgdArgs sa;
        sa.w = m->d_w[l], sa.b = m->d_b[l], sa.G = t->d_G[l], sa.g = t->d_g[l], sa.vw = t->d_vw[l], sa.vb = t->d_vb[l];
        sa.N = m->dims[l + 1], sa.K = m->dims[l], sa.Kp = kp_of(sa.K), sa.eta = eta, sa.mu = mu;
        const long long total = (long long)sa.N * sa.K + sa.N;
        hipLaunchKernelGGL(sea::dnn_sgd_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0, s, sa);
        HIP_TRY(hipGetLastError());
    }
    return mark(SEA_DNN_TRAIN_STAGE_UPDATE);
}

} // namespace

extern "C" {

sea_dnn_trainer *sea_dnn_trainer_create(sea_dnn *m, const float *const *feats, const float *const *targets, const int *n_rows,
                                        int n_utt, int max_batch)
{
    if (!m || !feats || !targets || !n_rows) return fail("dnn_trainer_create: a required argument is NULL"), nullptr;
    if (max_batch < 1 || max_batch > 4096) return fail("dnn_trainer_create: max_batch = %d (1..4096)", max_batch), nullptr;
    if (n_utt < 1) return fail("dnn_trainer_create: %d utterances", n_utt), nullptr;
    long long rows = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (n_rows[u] < 0) return fail("dnn_trainer_create: utterance %d has %d rows", u, n_rows[u]), nullptr;
        if (n_rows[u] > 0 && (!feats[u] || !targets[u])) return fail("dnn_trainer_create: utterance %d has a NULL array", u), nullptr;
        rows += n_rows[u];
    }
    if (rows < 1) return fail("dnn_trainer_create: the training set has no row"), nullptr;
    if (on_device(m, "dnn_trainer_create")) return nullptr;
    sea_dnn_trainer *t = new sea_dnn_trainer;
    t->m = m, t->n_utt = n_utt, t->max_batch = max_batch, t->rows = rows;
    if (trainer_fill(t, feats, targets, n_rows)) {
        sea_dnn_trainer_destroy(t);
        return nullptr;
    }
    return t;
}

void sea_dnn_trainer_destroy(sea_dnn_trainer *t)
{
    if (!t) return;
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    (void)hipFree(t->d_feats), (void)hipFree(t->d_targets), (void)hipFree(t->d_roff), (void)hipFree(t->d_r);
    (void)hipFree(t->d_order), (void)hipFree(t->d_losses);
    for (int l = 0; l < 9; ++l) (void)hipFree(t->d_a[l]), (void)hipFree(t->d_delta[l]);
    for (int l = 0; l < 8; ++l) (void)hipFree(t->d_G[l]), (void)hipFree(t->d_g[l]), (void)hipFree(t->d_vw[l]), (void)hipFree(t->d_vb[l]);
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int sea_dnn_trainer_run(sea_dnn_trainer *t, const long long *order, long long n_order, int batch, float eta, float mu, int update,
                        double *losses)
{
    /* what the arguments alone decide comes first, then what needs the trainer; the device comes after both */
    if (!t || !order || !losses) return fail("dnn_trainer_run: a required argument is NULL");
    if (batch < 1 || batch > 4096) return fail("dnn_trainer_run: batch = %d (1..4096)", batch);
    if (n_order < 1) return fail("dnn_trainer_run: n_order = %lld", n_order);
    if (!std::isfinite(eta)) return fail("dnn_trainer_run: eta is not finite");
    if (!std::isfinite(mu) || mu < 0.0f || mu >= 1.0f) return fail("dnn_trainer_run: mu = %g (0 <= mu < 1)", (double)mu);
    if (batch > t->max_batch) return fail("dnn_trainer_run: batch = %d, the trainer was created for at most %d", batch, t->max_batch);
    for (long long i = 0; i < n_order; ++i)
        if (order[i] < 0 || order[i] >= t->rows)
            return fail("dnn_trainer_run: order[%lld] = %lld, the training set has %lld rows", i, order[i], t->rows);
    if (on_device(t->m, "dnn_trainer_run")) return 1;
    const long long steps = (n_order + batch - 1) / batch;
    if (n_order > t->cap_order) {
        (void)hipFree(t->d_order), t->d_order = nullptr, t->cap_order = 0;
        if (dev_alloc(&t->d_order, (size_t)n_order)) return 1;
        t->cap_order = n_order;
    }
    if (steps > t->cap_losses) {
        (void)hipFree(t->d_losses), t->d_losses = nullptr, t->cap_losses = 0;
        if (dev_alloc(&t->d_losses, (size_t)steps)) return 1;
        t->cap_losses = steps;
    }
    HIP_TRY(hipMemcpyAsync(t->d_order, order, (size_t)n_order * sizeof(long long), hipMemcpyHostToDevice, t->stream));
    for (long long st = 0; st < steps; ++st) { /* back to back: nothing waits on the host between steps */
        const int B = (int)std::min<long long>(batch, n_order - st * batch);
        if (trainer_step(t, t->d_order + st * batch, B, eta, mu, update, t->d_losses + st, st == steps - 1)) return 1;
        t->last_batch = B;
    }
    HIP_TRY(hipMemcpyAsync(losses, t->d_losses, (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    for (double &v : t->stage_ms) v = 0.0;
    {   /* the last step's stages: each from the event recorded before it to its own */
        const int n = t->m->n_layers;
        int before = 0;
        auto take = [&](int stage) -> int {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, t->ev[before], t->ev[1 + stage]));
            t->stage_ms[stage] = ms;
            before = 1 + stage;
            return 0;
        };
        if (take(SEA_DNN_TRAIN_STAGE_GATHER)) return 1;
        for (int l = 0; l < n; ++l)
            if (take(SEA_DNN_TRAIN_STAGE_FORWARD0 + l)) return 1;
        if (take(SEA_DNN_TRAIN_STAGE_DELTA)) return 1;
        if (update) {
            for (int l = n; l >= 1; --l) {
                if (take(SEA_DNN_TRAIN_STAGE_WGRAD0 + l - 1)) return 1;
                if (l > 1 && take(SEA_DNN_TRAIN_STAGE_DGRAD0 + l - 1)) return 1;
            }
            if (take(SEA_DNN_TRAIN_STAGE_UPDATE)) return 1;
        }
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, t->ev[0], t->ev[before]));
        t->stage_ms[SEA_DNN_TRAIN_STAGE_ALL] = ms;
    }
    for (long long st = 0; st < steps; ++st)
        if (!std::isfinite(losses[st])) {
            fail("dnn_trainer_run: the loss of step %lld is not finite", st);
            return 2;
        }
    return 0;
}

double sea_dnn_trainer_stage_ms(const sea_dnn_trainer *t, int stage)
{
    return t && stage >= 0 && stage < SEA_DNN_TRAIN_STAGE_COUNT ? t->stage_ms[stage] : -1.0;
}

int sea_dnn_trainer_read(const sea_dnn_trainer *t, int what, int layer, float *out)
{
    if (!t || !out) return fail("dnn_trainer_read: a required argument is NULL");
    const sea_dnn *m = t->m;
    const int n = m->n_layers;
    if (what < SEA_DNN_TRAIN_ACT || what > SEA_DNN_TRAIN_BMOM) return fail("dnn_trainer_read: what = %d", what);
    const int first = what == SEA_DNN_TRAIN_ACT ? 0 : 1;
    if (layer < first || layer > n) return fail("dnn_trainer_read: layer %d of what = %d (%d..%d)", layer, what, first, n);
    if (on_device(m, "dnn_trainer_read")) return 1;
    const size_t B = (size_t)t->last_batch, ld = (size_t)m->ld, N = (size_t)m->dims[layer];
    if (what == SEA_DNN_TRAIN_ACT || what == SEA_DNN_TRAIN_DELTA) { /* [last batch][dims[layer]] */
        const float *src = what == SEA_DNN_TRAIN_ACT ? t->d_a[layer] : t->d_delta[layer];
        if (B) HIP_TRY(hipMemcpy2D(out, N * 4, src, ld * 4, N * 4, B, hipMemcpyDeviceToHost));
        return 0;
    }
    const size_t K = (size_t)m->dims[layer - 1];
    const float *src = what == SEA_DNN_TRAIN_WGRAD ? t->d_G[layer - 1] : what == SEA_DNN_TRAIN_BGRAD ? t->d_g[layer - 1]
                     : what == SEA_DNN_TRAIN_WMOM  ? t->d_vw[layer - 1] : t->d_vb[layer - 1];
    const size_t count = what == SEA_DNN_TRAIN_WGRAD || what == SEA_DNN_TRAIN_WMOM ? N * K : N;
    HIP_TRY(hipMemcpy(out, src, count * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_dnn_get_params(const sea_dnn *m, float *const *weights, float *const *biases)
{
    if (!m || !weights || !biases) return fail("dnn_get_params: a required argument is NULL");
    for (int l = 0; l < m->n_layers; ++l)
        if (!weights[l] || !biases[l]) return fail("dnn_get_params: layer %d has a NULL array", l);
    if (on_device(m, "dnn_get_params")) return 1;
    for (int l = 0; l < m->n_layers; ++l) {
        const size_t K = (size_t)m->dims[l], N = (size_t)m->dims[l + 1];
        HIP_TRY(hipMemcpy2D(weights[l], K * 4, m->d_w[l], (size_t)kp_of((int)K) * 4, K * 4, N, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(biases[l], m->d_b[l], N * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

} // extern "C"
