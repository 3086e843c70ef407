/*
 * dnn_train_model_driver.c -- the plain-C model of the DNN mask estimator's trainer: the gather, the
 * forward pass, the loss, the deltas, the two gradient chains, back-propagation and the momentum update, stated literally as
 * loops over individually rounded float operations, with csrc/dnn_math.h -- the header the device code includes.  Built by
 * tests/dnn_train_model.py with gcc -O2 -ffp-contract=off.
 *
 *   train IN OUT [decoy]   the steps of IN -> OUT;  decoy: G summed over m descending and E over j descending
 *
 * IN: int32 context, n_layers, dims[n_layers + 1], act[n_layers], n_utt, n_rows[n_utt], n_order, batch, update; float32 eta, mu,
 * shift[K0], scale[K0], per layer W[out][in] and b[out], per utterance feats[n_rows][64], per utterance
 * targets[n_rows][dims[n]]; int64 order[n_order].  The momentum starts at zero.
 * OUT: float64 losses[steps]; float32 per layer W, b, vW, vb after the steps; then of the last step a_0 .. a_n [B][dims[l]],
 * delta_1 .. delta_n [B][dims[l]], and per layer 1 .. n G_l [dims[l]][dims[l - 1]] and g_l [dims[l]].
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dnn_math.h"

static void die(const char *what)
{
    fprintf(stderr, "dnn_train_model_driver: %s\n", what);
    exit(2);
}

static void *slurp(const char *path, size_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open the input");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    void *p = malloc((size_t)n + 16);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) die("cannot read the input");
    fclose(f);
    *bytes = (size_t)n;
    return p;
}

static float *floats(size_t n)
{
    float *p = (float *)calloc(n ? n : 1, sizeof(float));
    if (!p) die("out of memory");
    return p;
}

/* delta = e d (a): the sigmoid's a (1 - a) is a subtract then a multiply, then one more multiply */
static float delta_of(float e, float a, int act)
{
    if (act == 1) {
        const float one_minus = 1.0f - a;
        const float d = a * one_minus;
        return e * d;
    }
    if (act == 2) return a > 0.0f ? e : 0.0f;
    return e;
}

static int train(const char *in_path, const char *out_path, int decoy)
{
    size_t bytes;
    const char *blob = (const char *)slurp(in_path, &bytes);
    const int32_t *h = (const int32_t *)blob;
    const int C = h[0], n = h[1];
    const int32_t *dims = h + 2, *act = dims + n + 1;
    const int n_utt = act[n];
    const int32_t *n_rows = act + n + 1;
    const int n_order = n_rows[n_utt], batch = n_rows[n_utt + 1], update = n_rows[n_utt + 2];
    const float *p = (const float *)(n_rows + n_utt + 3);
    const float eta = p[0], mu = p[1];
    p += 2;
    const int K0 = 64 * (2 * C + 1), n_out = dims[n];
    if (dims[0] != K0) die("dims[0] != K0");
    const float *shift = p, *scale = p + K0;
    p += 2 * (size_t)K0;
    float *W[9], *b[9], *vW[9], *vb[9], *G[9], *g[9], *a[9], *delta[9]; /* layer l = 1 .. n: dims[l - 1] -> dims[l] */
    for (int l = 1; l <= n; ++l) {
        const size_t K = (size_t)dims[l - 1], N = (size_t)dims[l];
        W[l] = floats(N * K), b[l] = floats(N), vW[l] = floats(N * K), vb[l] = floats(N), G[l] = floats(N * K), g[l] = floats(N);
        memcpy(W[l], p, N * K * sizeof(float));
        p += N * K;
        memcpy(b[l], p, N * sizeof(float));
        p += N;
    }
    long long *roff = (long long *)malloc(((size_t)n_utt + 1) * sizeof(long long));
    long long rows = 0;
    for (int u = 0; u < n_utt; ++u) roff[u] = rows, rows += n_rows[u];
    roff[n_utt] = rows;
    const float *feats = p, *targets = p + rows * 64;
    const char *order_at = (const char *)(targets + rows * n_out);
    if (order_at + (size_t)n_order * 8 != blob + bytes) die("the input's size does not match its header");
    long long *order = (long long *)malloc((size_t)n_order * 8 + 8);
    memcpy(order, order_at, (size_t)n_order * 8);
    for (int l = 0; l <= n; ++l) a[l] = floats((size_t)batch * dims[l]), delta[l] = floats((size_t)batch * dims[l]);
    float *r = floats((size_t)batch);
    const int steps = (n_order + batch - 1) / batch;
    double *losses = (double *)calloc((size_t)steps, sizeof(double));
    int B = 0;

    for (int st = 0; st < steps; ++st) {
        const long long *idx = order + (size_t)st * batch;
        B = n_order - st * batch < batch ? n_order - st * batch : batch;
        /* 1. gather: the row's utterance by bisection of the row offsets, the splice clamped to it */
        for (int m = 0; m < B; ++m) {
            const long long row = idx[m];
            if (row < 0 || row >= rows) die("an index is out of range");
            int lo = 0, hi = n_utt;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (roff[mid] <= row) lo = mid;
                else hi = mid;
            }
            const long long r0 = roff[lo], F = roff[lo + 1] - r0, f = row - r0;
            for (int d = -C; d <= C; ++d) {
                long long q = f + d;
                q = q < 0 ? 0 : (q > F - 1 ? F - 1 : q);
                for (int c = 0; c < 64; ++c) {
                    const int k = (d + C) * 64 + c;
                    const float t = feats[(r0 + q) * 64 + c] + shift[k];
                    a[0][(size_t)m * K0 + k] = t * scale[k];
                }
            }
        }
        /* 2. forward: the inference contract, every layer's output kept */
        for (int l = 1; l <= n; ++l) {
            const int K = dims[l - 1], N = dims[l];
            for (int m = 0; m < B; ++m)
                for (int j = 0; j < N; ++j) {
                    float acc = b[l][j];
                    for (int k = 0; k < K; ++k) acc = sea_fmaf(a[l - 1][(size_t)m * K + k], W[l][(size_t)j * K + k], acc);
                    a[l][(size_t)m * N + j] = sea_dnn_act(acc, act[l - 1]);
                }
        }
        /* 3. loss and 4. output delta */
        for (int m = 0; m < B; ++m) {
            float acc = 0.0f;
            for (int j = 0; j < n_out; ++j) {
                const float y = a[n][(size_t)m * n_out + j];
                const float e = y - targets[idx[m] * n_out + j];
                acc = sea_fmaf(e, e, acc);
                delta[n][(size_t)m * n_out + j] = delta_of(e, y, act[n - 1]);
            }
            r[m] = acc;
        }
        double pl[64], loss = 0.0;
        for (int l = 0; l < 64; ++l) {
            pl[l] = 0.0;
            for (int i = 0; 64 * i + l < B; ++i) pl[l] += (double)r[64 * i + l];
        }
        for (int l = 0; l < 64; ++l) loss += pl[l];
        losses[st] = 0.5 * loss;
        if (!update) continue;
        for (int l = n; l >= 1; --l) {
            const int K = dims[l - 1], N = dims[l];
            /* 5. weight gradient: one chain over m */
            for (int j = 0; j < N; ++j)
                for (int k = 0; k < K; ++k) {
                    float acc = 0.0f;
                    if (!decoy)
                        for (int m = 0; m < B; ++m) acc = sea_fmaf(delta[l][(size_t)m * N + j], a[l - 1][(size_t)m * K + k], acc);
                    else
                        for (int m = B - 1; m >= 0; --m) acc = sea_fmaf(delta[l][(size_t)m * N + j], a[l - 1][(size_t)m * K + k], acc);
                    G[l][(size_t)j * K + k] = acc;
                }
            /* 6. bias gradient */
            for (int j = 0; j < N; ++j) {
                float acc = 0.0f;
                for (int m = 0; m < B; ++m) acc = acc + delta[l][(size_t)m * N + j];
                g[l][j] = acc;
            }
            /* 7. back-propagation, with the weights as they were before this step's update; nothing goes into x0 */
            if (l > 1)
                for (int m = 0; m < B; ++m)
                    for (int k = 0; k < K; ++k) {
                        float acc = 0.0f;
                        if (!decoy)
                            for (int j = 0; j < N; ++j) acc = sea_fmaf(delta[l][(size_t)m * N + j], W[l][(size_t)j * K + k], acc);
                        else
                            for (int j = N - 1; j >= 0; --j) acc = sea_fmaf(delta[l][(size_t)m * N + j], W[l][(size_t)j * K + k], acc);
                        delta[l - 1][(size_t)m * K + k] = delta_of(acc, a[l - 1][(size_t)m * K + k], act[l - 2]);
                    }
        }
        /* 8. update: a multiply then an add, a multiply then a subtract */
        for (int l = 1; l <= n; ++l) {
            const size_t K = (size_t)dims[l - 1], N = (size_t)dims[l];
            for (size_t i = 0; i < N * K; ++i) {
                const float mv = mu * vW[l][i];
                vW[l][i] = mv + G[l][i];
                const float ev = eta * vW[l][i];
                W[l][i] = W[l][i] - ev;
            }
            for (size_t j = 0; j < N; ++j) {
                const float mv = mu * vb[l][j];
                vb[l][j] = mv + g[l][j];
                const float ev = eta * vb[l][j];
                b[l][j] = b[l][j] - ev;
            }
        }
    }

    FILE *f = fopen(out_path, "wb");
    if (!f) die("cannot write the output");
    fwrite(losses, sizeof(double), (size_t)steps, f);
    for (int l = 1; l <= n; ++l) {
        const size_t K = (size_t)dims[l - 1], N = (size_t)dims[l];
        fwrite(W[l], 4, N * K, f), fwrite(b[l], 4, N, f), fwrite(vW[l], 4, N * K, f), fwrite(vb[l], 4, N, f);
    }
    for (int l = 0; l <= n; ++l) fwrite(a[l], 4, (size_t)B * dims[l], f);
    for (int l = 1; l <= n; ++l) fwrite(delta[l], 4, (size_t)B * dims[l], f);
    for (int l = 1; l <= n; ++l) fwrite(G[l], 4, (size_t)dims[l] * dims[l - 1], f), fwrite(g[l], 4, (size_t)dims[l], f);
    if (fclose(f)) die("cannot write the output");
    for (int l = 1; l <= n; ++l) free(W[l]), free(b[l]), free(vW[l]), free(vb[l]), free(G[l]), free(g[l]);
    for (int l = 0; l <= n; ++l) free(a[l]), free(delta[l]);
    free(r), free(losses), free(order), free(roff), free((void *)blob);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "train")) return train(argv[2], argv[3], argc > 4 && !strcmp(argv[4], "decoy"));
    die("usage: train IN OUT [decoy]");
    return 2;
}
