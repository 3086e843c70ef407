/*
 * stoi_model_driver.c -- the STOI contract stated literally in plain C: every operation a single
 * correctly rounded float + - * / or sqrtf (built with -ffp-contract=off), the chains the contract names through sea_fmaf, the
 * tables from the same csrc/stoi_tables.inc the library includes.  The GPU results must equal this program's bit for bit.
 *
 *   stoi_model_driver stoi IN OUT
 *     IN:  int32 rate, int32 n; int64 length [n]; per utterance int16 ref [L], int16 est [L]
 *     OUT: per utterance int64 frames, int64 kept, int64 terms, double stoi_sum, float d [terms]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dnn_math.h"
#include "stoi_tables.inc"

static const float W[256] = {SEA_STOI_W_VALUES};
static const float CS[512] = {SEA_STOI_CS_VALUES};
static const float H16[161] = {SEA_STOI_H16_VALUES};
static const float H8[101] = {SEA_STOI_H8_VALUES};
static const int LO[16] = {SEA_STOI_BAND_LO};

static void *xmalloc(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p) {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    return p;
}

/* step a */
static float *resample(const int16_t *x, long long L, int rate, long long *L10)
{
    const int p = 5, q = rate == 16000 ? 8 : 4, half = rate == 16000 ? 80 : 50;
    const float *h = rate == 16000 ? H16 : H8;
    *L10 = (5 * L + q - 1) / q;
    float *y = xmalloc((size_t)*L10 * sizeof(float));
    for (long long i = 0; i < *L10; ++i) {
        float acc = 0.0f;
        for (long long k = i * q > half ? (i * q - half + p - 1) / p : 0; k < L; ++k) { /* the first k with i q - k p <= half */
            const long long t = i * q - k * p;
            if (t < -half) break;
            acc = sea_fmaf(h[half + t], (float)x[k], acc);
        }
        y[i] = acc;
    }
    return y;
}

/* step c: z [128 (M + 1)] from the kept frames of x10 */
static float *overlap_add(const float *x10, const long long *keep, long long M)
{
    float *z = xmalloc((size_t)(128 * (M + 1)) * sizeof(float));
    for (long long j = 0; j <= M; ++j)
        for (int n = 0; n < 128; ++n) {
            float v;
            if (j == 0) v = W[n] * x10[128 * keep[0] + n];
            else if (j == M) v = W[n + 128] * x10[128 * keep[M - 1] + n + 128];
            else v = W[n + 128] * x10[128 * keep[j - 1] + n + 128] + W[n] * x10[128 * keep[j] + n];
            z[128 * j + n] = v;
        }
    return z;
}

/* step d: [M][15] */
static float *bands(const float *z, long long M)
{
    float *X = xmalloc((size_t)(M * 15) * sizeof(float));
    for (long long m = 0; m < M; ++m) {
        float v[256], p[256];
        for (int n = 0; n < 256; ++n) v[n] = W[n] * z[128 * m + n];
        for (int k = 7; k <= 218; ++k) {
            float re = 0.0f, im = 0.0f;
            for (int n = 0; n < 256; ++n) re = sea_fmaf(v[n], CS[(n * k) & 511], re);
            for (int n = 0; n < 256; ++n) im = sea_fmaf(v[n], CS[(n * k + 128) & 511], im);
            p[k] = im * im + re * re;
        }
        for (int j = 0; j < 15; ++j) {
            float s = 0.0f;
            for (int k = LO[j]; k < LO[j + 1]; ++k) s = s + p[k];
            X[m * 15 + j] = sqrtf(s);
        }
    }
    return X;
}

/* step e for segment s, band j */
static float segment(const float *X, const float *Y, long long s, int j)
{
    float sx = 0.0f, sy = 0.0f;
    for (int f = 0; f < 30; ++f) {
        const float x = X[(s + f) * 15 + j], y = Y[(s + f) * 15 + j];
        sx = sx + x * x;
        sy = sy + y * y;
    }
    if (sy == 0.0f) return 0.0f;
    const float a = sqrtf(sx / sy);
    float yc[30], mx = 0.0f, my = 0.0f;
    for (int f = 0; f < 30; ++f) {
        const float x = X[(s + f) * 15 + j], t = a * Y[(s + f) * 15 + j], c = SEA_STOI_CLIP * x;
        yc[f] = t < c ? t : c;
        mx = mx + x;
        my = my + yc[f];
    }
    mx = mx / 30.0f;
    my = my / 30.0f;
    float num = 0.0f, vx = 0.0f, vy = 0.0f;
    for (int f = 0; f < 30; ++f) {
        const float dx = X[(s + f) * 15 + j] - mx, dy = yc[f] - my;
        num = num + dx * dy;
        vx = vx + dx * dx;
        vy = vy + dy * dy;
    }
    const float den = sqrtf(vx) * sqrtf(vy);
    return den > 0.0f ? num / den : 0.0f;
}

static void stoi(const int16_t *ref, const int16_t *est, long long L, int rate, FILE *out)
{
    long long L10;
    float *r10 = resample(ref, L, rate, &L10), *e10 = resample(est, L, rate, &L10);
    /* step b */
    const long long F = L10 < 256 ? 0 : (L10 - 256) / 128 + 1;
    float *e = xmalloc((size_t)F * sizeof(float)), emax = 0.0f;
    for (long long f = 0; f < F; ++f) {
        float s = 0.0f;
        for (int n = 0; n < 256; ++n) {
            const float v = W[n] * r10[128 * f + n];
            s = s + v * v;
        }
        e[f] = s;
        if (s > emax) emax = s;
    }
    long long *keep = xmalloc((size_t)F * sizeof(long long)), M = 0;
    for (long long f = 0; f < F; ++f)
        if (e[f] * 10000.0f > emax) keep[M++] = f;
    const long long S = M > 29 ? M - 29 : 0, terms = 15 * S;
    float *d = xmalloc((size_t)terms * sizeof(float));
    if (M > 0) {
        float *zr = overlap_add(r10, keep, M), *ze = overlap_add(e10, keep, M);
        float *X = bands(zr, M), *Y = bands(ze, M);
        for (long long s = 0; s < S; ++s)
            for (int j = 0; j < 15; ++j) d[15 * s + j] = segment(X, Y, s, j);
        free(zr), free(ze), free(X), free(Y);
    }
    /* step f: the shape of one wave */
    double lanes[64], sum = 0.0;
    for (int l = 0; l < 64; ++l) {
        lanes[l] = 0.0;
        for (long long i = l; i < terms; i += 64) lanes[l] += (double)d[i];
    }
    for (int l = 0; l < 64; ++l) sum += lanes[l];
    fwrite(&F, 8, 1, out), fwrite(&M, 8, 1, out), fwrite(&terms, 8, 1, out), fwrite(&sum, 8, 1, out);
    fwrite(d, sizeof(float), (size_t)terms, out);
    free(r10), free(e10), free(e), free(keep), free(d);
}

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "stoi")) {
        fprintf(stderr, "usage: %s stoi IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    int32_t head[2];
    if (!in || !out || fread(head, 4, 2, in) != 2 || (head[0] != 16000 && head[0] != 8000) || head[1] < 0) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    const int n = head[1];
    int64_t *lens = xmalloc((size_t)n * sizeof(int64_t));
    if (fread(lens, 8, (size_t)n, in) != (size_t)n) return 2;
    for (int u = 0; u < n; ++u) {
        const size_t L = (size_t)lens[u];
        int16_t *ref = xmalloc(L * 2), *est = xmalloc(L * 2);
        if (fread(ref, 2, L, in) != L || fread(est, 2, L, in) != L) return 2;
        stoi(ref, est, (long long)L, head[0], out);
        free(ref), free(est);
    }
    free(lens);
    fclose(in);
    return fclose(out) ? 2 : 0;
}
