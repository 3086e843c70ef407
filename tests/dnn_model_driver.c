/*
 * dnn_model_driver.c -- the plain-C model of the DNN mask estimator: the splice, the shift and the
 * scale, and the fmaf chains of the layers, stated literally, with the two elementary functions of csrc/dnn_math.h -- the
 * header the device code includes.  Built by tests/dnn_model.py with gcc -O2 -ffp-contract=off.
 *
 *   forward NET OUT [decoy]   the network on the features of NET (layout below) -> OUT, floats [rows][dims[n]]
 *                             decoy: the splice clamps at the ends of the whole list, not of the utterance
 *   lnf IN OUT                sea_lnf of every float of IN
 *   act IN OUT KIND           sea_dnn_act of every float of IN
 *   lnf_sweep                 every float of [1, 2^39] against the double log: the largest error in ulps
 *   exp_sweep                 every float z of [-20, 20] and a stride through [-88, 88]: the sigmoid against double, the
 *                             exponential (of -z) against double
 *
 * NET: int32 context, n_layers, dims[n_layers + 1], act[n_layers], n_utt, n_rows[n_utt]; then float32 shift[K0], scale[K0],
 * per layer W[out][in] and b[out], per utterance feats[n_rows][64].
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dnn_math.h"

static void die(const char *what)
{
    fprintf(stderr, "dnn_model_driver: %s\n", what);
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

static void spill(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) die("cannot write the output");
    fclose(f);
}

static int forward(const char *net, const char *out_path, int decoy)
{
    size_t bytes;
    const int32_t *h = (const int32_t *)slurp(net, &bytes);
    const int C = h[0], n_layers = h[1];
    const int32_t *dims = h + 2, *act = dims + n_layers + 1;
    const int n_utt = act[n_layers];
    const int32_t *n_rows = act + n_layers + 1;
    const float *p = (const float *)(n_rows + n_utt);
    const int K0 = 64 * (2 * C + 1);
    if (dims[0] != K0) die("dims[0] != K0");
    const float *shift = p, *scale = p + K0;
    p += 2 * (size_t)K0;
    const float *W[8], *b[8];
    int max_dim = K0;
    for (int l = 0; l < n_layers; ++l) {
        W[l] = p;
        p += (size_t)dims[l + 1] * dims[l];
        b[l] = p;
        p += dims[l + 1];
        if (dims[l + 1] > max_dim) max_dim = dims[l + 1];
    }
    long rows = 0;
    for (int u = 0; u < n_utt; ++u) rows += n_rows[u];
    const float *feats = p;
    if ((const char *)(feats + rows * 64) != (const char *)h + bytes) die("the input's size does not match its header");
    const int n_out = dims[n_layers];
    float *out = (float *)malloc((size_t)(rows ? rows : 1) * n_out * sizeof(float));
    float *x = (float *)malloc((size_t)max_dim * sizeof(float)), *y = (float *)malloc((size_t)max_dim * sizeof(float));
    long r0 = 0;
    for (int u = 0; u < n_utt; ++u) {
        const long F = n_rows[u];
        for (long f = 0; f < F; ++f) {
            for (int d = -C; d <= C; ++d) {
                long g = f + d; /* the row of the splice, clamped to the utterance */
                if (decoy) {
                    g += r0;
                    g = g < 0 ? 0 : (g > rows - 1 ? rows - 1 : g);
                } else {
                    g = g < 0 ? 0 : (g > F - 1 ? F - 1 : g);
                    g += r0;
                }
                for (int c = 0; c < 64; ++c) {
                    const int k = (d + C) * 64 + c;
                    const float t = feats[g * 64 + c] + shift[k]; /* a float add ... */
                    x[k] = t * scale[k];                          /* ... then a float multiply */
                }
            }
            for (int l = 0; l < n_layers; ++l) {
                const int K = dims[l], N = dims[l + 1];
                for (int j = 0; j < N; ++j) {
                    float acc = b[l][j];
                    for (int k = 0; k < K; ++k) acc = sea_fmaf(x[k], W[l][(size_t)j * K + k], acc);
                    y[j] = sea_dnn_act(acc, act[l]);
                }
                float *t = x;
                x = y;
                y = t;
            }
            memcpy(out + (r0 + f) * n_out, x, (size_t)n_out * sizeof(float));
        }
        r0 += F;
    }
    spill(out_path, out, (size_t)rows * n_out * sizeof(float));
    free(x), free(y), free(out), free((void *)h);
    return 0;
}

static int map_file(const char *in, const char *out_path, int kind)
{
    size_t bytes;
    float *v = (float *)slurp(in, &bytes);
    const size_t n = bytes / sizeof(float);
    for (size_t i = 0; i < n; ++i) v[i] = kind < 0 ? sea_lnf(v[i]) : sea_dnn_act(v[i], kind);
    spill(out_path, v, n * sizeof(float));
    free(v);
    return 0;
}

/* ---- the sweeps: a range of float bit patterns cut over the processors ---------------------------------------------------- */
typedef struct {
    uint32_t lo, hi; /* bit patterns lo .. hi - 1, of which this job takes the blocks of 2^16 numbered first, first + step, .. */
    int first, step;
    int sign;        /* exp sweep: the sign of z */
    double worst[3];
    float at[3];
} Job;

static double ulp_of(double t)
{ /* the spacing of the floats at |t| (t a normal float's magnitude) */
    int e;
    frexp(fabs(t), &e);
    return ldexp(1.0, e - 24);
}

static void *lnf_job(void *arg)
{
    Job *j = (Job *)arg;
    for (uint64_t b = j->lo + ((uint64_t)j->first << 16); b < j->hi; b += (uint64_t)j->step << 16)
        for (uint64_t u = b; u < b + 65536 && u < j->hi; ++u) {
            const float y = sea_dnn_float((uint32_t)u), got = sea_lnf(y);
            const double want = log((double)y);
            const double err = want == 0.0 ? (got == 0.0f ? 0.0 : INFINITY) : fabs((double)got - want) / ulp_of(want);
            if (!(err <= j->worst[0])) j->worst[0] = err, j->at[0] = y;
        }
    return NULL;
}

/* worst[0]: |sigmoid_float - sigmoid_double|; worst[1]: the exponential's relative error where its value is a normal float;
 * worst[2]: its absolute error in units of 2^-149 where it is not */
static void exp_point(Job *j, float z)
{
    const float s = sea_dnn_act(z, 1), e = sea_expf(-z);
    /* below 2^-30 the double logistic function is 1/2 + z/4 to the last bit (the next term is z^3 / 48 < 2^-95) */
    const int tiny = fabsf(z) < 0x1p-30f;
    const double zc = z > 88.0f ? 88.0 : (z < -88.0f ? -88.0 : (double)z); /* the exponential's argument is clamped */
    const double sd = tiny ? 0.5 + 0.25 * (double)z : 1.0 / (1.0 + exp(-(double)z));
    const double ed = tiny ? 1.0 - (double)z : exp(-zc);
    const double es = fabs((double)s - sd);
    if (!(es <= j->worst[0])) j->worst[0] = es, j->at[0] = z;
    if (ed >= 0x1p-126) {
        const double ee = fabs((double)e - ed);
        if (!(ee <= j->worst[1] * ed)) j->worst[1] = ee / ed, j->at[1] = z;
    } else {
        const double ea = fabs((double)e - ed) / 0x1p-149;
        if (!(ea <= j->worst[2])) j->worst[2] = ea, j->at[2] = z;
    }
}

static void *exp_job(void *arg)
{
    Job *j = (Job *)arg;
    for (uint64_t b = j->lo + ((uint64_t)j->first << 16); b < j->hi; b += (uint64_t)j->step << 16)
        for (uint64_t u = b; u < b + 65536 && u < j->hi; ++u) exp_point(j, sea_dnn_float((uint32_t)u | (j->sign ? 0x80000000u : 0u)));
    return NULL;
}

static int sweep(void *(*fn)(void *), uint32_t lo, uint32_t hi, int both_signs, Job *total)
{
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    const int T = ncpu < 1 ? 1 : (ncpu > 16 ? 16 : (int)ncpu), n = T * (both_signs ? 2 : 1);
    pthread_t th[32];
    Job jobs[32];
    for (int i = 0; i < n; ++i) {
        memset(&jobs[i], 0, sizeof jobs[i]);
        jobs[i].lo = lo;
        jobs[i].hi = hi;
        jobs[i].first = i % T;
        jobs[i].step = T;
        jobs[i].sign = i / T;
        if (pthread_create(&th[i], NULL, fn, &jobs[i])) die("pthread_create");
    }
    for (int i = 0; i < n; ++i) {
        pthread_join(th[i], NULL);
        for (int q = 0; q < 3; ++q)
            if (!(jobs[i].worst[q] <= total->worst[q])) total->worst[q] = jobs[i].worst[q], total->at[q] = jobs[i].at[q];
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "forward")) return forward(argv[2], argv[3], argc > 4 && !strcmp(argv[4], "decoy"));
    if (argc == 4 && !strcmp(argv[1], "lnf")) return map_file(argv[2], argv[3], -1);
    if (argc == 5 && !strcmp(argv[1], "act")) return map_file(argv[2], argv[3], atoi(argv[4]));
    if (argc == 2 && !strcmp(argv[1], "lnf_sweep")) {
        Job total;
        memset(&total, 0, sizeof total);
        const uint32_t lo = sea_dnn_bits(1.0f), hi = sea_dnn_bits(0x1p39f) + 1;
        sweep(lnf_job, lo, hi, 0, &total);
        printf("n=%llu max_ulp=%.9g at=%a\n", (unsigned long long)(hi - lo), total.worst[0], (double)total.at[0]);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "exp_sweep")) {
        Job total;
        memset(&total, 0, sizeof total);
        const uint32_t hi = sea_dnn_bits(20.0f) + 1;
        sweep(exp_job, 0, hi, 1, &total); /* +-0, every subnormal, every float up to +-20 */
        unsigned long long n = 2ULL * hi;
        for (int i = -88000; i <= 88000; ++i, ++n) exp_point(&total, (float)i / 1000.0f); /* the stride through +-88 */
        exp_point(&total, 88.0f), exp_point(&total, -88.0f), exp_point(&total, 100.0f), exp_point(&total, -100.0f);
        printf("n=%llu sigmoid_abs=%.9g at=%a exp_rel=%.9g at=%a exp_subnormal_ulps=%.9g at=%a\n", n + 4, total.worst[0],
               (double)total.at[0], total.worst[1], (double)total.at[1], total.worst[2], (double)total.at[2]);
        return 0;
    }
    die("usage: forward NET OUT [decoy] | lnf IN OUT | act IN OUT KIND | lnf_sweep | exp_sweep");
    return 2;
}
