/*
 * score_model_driver.c -- the plain-C model of the objective scores: the loops of the contract stated
 * literally, with sea_lnf of csrc/dnn_math.h -- the header the device code includes.  Built by tests/score_model.py with
 * gcc -O2 -ffp-contract=off, and with -fsanitize=address,undefined as a stand-alone program.
 *
 *   score IN OUT    IN: int32 hop, n_utt; int64 lengths[n_utt]; per utterance int16 ref[L], est[L]
 *                   OUT: per utterance int64 Srr, See, Sre, double seg_sum, int64 seg_frames, float d[F] (a skipped frame
 *                   0x7fc00000)
 *   mask IN OUT     IN: int32 n_utt, 0; float t_est, t_ideal; int32 rows[n_utt]; per utterance float est[rows][64],
 *                   ideal[rows][64].  OUT: int64 n11, n10, n01, n00 per utterance
 *   lnf_sweep       every float of (2^39, 2^41] against the double log: the largest error in ulps
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dnn_math.h"

static void die(const char *what)
{
    fprintf(stderr, "score_model_driver: %s\n", what);
    exit(2);
}

static unsigned char *slurp(const char *path, size_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open the input");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *p = (unsigned char *)malloc((size_t)n + 16);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) die("cannot read the input");
    fclose(f);
    *bytes = (size_t)n;
    return p;
}

static void put(FILE *f, const void *p, size_t bytes)
{
    if (fwrite(p, 1, bytes, f) != bytes) die("cannot write the output");
}

static int score(const char *in, const char *out_path)
{
    size_t bytes;
    unsigned char *buf = slurp(in, &bytes);
    int32_t head[2];
    memcpy(head, buf, sizeof head);
    const int hop = head[0], n_utt = head[1];
    if (hop != 80 && hop != 160) die("hop");
    int64_t *lengths = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n_utt ? n_utt : 1));
    memcpy(lengths, buf + 8, sizeof(int64_t) * (size_t)n_utt);
    const unsigned char *p = buf + 8 + 8 * (size_t)n_utt;
    FILE *out = fopen(out_path, "wb");
    if (!out) die("cannot write the output");
    const float c = 0x1.15f2cep+2f; /* the float nearest 10 / ln 10 */
    for (int u = 0; u < n_utt; ++u) {
        const int64_t L = lengths[u];
        if (p + 4 * (size_t)L > buf + bytes) die("the input's size does not match its header");
        int16_t *ref = (int16_t *)malloc(2 * (size_t)L + 2), *est = (int16_t *)malloc(2 * (size_t)L + 2);
        memcpy(ref, p, 2 * (size_t)L);
        memcpy(est, p + 2 * (size_t)L, 2 * (size_t)L);
        p += 4 * (size_t)L;
        int64_t S[3] = {0, 0, 0}; /* the whole utterance, the tail past the last frame included */
        for (int64_t i = 0; i < L; ++i) {
            const int64_t r = ref[i], e = est[i];
            S[0] += r * r, S[1] += e * e, S[2] += r * e;
        }
        const int64_t F = L < 2 * hop ? 0 : (L - 2 * hop) / hop + 1;
        float *d = (float *)malloc(sizeof(float) * (size_t)(F ? F : 1));
        int64_t used = 0;
        for (int64_t f = 0; f < F; ++f) {
            int64_t srr = 0, see = 0, sre = 0;
            for (int64_t i = hop * f; i < hop * f + 2 * hop; ++i) {
                const int64_t r = ref[i], e = est[i];
                srr += r * r, see += e * e, sre += r * e;
            }
            if (srr == 0) {
                d[f] = sea_dnn_float(0x7fc00000u);
                continue;
            }
            const int64_t n = srr - 2 * sre + see;
            const float a = sea_lnf((float)(srr + 1)), b = sea_lnf((float)(n + 1));
            const float diff = a - b;
            float v = diff * c;
            v = v < -10.0f ? -10.0f : v > 35.0f ? 35.0f : v;
            d[f] = v;
            ++used;
        }
        double lane[64], seg = 0.0;
        for (int l = 0; l < 64; ++l) {
            lane[l] = 0.0;
            for (int64_t f = l; f < F; f += 64)
                if (sea_dnn_bits(d[f]) != 0x7fc00000u) lane[l] += (double)d[f];
        }
        for (int l = 0; l < 64; ++l) seg += lane[l];
        put(out, S, sizeof S);
        put(out, &seg, sizeof seg);
        put(out, &used, sizeof used);
        put(out, d, sizeof(float) * (size_t)F);
        free(ref), free(est), free(d);
    }
    if (p != buf + bytes) die("the input's size does not match its header");
    fclose(out);
    free(lengths), free(buf);
    return 0;
}

static int mask(const char *in, const char *out_path)
{
    size_t bytes;
    unsigned char *buf = slurp(in, &bytes);
    int32_t head[2];
    float t[2];
    memcpy(head, buf, sizeof head);
    memcpy(t, buf + 8, sizeof t);
    const int n_utt = head[0];
    int32_t *rows = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_utt ? n_utt : 1));
    memcpy(rows, buf + 16, sizeof(int32_t) * (size_t)n_utt);
    const unsigned char *p = buf + 16 + 4 * (size_t)n_utt;
    FILE *out = fopen(out_path, "wb");
    if (!out) die("cannot write the output");
    for (int u = 0; u < n_utt; ++u) {
        const size_t n = (size_t)rows[u] * 64;
        if (p + 8 * n > buf + bytes) die("the input's size does not match its header");
        int64_t count[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < n; ++i) {
            float e, x;
            memcpy(&e, p + 4 * i, 4);
            memcpy(&x, p + 4 * (n + i), 4);
            const int e_on = e > t[0], x_on = x > t[1];
            ++count[e_on ? (x_on ? 0 : 1) : (x_on ? 2 : 3)];
        }
        p += 8 * n;
        put(out, count, sizeof count);
    }
    if (p != buf + bytes) die("the input's size does not match its header");
    fclose(out);
    free(rows), free(buf);
    return 0;
}

static int lnf_sweep(void)
{
    const uint32_t lo = sea_dnn_bits(0x1p39f) + 1, hi = sea_dnn_bits(0x1p41f);
    double worst = 0.0;
    float at = 0.0f;
    for (uint32_t u = lo; u <= hi; ++u) {
        const float y = sea_dnn_float(u), got = sea_lnf(y);
        const double want = log((double)y);
        int e;
        frexp(want, &e);
        const double err = fabs((double)got - want) / ldexp(1.0, e - 24); /* in spacings of the floats at `want` */
        if (!(err <= worst)) worst = err, at = y;
    }
    printf("n=%llu max_ulp=%.9g at=%a\n", (unsigned long long)(hi - lo + 1), worst, (double)at);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "score")) return score(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "mask")) return mask(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "lnf_sweep")) return lnf_sweep();
    die("usage: score IN OUT | mask IN OUT | lnf_sweep");
    return 2;
}
