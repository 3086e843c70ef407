/* Stand-alone host driver of the IRM-target kernel's arithmetic for tests/test_irm_cpu.py (no HIP, no GPU; built by g++ with the address
 * and undefined-behaviour sanitizers and -ffp-contract=off, so that every float operation below is exactly the one written).
 *
 *   irm_kernel_driver codelet <seed> <n_random>
 *       csrc/irm_rdft128.inc, included as irm_kernel.hip's rdft128_80 includes it, on the 80 unit impulses and on n_random vectors of
 *       int16-valued floats.  stdout, per input:  "in <80 values>"  then  "out <g_re[0]> <g_im[0]> ... <g_re[63]> <g_im[63]>".
 *   irm_kernel_driver frames <file> <form>
 *       what one lane group of irm_target_kernel does to a frame, in float, in the kernel's order: the window as (float) of the double
 *       formula; x_r[m] = w[4m + r] * x[4m + r]; the codelet; times ((float)cos, (float)-sin)(2 pi r k / 512); the four rows added as
 *       rows_reduce adds them, (row 0 + row 1) + (row 2 + row 3); the 16 powers a row ends with (row 0 bins 0..15, row 1 bins 32..47,
 *       row 2 bins 16..31, row 3 bins 48..63) summed in k order; rows_sum, (row 0 + row 1) + (row 2 + row 3); the ratio.
 *       form 0: the twiddle product and the power sum as written, every product and sum rounded; form 1: with fmaf where a compiler that
 *       contracts may fuse them (a * b - c * d -> fma(a, b, -(c * d)); p + (a * a + b * b) -> p + fma(a, a, b * b)).
 *       <file>: int32 n_cases, then per case int32 window, int32 L, pure [64][L] int16, noise [64][L] int16.
 *       stdout: per case "case <index> <F>", then F lines of 64 ratios ("%.9g", "nan" where both sums are 0). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static void rdft128_80(const float (&x)[80], float (&g_re)[64], float (&g_im)[64])
{
#include "irm_rdft128.inc"
}

static const double kPi = 3.1415926535897932384626433832795;

static float window_at(int kind, int i)
{
    double w = 1.0;
    if (kind == 1) w = 0.54 - 0.46 * cos(2.0 * kPi * i / 319.0);
    if (kind == 2) w = 0.5 - 0.5 * cos(2.0 * kPi * i / 319.0);
    return (float)w;
}

/* sum over bins 0..63 of |X[k]|^2 of one frame (320 samples at s), as the four rows of a lane group leave it */
static float frame_power(const int16_t *s, const float (&w)[320], const float (&tw_re)[4][64], const float (&tw_im)[4][64], int form)
{
    float re[4][64], im[4][64];
    for (int r = 0; r < 4; ++r) {
        float x[80], g_re[64], g_im[64];
        for (int m = 0; m < 80; ++m) x[m] = (float)s[4 * m + r] * w[4 * m + r];
        rdft128_80(x, g_re, g_im);
        for (int k = 0; k < 64; ++k) {
            const float tx = tw_re[r][k], ty = tw_im[r][k];
            if (form == 0) {
                re[r][k] = g_re[k] * tx - g_im[k] * ty;
                im[r][k] = g_re[k] * ty + g_im[k] * tx;
            } else {
                re[r][k] = fmaf(g_re[k], tx, -(g_im[k] * ty));
                im[r][k] = fmaf(g_re[k], ty, g_im[k] * tx);
            }
        }
    }
    static const int first_bin[4] = {0, 32, 16, 48}; /* the quarter of the bins row 0, 1, 2, 3 ends with */
    float p[4];
    for (int row = 0; row < 4; ++row) {
        float acc = 0.0f;
        for (int j = 0; j < 16; ++j) {
            const int k = first_bin[row] + j;
            const float qre = (re[0][k] + re[1][k]) + (re[2][k] + re[3][k]);
            const float qim = (im[0][k] + im[1][k]) + (im[2][k] + im[3][k]);
            if (form == 0)
                acc += qre * qre + qim * qim;
            else
                acc += fmaf(qre, qre, qim * qim);
        }
        p[row] = acc;
    }
    return (p[0] + p[1]) + (p[2] + p[3]);
}

static int run_codelet(unsigned seed, int n_random)
{
    uint64_t state = seed * 2654435761u + 12345u;
    for (int t = 0; t < 80 + n_random; ++t) {
        float x[80], g_re[64], g_im[64];
        for (int n = 0; n < 80; ++n) {
            if (t < 80) {
                x[n] = n == t ? 1.0f : 0.0f;
            } else {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                x[n] = (float)((int)((state >> 33) & 0xffffu) - 32768);
            }
        }
        rdft128_80(x, g_re, g_im);
        printf("in");
        for (int n = 0; n < 80; ++n) printf(" %.9g", (double)x[n]);
        printf("\nout");
        for (int k = 0; k < 64; ++k) printf(" %.9g %.9g", (double)g_re[k], (double)g_im[k]);
        printf("\n");
    }
    return 0;
}

static int run_frames(const char *path, int form)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 3;
    int32_t n_cases = 0;
    if (fread(&n_cases, sizeof n_cases, 1, f) != 1 || n_cases < 0) return 4;
    float tw_re[4][64], tw_im[4][64];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 64; ++k) {
            const double ang = 2.0 * kPi * (double)(r * k) / 512.0;
            tw_re[r][k] = (float)cos(ang);
            tw_im[r][k] = (float)-sin(ang);
        }
    for (int32_t i = 0; i < n_cases; ++i) {
        int32_t head[2];
        if (fread(head, sizeof head[0], 2, f) != 2) return 5;
        const int kind = head[0];
        const long L = head[1];
        if (kind < 0 || kind > 2 || L < 0 || L > (1L << 24)) return 6;
        std::vector<int16_t> pure((size_t)64 * L), noise((size_t)64 * L);
        if (L && (fread(pure.data(), sizeof(int16_t), pure.size(), f) != pure.size() ||
                  fread(noise.data(), sizeof(int16_t), noise.size(), f) != noise.size()))
            return 7;
        float w[320];
        for (int n = 0; n < 320; ++n) w[n] = window_at(kind, n);
        const long F = L >= 320 ? (L - 320) / 160 + 1 : 0;
        printf("case %d %ld\n", (int)i, F);
        for (long fr = 0; fr < F; ++fr) {
            for (int c = 0; c < 64; ++c) {
                const float sp = frame_power(pure.data() + (size_t)c * L + 160 * fr, w, tw_re, tw_im, form);
                const float sn = frame_power(noise.data() + (size_t)c * L + 160 * fr, w, tw_re, tw_im, form);
                printf(c ? " %.9g" : "%.9g", (double)(sp / (sp + sn)));
            }
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "codelet")) return run_codelet((unsigned)atoi(argv[2]), atoi(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "frames")) return run_frames(argv[2], atoi(argv[3]));
    return 2;
}
