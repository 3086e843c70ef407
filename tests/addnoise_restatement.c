/*
 * addnoise_restatement.c -- the SNR mixer's arithmetic written in plain C from its description, for
 * tests/test_trainset_cpu.py.  Only the expression shapes matter: a float accumulator fed by `int * int * 1.0`, a double pow
 * and a double sqrt each assigned to a float, `a / b / c` in float, and a float product assigned to a short.  The test
 * compiles it at -O0 and -O2 and compares both with the numpy model; it is given no input whose product leaves the int16
 * range or is NaN, where C leaves the conversion undefined.
 *
 *   in   int32 n_cases, then per case: int32 L, int32 db, int16 pure[L], int16 noise[L]
 *   out  per case: float puresum, float noisesum, float gain, int16 noise[L] (scaled), int16 noisy[L]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

/* energy of a signal the way the mixer takes it: a float total that receives int * int * 1.0, sample after sample */
static float energy_in_order(const short *x, long n)
{
    float total = 0;
    long k;
    for (k = 0; k < n; k++) total += x[k] * x[k] * 1.0;
    return total;
}

/* scales `noise` in place to `snr_db` below `clean` and writes their sum to `mix`; report3 = both energies and the factor */
static void mix_at_snr(const short *clean, short *noise, short *mix, long n, int snr_db, float *report3)
{
    float ratio = pow(10.0, snr_db / 10.0);
    float e_clean = energy_in_order(clean, n);
    float e_noise = energy_in_order(noise, n);
    float factor = sqrt(e_clean / e_noise / ratio);
    long k;
    for (k = 0; k < n; k++) {
        noise[k] = noise[k] * factor;
        mix[k] = clean[k] + noise[k];
    }
    report3[0] = e_clean;
    report3[1] = e_noise;
    report3[2] = factor;
}

int main(int argc, char **argv)
{
    FILE *in, *out;
    int n, k;
    if (argc < 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    if (fread(&n, sizeof n, 1, in) != 1) return 2;
    for (k = 0; k < n; k++) {
        int L, db;
        short *pure, *noise, *noisy;
        float out3[3];
        if (fread(&L, sizeof L, 1, in) != 1 || fread(&db, sizeof db, 1, in) != 1) return 2;
        pure = (short *)malloc((size_t)L * sizeof(short));
        noise = (short *)malloc((size_t)L * sizeof(short));
        noisy = (short *)malloc((size_t)L * sizeof(short));
        if (fread(pure, sizeof(short), (size_t)L, in) != (size_t)L || fread(noise, sizeof(short), (size_t)L, in) != (size_t)L) return 2;
        mix_at_snr(pure, noise, noisy, L, db, out3);
        fwrite(out3, sizeof(float), 3, out);
        fwrite(noise, sizeof(short), (size_t)L, out);
        fwrite(noisy, sizeof(short), (size_t)L, out);
        free(pure), free(noise), free(noisy);
    }
    fclose(in);
    return fclose(out) ? 1 : 0;
}
