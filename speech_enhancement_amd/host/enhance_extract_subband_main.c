/*
 * enhance_extract_subband_main.c -- file-in/file-out driver of the training-set builder with the reference's command line
 * (enhancement_extract_subband_linux/cpp/main.cpp:50-279; fixed-SNR variant: enhancement_extract_test/cpp/main.cpp) over
 * sea_trainset_utterances.
 *
 *   cfg   20 positional "key value" lines (sea_read_extract_cfg)
 *   in    <purewavDictionary><id>.wav for every id of purewavlist; the four noise files
 *   out   <outputDictionary><save_noisy_dir><id>_noisy.wav
 *         <outputDictionary><save_subband_pure_wav_dir><id>_<chan>.wav, ...<save_subband_noise_wav_dir><id>_noise_<chan>.wav,
 *         ...<save_subband_noisy_wav_dir><id>_noisy_<chan>.wav, chan 0..63   (not with --no-subband-wavs)
 *         <outputDictionary>IRM.sIRM : one text matrix per utterance appended under the id <id>_noisy (sea_mask_text_write)
 *         <outputDictionary><Log> : the reference's entries and one line "<id> <rec> <off> <db>" per utterance, the plan used
 *
 * The plan -- noise recording 0..3, offset of the stretch, dB -- is drawn as the reference draws it (sea_plan_draw) from
 * srand (seed); --seed N makes a run repeatable (the reference seeds with the clock, as the default here does), --fixed is
 * enhancement_extract_test's plan (noisepath1, offset 0, the cfg's addnoisedB), --plan FILE takes it from a plan file or an
 * earlier Log.  An utterance whose plan cannot run (a recording shorter than the utterance, fewer than 320 samples, no line in
 * the plan file) is reported and skipped and makes the exit status non-zero; the reference reads out of bounds there.
 *
 * func: the reference's test is inverted -- mixing is ON unless func is "test" (main.cpp:89-90) -- and so it is here: with
 * func equal to "test" the noisy file is a copy of the clean one, the noise subbands are those of the unscaled stretch, and no
 * IRM is written.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/sea_mi355x.h"
#include "sea_host.h"

static void usage(const char *argv0)
{
    fprintf(stderr,
            "usage: %s <cfg> [--no-subband-wavs] [--seed N | --fixed | --plan FILE]\n"
            "  cfg: the 20 lines of the reference's Read_CFG.  func: as in the reference, mixing is ON unless func is \"test\"\n"
            "  (its test is inverted); with func = test the noisy file is a copy of the clean one and no IRM is written.\n"
            "  --no-subband-wavs  write only <id>_noisy.wav and IRM.sIRM, not the 192 subband files per utterance\n"
            "  --seed N           seed of the plan draw (default: the clock, as in the reference)\n"
            "  --fixed            enhancement_extract_test's plan: noisepath1, offset 0, the cfg's addnoisedB\n"
            "  --plan FILE        lines \"<id> <rec> <off> <db>\" (rec 0..3), e.g. the Log of an earlier run\n",
            argv0);
}

typedef struct {
    char *id;
    short *clean, *noisy, *sub[3];
    float *irm;
    long len;
    int fs;
    sea_plan plan;
} utt_t;

static void utt_free(utt_t *u)
{
    int s;
    free(u->clean);
    free(u->noisy);
    free(u->irm);
    for (s = 0; s < 3; s++) free(u->sub[s]);
    memset(u, 0, sizeof *u);
}

static int write_subbands(const sea_extract_cfg *o, const char *dir, const char *tail, const char *id, const short *blk, long L, int fs)
{
    char path[4 * SEA_FILE_LEN];
    int ch;
    for (ch = 0; ch < 64; ch++) {
        snprintf(path, sizeof path, "%s%s%s%s_%d.wav", o->outputDictionary, dir, id, tail, ch);
        if (sea_wav_write(path, blk + (size_t)ch * L, L, fs)) return 1;
    }
    return 0;
}

int main(int argc, char *argv[])
{
    sea_extract_cfg o;
    char path[4 * SEA_FILE_LEN], **ids = NULL;
    const char *plan_file = NULL;
    int n_ids, k, a, rc = 0, want_sub = 1, fixed = 0, mix, group, fs = 0;
    unsigned seed = (unsigned)time(0);
    short *noise[4] = {NULL, NULL, NULL, NULL};
    long noise_len[4] = {0, 0, 0, 0};
    FILE *Log, *fp_irm = NULL;
    sea_plan_table *plan_table = NULL;
    utt_t *U;
    if (argc < 2) {
        usage(argv[0]);
        return 2;
    }
    for (a = 2; a < argc; a++) {
        if (!strcmp(argv[a], "--no-subband-wavs")) want_sub = 0;
        else if (!strcmp(argv[a], "--fixed")) fixed = 1;
        else if (!strcmp(argv[a], "--seed") && a + 1 < argc) seed = (unsigned)strtoul(argv[++a], NULL, 10);
        else if (!strcmp(argv[a], "--plan") && a + 1 < argc) plan_file = argv[++a];
        else {
            usage(argv[0]);
            return 2;
        }
    }
    if (sea_read_extract_cfg(argv[1], &o)) return 2;
    mix = strcmp(o.func, "test") != 0;
    n_ids = sea_read_list(o.purewavlist, &ids);
    if (n_ids < 0) {
        fprintf(stderr, "Open %s file error!\n", o.purewavlist);
        return 2;
    }
    for (k = 0; k < 4; k++) {
        int fs_k = 0;
        if (sea_wav_read(o.noisepath[k], &noise[k], &noise_len[k], &fs_k)) {
            fprintf(stderr, "ERROR:   cannot read the noise file %s\n", o.noisepath[k]);
            return 2;
        }
        if (k && fs_k != fs) {
            fprintf(stderr, "ERROR:   the noise file %s is sampled at %d Hz, %s at %d Hz\n", o.noisepath[k], fs_k, o.noisepath[0], fs);
            return 2;
        }
        fs = fs_k;
    }
    if (plan_file && !(plan_table = sea_plan_load(plan_file))) {
        fprintf(stderr, "ERROR:   cannot read the plan file %s\n", plan_file);
        return 2;
    }
    printf("read noise\n");
    snprintf(path, sizeof path, "%s%s", o.outputDictionary, o.Log);
    Log = fopen(path, "a+");
    snprintf(path, sizeof path, "%sIRM.sIRM", o.outputDictionary);
    if (mix) fp_irm = fopen(path, "a");
    if (!Log || (mix && !fp_irm)) {
        fprintf(stderr, "ERROR:   cannot open the Log or %s\n", path);
        return 2;
    }
    if (sea_init(-1)) {
        fprintf(stderr, "ERROR:   %s\n", sea_last_error());
        return 1;
    }
    srand(seed);
    /* utterances per library call: host memory holds their outputs, 384 B per sample with the subband sets */
    group = want_sub ? 16 : 256;
    U = (utt_t *)calloc((size_t)group, sizeof *U);
    for (k = 0; k < n_ids; k += group) {
        int n = 0, j, s;
        for (j = k; j < n_ids && j < k + group; j++) {
            utt_t *u = &U[n];
            int why;
            printf("%s\n", ids[j]);
            fprintf(Log, "%s\n ", ids[j]);
            snprintf(path, sizeof path, "%s%s.wav", o.purewavDictionary, ids[j]);
            if (sea_wav_read(path, &u->clean, &u->len, &u->fs)) {
                fprintf(stderr, "ERROR:   cannot read %s\n", path);
                free(u->clean);
                u->clean = NULL;
                rc = 3;
                continue;
            }
            if (u->fs != fs) { /* mixing signals of two rates would go unnoticed in the output */
                fprintf(stderr, "ERROR:   %s is sampled at %d Hz, the noise files at %d Hz: skipped\n", path, u->fs, fs);
                utt_free(u);
                rc = 3;
                continue;
            }
            if (plan_table) {
                if (sea_plan_find(plan_table, ids[j], &u->plan)) {
                    fprintf(stderr, "ERROR:   %s has no plan line for %s\n", plan_file, ids[j]);
                    utt_free(u);
                    rc = 3;
                    continue;
                }
            } else if (fixed) {
                u->plan.rec = 0;
                u->plan.off = 0;
                u->plan.db = o.addnoisedB;
            } else
                sea_plan_draw(noise_len, u->len, &u->plan);
            if ((why = sea_plan_check(&u->plan, noise_len, 4, u->len)) != 0) {
                fprintf(stderr, "ERROR:   %s (%ld samples) skipped: %s\n", ids[j], u->len,
                        why == 1 ? "shorter than one 320-sample frame"
                                 : why == 2 ? "the plan names no noise recording" : "the stretch does not lie inside the noise recording");
                utt_free(u);
                rc = 3;
                continue;
            }
            fprintf(Log, "\n");
            sea_plan_write(Log, ids[j], &u->plan);
            u->id = ids[j];
            u->noisy = (short *)malloc((size_t)u->len * sizeof(short));
            u->irm = (float *)malloc((size_t)((u->len - 320) / 160 + 1) * 64 * sizeof(float));
            for (s = 0; s < 3 && want_sub; s++) u->sub[s] = (short *)malloc((size_t)u->len * 64 * sizeof(short));
            n++;
        }
        if (n && mix) {
            const short **cl = (const short **)malloc((size_t)n * sizeof *cl);
            short **ny = (short **)malloc((size_t)n * sizeof *ny), **sb[3];
            float **im = (float **)malloc((size_t)n * sizeof *im);
            long *len = (long *)malloc((size_t)n * sizeof *len), *off = (long *)malloc((size_t)n * sizeof *off);
            int *rec = (int *)malloc((size_t)n * sizeof *rec), *db = (int *)malloc((size_t)n * sizeof *db);
            for (s = 0; s < 3; s++) sb[s] = (short **)malloc((size_t)n * sizeof **sb);
            for (j = 0; j < n; j++) {
                cl[j] = U[j].clean;
                ny[j] = U[j].noisy;
                im[j] = U[j].irm;
                len[j] = U[j].len;
                rec[j] = U[j].plan.rec;
                off[j] = U[j].plan.off;
                db[j] = U[j].plan.db;
                for (s = 0; s < 3; s++) sb[s][j] = U[j].sub[s];
            }
            if (sea_trainset_utterances(cl, len, n, (const short *const *)noise, noise_len, 4, rec, off, db, 1, ny, im, NULL,
                                        want_sub ? sb[0] : NULL, want_sub ? sb[1] : NULL, want_sub ? sb[2] : NULL)) {
                fprintf(stderr, "ERROR:   %s\n", sea_last_error());
                return 1;
            }
            free(cl), free(ny), free(im), free(len), free(off), free(rec), free(db);
            for (s = 0; s < 3; s++) free(sb[s]);
        }
        for (j = 0; j < n; j++) {
            utt_t *u = &U[j];
            int bad = 0;
            fprintf(Log, mix ? "subband\n single_IBM\n " : "subband\n "); /* once per utterance, as the reference logs them */
            if (!mix) {
                memcpy(u->noisy, u->clean, (size_t)u->len * sizeof(short));
                if (want_sub) {
                    bad |= sea_subband64(u->clean, u->len, u->sub[0]);
                    bad |= sea_subband64(noise[u->plan.rec] + u->plan.off, u->len, u->sub[1]);
                    memcpy(u->sub[2], u->sub[0], (size_t)u->len * 64 * sizeof(short));
                    if (bad) fprintf(stderr, "ERROR:   %s\n", sea_last_error());
                }
            }
            snprintf(path, sizeof path, "%s%s%s_noisy.wav", o.outputDictionary, o.save_noisy_dir, u->id);
            bad |= sea_wav_write(path, u->noisy, u->len, u->fs);
            if (want_sub) {
                bad |= write_subbands(&o, o.save_subband_pure_wav_dir, "", u->id, u->sub[0], u->len, u->fs);
                bad |= write_subbands(&o, o.save_subband_noise_wav_dir, "_noise", u->id, u->sub[1], u->len, u->fs);
                bad |= write_subbands(&o, o.save_subband_noisy_wav_dir, "_noisy", u->id, u->sub[2], u->len, u->fs);
            }
            if (mix) {
                snprintf(path, sizeof path, "%s_noisy", u->id);
                bad |= sea_mask_text_write(fp_irm, path, u->irm, (u->len - 320) / 160 + 1);
            }
            if (bad) {
                fprintf(stderr, "ERROR:   cannot write the outputs of %s\n", u->id);
                rc = 4;
            }
            utt_free(u);
        }
    }
    free(U);
    sea_plan_free(plan_table);
    if (fp_irm) fclose(fp_irm);
    fclose(Log);
    for (k = 0; k < 4; k++) free(noise[k]);
    sea_free_list(ids, n_ids);
    return rc;
}
