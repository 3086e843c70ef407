/*
 * hw25_resynth_capi.hip -- the C ABI of the Hu-Wang 25-channel resynthesis (hw25_resynth_kernel.hip):
 * sea_hw25_resynth_tables_host, sea_hw25_resynth_batch, sea_hw25_enhance_batch (the whole estimator followed by the
 * resynthesis of its own mask), the single-utterance forms sea_hw25_resynth and sea_hw25_enhance, and the text writer.  The
 * batch calls are the shared launches of hw_bank.h on this bank: launches on one stream, the lengths stay on the device.
 */
#include <cstdio>

#include "hw_bank.h"

using namespace sea_capi;

int sea_hw25_resynth_tables_host(float *w640, double *up80, double *down120)
{
    sea_hw25_ola_tables(w640, up80, down120);
    return 0;
}

int sea_hw25_resynth_batch(const float *d_gout, const float *d_mask, const long long *d_offsets, const long long *d_lengths,
                           const long long *d_row_offsets, float threshold, float *d_out_f32, short *d_out_i16, const int *d_order,
                           int n_utt, void *stream)
{
    return resynth_launch<Bank25>(d_gout, d_mask, d_offsets, d_lengths, d_row_offsets, threshold, d_out_f32, d_out_i16, d_order, n_utt,
                                  (hipStream_t)stream);
}

int sea_hw25_enhance_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                           float *d_out_f32, short *d_out_i16, float *d_mask, int *d_pitch, int *d_status, void *d_scratch,
                           long long total_padded_samples, long long total_rows, const int *d_order, int n_utt, void *stream)
{
    return enhance_launch<Bank25>(d_in_f32, d_offsets, d_lengths, d_row_offsets, d_out_f32, d_out_i16, d_mask, d_pitch, d_status,
                                  d_scratch, total_padded_samples, total_rows, d_order, n_utt, (hipStream_t)stream);
}

int sea_hw25_resynth(const float *x, long L, const float *mask, long F, float threshold, float *out_f32)
{
    if (L < 0) return fail("hw25_resynth: L=%ld", L);
    if (L == 0) return 0;
    if (!x || !out_f32) return fail("hw25_resynth: null pointer");
    if (F != (long)sea_hw25_frames(L)) return fail("hw25_resynth: F=%ld, not L / 80 = %lld", F, sea_hw25_frames(L));
    if (F > 0 && !mask) return fail("hw25_resynth: null pointer");
    Hw25Single u;
    if (u.load(x, L)) return 1;
    const size_t plane = (size_t)u.Lp * SEA_HW25_NCHAN, units = (size_t)u.rows * SEA_HW25_NCHAN;
    DevBuf<float> dstreams, dmask, dout;
    HIP_TRY(dstreams.alloc(plane * 3)); /* hout | hev | gout */
    HIP_TRY(dmask.alloc(units));
    HIP_TRY(dout.alloc((size_t)u.Lp));
    HIP_TRY(hipMemset(dmask.p, 0, units * sizeof(float)));
    if (F > 0) HIP_TRY(hipMemcpy(dmask.p, mask, (size_t)F * SEA_HW25_NCHAN * sizeof(float), hipMemcpyHostToDevice));
    if (sea_hw25_periphery_gout_batch(u.d_in, dstreams.p, dstreams.p + plane, dstreams.p + 2 * plane, u.d_offsets, u.d_lengths, nullptr,
                                      1, nullptr))
        return 1;
    if (sea_hw25_resynth_batch(dstreams.p + 2 * plane, dmask.p, u.d_offsets, u.d_lengths, u.d_row_offsets, threshold, dout.p, nullptr,
                               nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_f32, dout.p, (size_t)L * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_hw25_enhance(const float *x, long L, float *out_f32, float *mask, int *pitch, int *status)
{
    if (L < 0) return fail("hw25_enhance: L=%ld", L);
    if (!status || (L > 0 && (!x || !out_f32))) return fail("hw25_enhance: null pointer");
    if (L == 0) { /* no sample: nothing to compute */
        *status = 0;
        return 0;
    }
    Hw25Single u;
    if (u.load(x, L)) return 1;
    const long long rows = u.rows;
    DevBuf<float> dmask, dout;
    DevBuf<int> dint;
    DevBuf<char> dscr;
    HIP_TRY(dout.alloc((size_t)u.Lp));
    HIP_TRY(dmask.alloc((size_t)rows * SEA_HW25_NCHAN));
    HIP_TRY(dint.alloc((size_t)rows + 1)); /* pitch | status */
    HIP_TRY(dscr.alloc((size_t)sea_hw25_ibm_scratch_bytes(u.Lp, rows, 1)));
    if (sea_hw25_enhance_batch(u.d_in, u.d_offsets, u.d_lengths, u.d_row_offsets, dout.p, nullptr, dmask.p, dint.p, dint.p + rows, dscr.p,
                               u.Lp, rows, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(status, dint.p + rows, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_f32, dout.p, (size_t)L * sizeof(float), hipMemcpyDeviceToHost));
    return u.rows_back(mask, dmask.p, SEA_HW25_NCHAN) || u.rows_back(pitch, dint.p, 1);
}

int sea_hw25_resynth_text_write(const char *path, const float *out, long L)
{
    if (!path || L < 0 || (L > 0 && !out)) return fail("hw25_resynth_text_write: bad argument");
    FILE *fp = fopen(path, "w");
    if (!fp) return fail("hw25_resynth_text_write: cannot open %s", path);
    bool ok = true;
    for (long n = 0; n < L; n++) ok = fprintf(fp, "%f\n", out[n]) > 0 && ok; /* resynthesis:1543-1544 */
    ok = fclose(fp) == 0 && ok;
    return ok ? 0 : fail("hw25_resynth_text_write: writing %s failed", path);
}
