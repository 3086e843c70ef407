/*
 * hw64_capi.hip -- the C ABI of the Hu-Wang estimator's front half at 16 kHz on the 64-channel bank (hw64_kernel.hip): the
 * sea_hw64_* calls of include/sea_mi355x.h.  They mirror the sea_hw25_* front-half calls of capi.hip argument for argument.
 */
#include "hw25_capi.h"

using namespace sea_capi;

int sea_hw64_tables_host(float *cf64, float *bw64, float *midEar64, float *gain64, float *f1_64, float *f2_64, int *winsize64,
                         float *lp181, float *hair10)
{
    sea_hw64_plain_tables(cf64, bw64, midEar64, gain64, f1_64, f2_64, winsize64, lp181, hair10);
    return 0;
}

long long sea_hw64_frames(long long length) { return length > 0 ? length / SEA_HW64_HOP : 0; }

/* A workgroup holds 67.6 KB of LDS, so a CU runs two at a time: about four per CU over the batch lets the short utterances'
 * workgroups make room for the long ones'.  The lengths stay on the device, so the number is the same for every utterance. */
int sea_hw64_workgroups_per_utterance(int n_utt)
{
    DeviceCtx *c;
    if (n_utt <= 0 || ctx(&c)) return 0;
    const int per_utt = (4 * c->n_cu + n_utt - 1) / n_utt;
    return per_utt < 1 ? 1 : (per_utt > 1024 ? 1024 : per_utt);
}

static int hw64_args(sea::Hw64Args &a, int n_utt)
{
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    a = sea::Hw64Args{};
    a.tables = c->hw64;
    a.n_utt = n_utt;
    return 0;
}

int sea_hw64_periphery_batch(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_in_f32 || !d_hout || !d_hev || !d_offsets || !d_lengths) return fail("hw64_periphery: null pointer");
    const void *const outs[] = {d_hout, d_hev, d_gout};
    if (shared_buffer(outs, 3, {d_in_f32, d_offsets, d_lengths, d_order}))
        return fail("hw64_periphery: every output must be a buffer of its own");
    sea::Hw64Args a;
    if (hw64_args(a, n_utt)) return 1;
    a.in = d_in_f32;
    a.hout = d_hout;
    a.hev = d_hev;
    a.gout = d_gout;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    hipLaunchKernelGGL(sea::hw64_periphery_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sea::hw64_lowpass_kernel, dim3(n_utt, SEA_HW64_NCHAN), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_hw64_correlogram_batch(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                               const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc,
                               float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                               const int *d_order, int n_utt, void *stream)
{
    (void)d_scratch; /* this form needs none: the argument keeps the call in step with sea_hw25_correlogram_batch */
    if (n_utt <= 0) return 0;
    if (!d_hout || !d_hev || !d_offsets || !d_lengths || !d_row_offsets || !d_cross_hc || !d_cross_ev || !d_pitch || !d_pratio ||
        !d_mark)
        return fail("hw64_correlogram: null pointer (only d_acf_hc, d_acf_ev, d_scratch and d_order may be null)");
    const void *const outs[] = {d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev, d_pitch, d_pratio, d_mark};
    if (shared_buffer(outs, 7, {d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("hw64_correlogram: every output must be a buffer of its own");
    sea::Hw64Args a;
    if (hw64_args(a, n_utt)) return 1;
    a.hout = const_cast<float *>(d_hout);
    a.hev = const_cast<float *>(d_hev);
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.acf_hc = d_acf_hc;
    a.acf_ev = d_acf_ev;
    a.cross_hc = d_cross_hc;
    a.cross_ev = d_cross_ev;
    a.pitch = d_pitch;
    a.pratio = d_pratio;
    a.mark = d_mark;
    a.order = d_order;
    /* the lengths stay on the device: a fixed number of workgroups per utterance walks its frames; the utterances go on grid
     * x (y ends at 65535) */
    const int per_utt = sea_hw64_workgroups_per_utterance(n_utt);
    if (per_utt < 1) return 1;
    hipLaunchKernelGGL(sea::hw64_correlogram_kernel, dim3(n_utt, per_utt), dim3(sea::kHw64CorrThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_hw64_frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev,
                            float *d_cross_hc, float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                            const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    /* refuse what the second call would refuse before the first one launches anything */
    if (!d_row_offsets || !d_cross_hc || !d_cross_ev || !d_pitch || !d_pratio || !d_mark)
        return fail("hw64_frontend: null pointer (only d_acf_hc, d_acf_ev, d_scratch and d_order may be null)");
    const void *const outs[] = {d_hout, d_hev, d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev, d_pitch, d_pratio, d_mark};
    if (shared_buffer(outs, 9, {d_in_f32, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("hw64_frontend: every output must be a buffer of its own");
    if (sea_hw64_periphery_batch(d_in_f32, d_hout, d_hev, nullptr, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    return sea_hw64_correlogram_batch(d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc,
                                      d_cross_ev, d_pitch, d_pratio, d_mark, d_scratch, d_order, n_utt, stream);
}

int sea_hw64_frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc,
                      float *cross_ev, int *pitch, float *pratio, float *mark)
{
    if (!in) return fail("hw64_frontend: null input");
    if (L <= 0) return fail("hw64_frontend: L=%ld", L);
    Hw25Single u;
    if (u.load(in, L, SEA_HW64_HOP)) return 1;
    const size_t Lp = (size_t)u.Lp, fr = (size_t)u.rows * SEA_HW64_NCHAN, acf = (size_t)SEA_HW64_NCHAN * SEA_HW64_DELAYS;
    DevBuf<float> dho, dhe, dah, dae, dfr;
    DevBuf<int> dp;
    HIP_TRY(dho.alloc(Lp * SEA_HW64_NCHAN));
    HIP_TRY(dhe.alloc(Lp * SEA_HW64_NCHAN));
    if (acf_hc) HIP_TRY(dah.alloc(fr * SEA_HW64_DELAYS));
    if (acf_ev) HIP_TRY(dae.alloc(fr * SEA_HW64_DELAYS));
    HIP_TRY(dfr.alloc(fr * 4)); /* cross_hc | cross_ev | pratio | mark */
    HIP_TRY(dp.alloc((size_t)u.rows));
    if (sea_hw64_frontend_batch(u.d_in, dho.p, dhe.p, u.d_offsets, u.d_lengths, u.d_row_offsets, dah.p, dae.p, dfr.p, dfr.p + fr,
                                dp.p, dfr.p + 2 * fr, dfr.p + 3 * fr, nullptr, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    const size_t rowb = (size_t)L * sizeof(float);
    if (hout) HIP_TRY(hipMemcpy2D(hout, rowb, dho.p, Lp * sizeof(float), rowb, SEA_HW64_NCHAN, hipMemcpyDeviceToHost));
    if (hev) HIP_TRY(hipMemcpy2D(hev, rowb, dhe.p, Lp * sizeof(float), rowb, SEA_HW64_NCHAN, hipMemcpyDeviceToHost));
    return u.rows_back(acf_hc, dah.p, acf) || u.rows_back(acf_ev, dae.p, acf) || u.rows_back(cross_hc, dfr.p, SEA_HW64_NCHAN) ||
           u.rows_back(cross_ev, dfr.p + fr, SEA_HW64_NCHAN) || u.rows_back(pratio, dfr.p + 2 * fr, SEA_HW64_NCHAN) ||
           u.rows_back(mark, dfr.p + 3 * fr, SEA_HW64_NCHAN) || u.rows_back(pitch, dp.p, 1);
}
