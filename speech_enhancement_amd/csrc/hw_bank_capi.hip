/*
 * hw_bank_capi.hip -- the C ABI of the Hu-Wang chain on both banks, 25 channels at 8 kHz (sea_hw25_*) and 64 at 16 kHz
 * (sea_hw64_*): the front half (periphery, correlogram), initial grouping and pitch tracking, AM labels and final grouping, the
 * whole estimator and the two launches of the resynthesis.  Every stage is stated once as a function template on a bank
 * (hw_bank.h), and the exported calls at the end are forwards onto it.  The batch calls are launches on one stream and nothing
 * else: the lengths stay on the device.  Every refusal comes before anything touches a device: the null pointers first, then
 * every output against every input and every other output (the kernels read inputs after they have begun to write outputs).
 */
#include "hw_bank.h"

using namespace sea_capi;

namespace {

long long pos(long long v) { return v > 0 ? v : 0; }
long long up256(long long v) { return (v + 255) & ~255LL; }

/* ---- the front half: periphery and correlogram ----------------------------------------------------------------------------- */
template <class B>
int periphery(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
              const long long *d_lengths, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_in_f32 || !d_hout || !d_hev || !d_offsets || !d_lengths) return fail("%s_periphery: null pointer", B::name);
    const void *const outs[] = {d_hout, d_hev, d_gout};
    if (shared_buffer(outs, 3, {d_in_f32, d_offsets, d_lengths, d_order}))
        return fail("%s_periphery: every output must be a buffer of its own", B::name);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    typename B::Args a{};
    a.tables = B::tables(*c);
    a.n_utt = n_utt;
    a.in = d_in_f32;
    a.hout = d_hout;
    a.hev = d_hev;
    a.gout = d_gout;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    hipLaunchKernelGGL(B::periphery, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(B::lowpass, dim3(n_utt, B::NCHAN), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class B>
int correlogram(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc, float *d_cross_ev, int *d_pitch,
                float *d_pratio, float *d_mark, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_hout || !d_hev || !d_offsets || !d_lengths || !d_row_offsets || !d_cross_hc || !d_cross_ev || !d_pitch || !d_pratio ||
        !d_mark)
        return fail("%s_correlogram: null pointer (only d_acf_hc, d_acf_ev, d_scratch and d_order may be null)", B::name);
    const void *const outs[] = {d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev, d_pitch, d_pratio, d_mark};
    if (shared_buffer(outs, 7, {d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_correlogram: every output must be a buffer of its own", B::name);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    typename B::Args a{};
    a.tables = B::tables(*c);
    a.n_utt = n_utt;
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
    /* B::CORR_PER_CU workgroups per CU over the batch: per_utterance (capi.hip) deals eight, and ceil (8 n_cu / k n_utt) is
     * ceil ((8 / k) n_cu / n_utt) */
    static_assert(8 % B::CORR_PER_CU == 0);
    const int per_utt = per_utterance(n_utt * (8 / B::CORR_PER_CU));
    if (per_utt < 1) return 1;
    hipLaunchKernelGGL(B::correlogram, dim3(n_utt, per_utt), dim3(B::CORR_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class B>
int frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets, const long long *d_lengths,
                   const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc, float *d_cross_ev,
                   int *d_pitch, float *d_pratio, float *d_mark, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    /* refuse what the second call would refuse before the first one launches anything */
    if (!d_in_f32 || !d_hout || !d_hev || !d_offsets || !d_lengths || !d_row_offsets || !d_cross_hc || !d_cross_ev || !d_pitch ||
        !d_pratio || !d_mark)
        return fail("%s_frontend: null pointer (only d_acf_hc, d_acf_ev, d_scratch and d_order may be null)", B::name);
    const void *const outs[] = {d_hout, d_hev, d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev, d_pitch, d_pratio, d_mark};
    if (shared_buffer(outs, 9, {d_in_f32, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_frontend: every output must be a buffer of its own", B::name);
    if (periphery<B>(d_in_f32, d_hout, d_hev, nullptr, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    return correlogram<B>(d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev, d_pitch,
                          d_pratio, d_mark, d_order, n_utt, stream);
}

template <class B>
int frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc, float *cross_ev,
             int *pitch, float *pratio, float *mark)
{
    if (!in) return fail("%s_frontend: null input", B::name);
    if (L <= 0) return fail("%s_frontend: L=%ld", B::name, L);
    Hw25Single u;
    if (u.load(in, L, B::HOP)) return 1;
    const size_t Lp = (size_t)u.Lp, fr = (size_t)u.rows * B::NCHAN, acf = (size_t)B::NCHAN * B::DELAYS;
    DevBuf<float> dho, dhe, dah, dae, dfr;
    DevBuf<int> dp;
    HIP_TRY(dho.alloc(Lp * B::NCHAN));
    HIP_TRY(dhe.alloc(Lp * B::NCHAN));
    if (acf_hc) HIP_TRY(dah.alloc(fr * B::DELAYS));
    if (acf_ev) HIP_TRY(dae.alloc(fr * B::DELAYS));
    HIP_TRY(dfr.alloc(fr * 4)); /* cross_hc | cross_ev | pratio | mark */
    HIP_TRY(dp.alloc((size_t)u.rows));
    if (frontend_batch<B>(u.d_in, dho.p, dhe.p, u.d_offsets, u.d_lengths, u.d_row_offsets, dah.p, dae.p, dfr.p, dfr.p + fr, dp.p,
                          dfr.p + 2 * fr, dfr.p + 3 * fr, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    const size_t rowb = (size_t)L * sizeof(float);
    if (hout) HIP_TRY(hipMemcpy2D(hout, rowb, dho.p, Lp * sizeof(float), rowb, B::NCHAN, hipMemcpyDeviceToHost));
    if (hev) HIP_TRY(hipMemcpy2D(hev, rowb, dhe.p, Lp * sizeof(float), rowb, B::NCHAN, hipMemcpyDeviceToHost));
    return u.rows_back(acf_hc, dah.p, acf) || u.rows_back(acf_ev, dae.p, acf) || u.rows_back(cross_hc, dfr.p, B::NCHAN) ||
           u.rows_back(cross_ev, dfr.p + fr, B::NCHAN) || u.rows_back(pratio, dfr.p + 2 * fr, B::NCHAN) ||
           u.rows_back(mark, dfr.p + 3 * fr, B::NCHAN) || u.rows_back(pitch, dp.p, 1);
}

/* ---- initial grouping and pitch tracking ----------------------------------------------------------------------------------- */
/* the scratch: segse [n_utt][2][400] ints first (its size needs n_utt alone), then B::SCRATCH_WORDS words per row; utterance
 * u's block starts at its first row, so the batch call needs no row total */
long long segse_words(int n_utt) { return pos(n_utt) * 2 * SEA_HW25_MAX_SEGMENTS; }

template <class B>
long long pitch_scratch_bytes(long long total_rows, int n_utt)
{
    return 4 * (segse_words(n_utt) + pos(total_rows) * B::SCRATCH_WORDS);
}

template <class B>
int pitch_launch(typename B::PitchArgs a, int n_utt, hipStream_t stream)
{
    const int waves = per_utterance(n_utt); /* eight waves per CU over the batch */
    if (waves < 1) return 1;
    const dim3 per_frame(n_utt, waves), one_wave(n_utt), block(64);
    hipLaunchKernelGGL(B::pitch_max, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(B::pitch_segment, one_wave, block, 0, stream, a); /* initGroup */
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_FIND | SEA_HW25_FRAME_TIMECRN; /* findPitch, timeCrn */
    a.stage = 0;
    hipLaunchKernelGGL(B::pitch_frame, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.theta = 0.95f; /* reGroup (THETAP): the double constant converted to the float parameter */
    a.stage = 1;
    hipLaunchKernelGGL(B::pitch_regroup, one_wave, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_FIND; /* findPitch */
    hipLaunchKernelGGL(B::pitch_frame, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(B::pitch_track, one_wave, block, 0, stream, a); /* checkPitch .. linearEstimate */
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_TIMECRN; /* timeCrn */
    hipLaunchKernelGGL(B::pitch_frame, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.theta = 0.85f; /* reGroup (THETAT) */
    a.stage = -1;
    hipLaunchKernelGGL(B::pitch_regroup, one_wave, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* d_cross_hc: required and read where B::PITCH_READS_CROSS only */
template <class B>
int pitch_batch(const float *d_acf_hc, const float *d_cross_hc, const float *d_pratio_in, const float *d_mark_in,
                const long long *d_lengths, const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio, int *d_status,
                void *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_acf_hc || (B::PITCH_READS_CROSS && !d_cross_hc) || !d_pratio_in || !d_mark_in || !d_lengths || !d_row_offsets || !d_pitch ||
        !d_grp || !d_pratio || !d_status || !d_scratch)
        return fail("%s_pitch: null pointer (only d_stages and d_order may be null)", B::name);
    const void *const outs[] = {d_pitch, d_grp, d_pratio, d_status, d_stages, d_scratch};
    if (shared_buffer(outs, 6, {d_acf_hc, d_cross_hc, d_pratio_in, d_mark_in, d_lengths, d_row_offsets, d_order}))
        return fail("%s_pitch: every output must be a buffer of its own", B::name);
    typename B::PitchArgs a{};
    a.acf = d_acf_hc;
    if constexpr (B::PITCH_READS_CROSS) a.cross = d_cross_hc;
    a.pratio_in = d_pratio_in;
    a.mark_in = d_mark_in;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.pitch = d_pitch;
    a.grp = d_grp;
    a.pratio = d_pratio;
    a.status = d_status;
    a.stages = static_cast<int *>(d_stages);
    a.segse = static_cast<int *>(d_scratch);
    a.rowscr = a.segse + segse_words(n_utt);
    a.order = d_order;
    a.n_utt = n_utt;
    return pitch_launch<B>(a, n_utt, (hipStream_t)stream);
}

template <class B>
int pitch_utterance(const float *x, long L, int *pitch, float *grp, float *pratio, int *status)
{
    if (L <= 0) return fail("%s_pitch: L=%ld", B::name, L);
    if (!x || !status) return fail("%s_pitch: null pointer", B::name);
    Hw25Single u;
    if (u.load(x, L, B::HOP)) return 1;
    const long long rows = u.rows;
    const size_t fr = (size_t)rows * B::NCHAN;
    DevBuf<float> dho, dhe, dah, dfr;
    DevBuf<int> dp, dint;
    DevBuf<char> dscr;
    HIP_TRY(dho.alloc((size_t)u.Lp * B::NCHAN));
    HIP_TRY(dhe.alloc((size_t)u.Lp * B::NCHAN));
    HIP_TRY(dah.alloc(fr * B::DELAYS));
    HIP_TRY(dfr.alloc(fr * 6)); /* cross_hc | cross_ev | pratio_in | mark | grp | pratio */
    HIP_TRY(dp.alloc((size_t)rows));
    HIP_TRY(dint.alloc((size_t)rows + 1)); /* pitch | status */
    HIP_TRY(dscr.alloc((size_t)pitch_scratch_bytes<B>(rows, 1)));
    if (frontend_batch<B>(u.d_in, dho.p, dhe.p, u.d_offsets, u.d_lengths, u.d_row_offsets, dah.p, nullptr, dfr.p, dfr.p + fr, dp.p,
                          dfr.p + 2 * fr, dfr.p + 3 * fr, nullptr, 1, nullptr))
        return 1;
    if (pitch_batch<B>(dah.p, dfr.p, dfr.p + 2 * fr, dfr.p + 3 * fr, u.d_lengths, u.d_row_offsets, dint.p, dfr.p + 4 * fr,
                       dfr.p + 5 * fr, dint.p + rows, nullptr, dscr.p, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(status, dint.p + rows, sizeof(int), hipMemcpyDeviceToHost));
    return u.rows_back(pitch, dint.p, 1) || u.rows_back(grp, dfr.p + 4 * fr, B::NCHAN) ||
           u.rows_back(pratio, dfr.p + 5 * fr, B::NCHAN);
}

/* ---- AM labels and final grouping ------------------------------------------------------------------------------------------ */
/* The FFT works on `chunk` channels at a time, two complex buffers of 2 x the padded length each: all of the bank's channels
 * while that stays under 256 MiB (335 544 padded samples at 25 channels, 131 072 at 64), else launch groups of
 * B::AM_SMALL_CHUNK channels. */
template <class B>
int am_chunk(long long total_padded_samples)
{
    return pos(total_padded_samples) * 2 * B::NCHAN * 16 <= (256LL << 20) ? B::NCHAN : B::AM_SMALL_CHUNK;
}

/* the AM scratch: info [n_utt] ints | ampatt | am (hout's layout, used when the caller passes none) | fa | fb */
struct AmLayout {
    long long info, ampatt, am, fa, fb, end;
};
template <class B>
AmLayout am_layout(long long total, int n_utt)
{
    total = pos(total);
    const long long plane = up256(total * B::NCHAN * 4 + 64), fft = up256(total * 2 * am_chunk<B>(total) * 8 + 64);
    AmLayout l;
    l.info = 0;
    l.ampatt = up256(4LL * pos(n_utt));
    l.am = l.ampatt + plane;
    l.fa = l.am + plane;
    l.fb = l.fa + fft;
    l.end = l.fb + fft;
    return l;
}

template <class B>
int am_launch(sea::Hw25AmArgs a, long long total, hipStream_t stream)
{
    const int n_utt = a.n_utt;
    const dim3 b64(64), b256(256);
    hipLaunchKernelGGL(B::am_prepare, dim3(n_utt), b64, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(B::am_patt, dim3(n_utt, SEA_HW25_AM_PATT_GRID, B::NCHAN), b256, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.chunk = am_chunk<B>(total);
    for (a.chan0 = 0; a.chan0 < B::NCHAN; a.chan0 += a.chunk) {
        const dim3 grid(n_utt, SEA_HW25_AM_FFT_GRID, a.chunk);
        for (a.inverse = 0; a.inverse < 2; ++a.inverse) {
            hipLaunchKernelGGL(B::am_fft_head, grid, b256, 0, stream, a);
            HIP_TRY(hipGetLastError());
            /* the lengths are not known here: every stage up to the largest N is launched, and the workgroups of an
             * utterance whose N is smaller leave at once */
            for (a.stage = SEA_HW25_AM_LDS_LOG2 + 1; a.stage <= SEA_HW25_MAXLOG2; ++a.stage) {
                hipLaunchKernelGGL(B::am_fft_stage, grid, b256, 0, stream, a);
                HIP_TRY(hipGetLastError());
            }
        }
        a.inverse = 0;
        hipLaunchKernelGGL(B::am_norm, grid, b256, 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(B::am_rate, dim3(n_utt, SEA_HW25_AM_RATE_GRID), b64, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class B>
int am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
             const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
             int *d_status, int status_or, void *d_scratch, long long total, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_gout || !d_pitch || !d_offsets || !d_lengths || !d_row_offsets || !d_amcrn || !d_status || !d_scratch)
        return fail("%s_am: null pointer (only d_ratio, d_seng, d_ampatt, d_am and d_order may be null)", B::name);
    if (total <= 0) return fail("%s_am: total_padded_samples=%lld", B::name, total);
    const void *const outs[] = {d_amcrn, d_ratio, d_seng, d_ampatt, d_am, d_status, d_scratch};
    if (shared_buffer(outs, 7, {d_gout, d_pitch, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_am: an output must not be an input or another output", B::name);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const AmLayout l = am_layout<B>(total, n_utt);
    char *scr = static_cast<char *>(d_scratch);
    sea::Hw25AmArgs a{};
    a.gout = d_gout;
    a.pitch = d_pitch;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.amcrn = d_amcrn;
    a.ratio = d_ratio;
    a.seng = d_seng;
    a.ampatt = d_ampatt ? d_ampatt : reinterpret_cast<float *>(scr + l.ampatt);
    a.am = d_am ? d_am : reinterpret_cast<float *>(scr + l.am);
    a.fa = reinterpret_cast<float2 *>(scr + l.fa);
    a.fb = reinterpret_cast<float2 *>(scr + l.fb);
    a.info = reinterpret_cast<int *>(scr + l.info);
    a.status = d_status;
    a.status_or = status_or;
    a.order = d_order;
    a.tables = c->hw25; /* on both banks: am_a and am_beta, kaiserPara (0.01, ..), know neither rate nor bank */
    a.tw = reinterpret_cast<const float2 *>(c->hw25_tw);
    a.n_utt = n_utt;
    return am_launch<B>(a, total, (hipStream_t)stream);
}

template <class B>
long long finalseg_scratch_bytes(long long total_rows, int /* n_utt: the rows alone decide */)
{
    return 4 * pos(total_rows) * B::FINAL_SCRATCH_WORDS + 64;
}

template <class B>
int finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                   const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final, int *d_status,
                   int status_or, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_grp || !d_amcrn || !d_cross_ev || !d_pratio || !d_lengths || !d_row_offsets || !d_mask || !d_status || !d_scratch)
        return fail("%s_finalseg: null pointer (only d_grp_final, d_stages and d_order may be null)", B::name);
    const void *const outs[] = {d_mask, d_grp_final, d_stages, d_status, d_scratch};
    if (shared_buffer(outs, 5, {d_grp, d_amcrn, d_cross_ev, d_pratio, d_lengths, d_row_offsets, d_order}))
        return fail("%s_finalseg: an output must not be an input or another output", B::name);
    sea::Hw25FinalArgs a{};
    a.grp = d_grp;
    a.amcrn = d_amcrn;
    a.cross_ev = d_cross_ev;
    a.pratio = d_pratio;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.mask = d_mask;
    a.grp_final = d_grp_final;
    a.stages = d_stages;
    a.status = d_status;
    a.status_or = status_or;
    a.rowscr = static_cast<int *>(d_scratch);
    a.order = d_order;
    a.n_utt = n_utt;
    hipLaunchKernelGGL(B::finalseg, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- the whole estimator --------------------------------------------------------------------------------------------------- */
/* its scratch: hout | hev | gout | acf_hc | six frame planes (cross_hc, cross_ev, pratio_in, mark, grp, pratio) | amcrn | the
 * three stages' own scratch; enhance_launch resynthesises from gout */
struct IbmLayout {
    long long hout, hev, gout, acf, fr, plane, amcrn, pitch, am, fin, end;
};
template <class B>
IbmLayout ibm_layout(long long total, long long rows, int n_utt)
{
    total = pos(total);
    rows = pos(rows) + 1;
    const long long stream = up256(total * B::NCHAN * 4 + 64);
    IbmLayout l;
    l.plane = up256(rows * B::NCHAN * 4);
    l.hout = 0;
    l.hev = stream;
    l.gout = 2 * stream;
    l.acf = 3 * stream;
    l.fr = l.acf + up256(rows * B::NCHAN * B::DELAYS * 4);
    l.amcrn = l.fr + 6 * l.plane;
    l.pitch = l.amcrn + l.plane;
    l.am = l.pitch + up256(pitch_scratch_bytes<B>(rows, n_utt));
    l.fin = l.am + up256(am_layout<B>(total, n_utt).end);
    l.end = l.fin + up256(finalseg_scratch_bytes<B>(rows, n_utt));
    return l;
}

template <class B>
int ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
              float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
              long long total_rows, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_in_f32 || !d_offsets || !d_lengths || !d_row_offsets || !d_mask || !d_pitch || !d_status || !d_scratch)
        return fail("%s_ibm: null pointer (only d_stages and d_order may be null)", B::name);
    const void *const outs[] = {d_mask, d_pitch, d_status, d_stages, d_scratch};
    if (shared_buffer(outs, 5, {d_in_f32, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_ibm: an output must not be the input or another output", B::name);
    if (total_padded_samples <= 0) return fail("%s_ibm: total_padded_samples=%lld", B::name, total_padded_samples);
    const IbmLayout l = ibm_layout<B>(total_padded_samples, total_rows, n_utt);
    char *scr = static_cast<char *>(d_scratch);
    auto f32 = [&](long long at) { return reinterpret_cast<float *>(scr + at); };
    float *hout = f32(l.hout), *hev = f32(l.hev), *gout = f32(l.gout), *acf = f32(l.acf);
    float *cross_hc = f32(l.fr), *cross_ev = f32(l.fr + l.plane), *pratio_in = f32(l.fr + 2 * l.plane), *mark = f32(l.fr + 3 * l.plane);
    float *grp = f32(l.fr + 4 * l.plane), *pratio = f32(l.fr + 5 * l.plane), *amcrn = f32(l.amcrn);
    /* globalPitch's Pitch goes to d_pitch first; pitchDtm's replaces it */
    if (periphery<B>(d_in_f32, hout, hev, gout, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    if (correlogram<B>(hout, hev, d_offsets, d_lengths, d_row_offsets, acf, nullptr, cross_hc, cross_ev, d_pitch, pratio_in, mark,
                       d_order, n_utt, stream))
        return 1;
    if (pitch_batch<B>(acf, cross_hc, pratio_in, mark, d_lengths, d_row_offsets, d_pitch, grp, pratio, d_status, nullptr,
                       scr + l.pitch, d_order, n_utt, stream))
        return 1;
    if (am_batch<B>(gout, d_pitch, d_offsets, d_lengths, d_row_offsets, amcrn, nullptr, nullptr, nullptr, nullptr, d_status, 1,
                    scr + l.am, total_padded_samples, d_order, n_utt, stream))
        return 1;
    return finalseg_batch<B>(grp, amcrn, cross_ev, pratio, d_lengths, d_row_offsets, d_mask, nullptr, d_status, 1, d_stages,
                             scr + l.fin, d_order, n_utt, stream);
}

template <class B>
int ibm(const float *x, long L, float *mask, int *pitch, int *status)
{
    if (L < 0) return fail("%s_ibm: L=%ld", B::name, L);
    if (!status || (L > 0 && !x)) return fail("%s_ibm: null pointer", B::name);
    if (L == 0) { /* no frame: nothing to compute, as a zero-length utterance of the batch form */
        *status = 0;
        return 0;
    }
    Hw25Single u;
    if (u.load(x, L, B::HOP)) return 1;
    const long long rows = u.rows;
    DevBuf<float> dmask;
    DevBuf<int> dint;
    DevBuf<char> dscr;
    HIP_TRY(dmask.alloc((size_t)rows * B::NCHAN));
    HIP_TRY(dint.alloc((size_t)rows + 1)); /* pitch | status */
    HIP_TRY(dscr.alloc((size_t)ibm_layout<B>(u.Lp, rows, 1).end));
    if (ibm_batch<B>(u.d_in, u.d_offsets, u.d_lengths, u.d_row_offsets, dmask.p, dint.p, dint.p + rows, nullptr, dscr.p, u.Lp, rows,
                     nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(status, dint.p + rows, sizeof(int), hipMemcpyDeviceToHost));
    return u.rows_back(mask, dmask.p, B::NCHAN) || u.rows_back(pitch, dint.p, 1);
}

} // namespace

/* ---- the resynthesis launches (hw_bank.h) ---------------------------------------------------------------------------------- */
template <class B>
int sea_capi::resynth_launch(const float *d_gout, const float *d_mask, const long long *d_offsets, const long long *d_lengths,
                             const long long *d_row_offsets, float threshold, float *d_out_f32, short *d_out_i16, const int *d_order,
                             int n_utt, hipStream_t stream)
{
    if (n_utt <= 0) return 0;
    if (!d_gout || !d_mask || !d_offsets || !d_lengths || !d_row_offsets)
        return fail("%s_resynth: null pointer (only d_order and one output may be null)", B::name);
    if (!d_out_f32 && !d_out_i16) return fail("%s_resynth: no output (d_out_f32 and d_out_i16 are both null)", B::name);
    const void *const outs[] = {d_out_f32, d_out_i16};
    if (shared_buffer(outs, 2, {d_gout, d_mask, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_resynth: an output must not be an input or the other output", B::name);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    typename B::ResynthArgs a{};
    a.gout = d_gout;
    a.mask = d_mask;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.out_f32 = d_out_f32;
    a.out_i16 = d_out_i16;
    a.order = d_order;
    a.tables = B::tables(*c);
    a.threshold = threshold;
    a.n_utt = n_utt;
    hipLaunchKernelGGL(B::resynth, dim3(n_utt), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class B>
int sea_capi::enhance_launch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths,
                             const long long *d_row_offsets, float *d_out_f32, short *d_out_i16, float *d_mask, int *d_pitch,
                             int *d_status, void *d_scratch, long long total_padded_samples, long long total_rows, const int *d_order,
                             int n_utt, hipStream_t stream, hipEvent_t before_resynth, hipEvent_t after_resynth)
{
    if (n_utt <= 0) return 0;
    if (!d_in_f32 || !d_offsets || !d_lengths || !d_row_offsets || !d_mask || !d_pitch || !d_status || !d_scratch)
        return fail("%s_enhance: null pointer (only d_order and one output may be null)", B::name);
    if (!d_out_f32 && !d_out_i16) return fail("%s_enhance: no output (d_out_f32 and d_out_i16 are both null)", B::name);
    const void *const outs[] = {d_out_f32, d_out_i16, d_mask, d_pitch, d_status, d_scratch};
    if (shared_buffer(outs, 6, {d_in_f32, d_offsets, d_lengths, d_row_offsets, d_order}))
        return fail("%s_enhance: an output must not be the input or another output", B::name);
    /* the mask of createIBM :99-106 is 0 / 1: the reference's `mark > 0` */
    if (ibm_batch<B>(d_in_f32, d_offsets, d_lengths, d_row_offsets, d_mask, d_pitch, d_status, nullptr, d_scratch,
                     total_padded_samples, total_rows, d_order, n_utt, stream))
        return 1;
    const float *gout = reinterpret_cast<const float *>(static_cast<const char *>(d_scratch) +
                                                        ibm_layout<B>(total_padded_samples, total_rows, n_utt).gout);
    if (before_resynth) HIP_TRY(hipEventRecord(before_resynth, stream));
    if (resynth_launch<B>(gout, d_mask, d_offsets, d_lengths, d_row_offsets, 0.0f, d_out_f32, d_out_i16, d_order, n_utt, stream))
        return 1;
    if (after_resynth) HIP_TRY(hipEventRecord(after_resynth, stream));
    return 0;
}

/* for sea_hw25_resynth_batch and sea_hw25_enhance_batch (hw25_resynth_capi.hip) and the list forms of hw64_resynth_capi.hip */
template int sea_capi::resynth_launch<Bank25>(const float *, const float *, const long long *, const long long *, const long long *,
                                              float, float *, short *, const int *, int, hipStream_t);
template int sea_capi::resynth_launch<Bank64>(const float *, const float *, const long long *, const long long *, const long long *,
                                              float, float *, short *, const int *, int, hipStream_t);
template int sea_capi::enhance_launch<Bank25>(const float *, const long long *, const long long *, const long long *, float *, short *,
                                              float *, int *, int *, void *, long long, long long, const int *, int, hipStream_t,
                                              hipEvent_t, hipEvent_t);
template int sea_capi::enhance_launch<Bank64>(const float *, const long long *, const long long *, const long long *, float *, short *,
                                              float *, int *, int *, void *, long long, long long, const int *, int, hipStream_t,
                                              hipEvent_t, hipEvent_t);

/* ---- the exported calls (include/sea_mi355x.h): each is its stage above on its bank ---------------------------------------- */
int sea_hw25_tables_host(float *cf25, float *bw25, float *midEar25, float *gain25, float *f1_25, float *f2_25, int *winsize25,
                         float *lp91, float *hair10)
{
    sea_hw25_plain_tables(cf25, bw25, midEar25, gain25, f1_25, f2_25, winsize25, lp91, hair10);
    return 0;
}

int sea_hw64_tables_host(float *cf64, float *bw64, float *midEar64, float *gain64, float *f1_64, float *f2_64, int *winsize64,
                         float *lp181, float *hair10)
{
    sea_hw64_plain_tables(cf64, bw64, midEar64, gain64, f1_64, f2_64, winsize64, lp181, hair10);
    return 0;
}

int sea_hw25_am_tables_host(float *a_beta2, int *n_at_pow2_11, float *twiddles, int n_twiddles)
{
    static const int at_pow2[11] = SEA_HW25_N_AT_POW2;
    sea_hw25_tables t;
    sea_build_hw25_tables(&t);
    if (a_beta2) {
        a_beta2[0] = t.am_a;
        a_beta2[1] = t.am_beta;
    }
    if (n_at_pow2_11)
        for (int i = 0; i < 11; ++i) n_at_pow2_11[i] = at_pow2[i];
    if (twiddles) {
        if (n_twiddles != SEA_HW25_TWIDDLES) return fail("hw25_am_tables: n_twiddles=%d, not %d", n_twiddles, SEA_HW25_TWIDDLES);
        sea_build_hw25_twiddles(twiddles, 1);
    }
    return 0;
}

long long sea_hw25_frames(long long length) { return length > 0 ? length / Bank25::HOP : 0; }
long long sea_hw64_frames(long long length) { return length > 0 ? length / Bank64::HOP : 0; }

/* the correlogram keeps a frame's ACFs in LDS: this form needs no scratch */
long long sea_hw25_scratch_bytes(long long total_padded_samples, int n_utt)
{
    (void)total_padded_samples;
    (void)n_utt;
    return 0;
}

int sea_hw64_workgroups_per_utterance(int n_utt) { return per_utterance(n_utt * (8 / Bank64::CORR_PER_CU)); }
int sea_hw64_pitch_waves_per_utterance(int n_utt) { return per_utterance(n_utt); }

int sea_hw25_periphery_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int n_utt, void *stream)
{
    return periphery<Bank25>(d_in_f32, d_hout, d_hev, nullptr, d_offsets, d_lengths, d_order, n_utt, stream);
}

int sea_hw25_periphery_gout_batch(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int n_utt, void *stream)
{
    return periphery<Bank25>(d_in_f32, d_hout, d_hev, d_gout, d_offsets, d_lengths, d_order, n_utt, stream);
}

int sea_hw64_periphery_batch(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int n_utt, void *stream)
{
    return periphery<Bank64>(d_in_f32, d_hout, d_hev, d_gout, d_offsets, d_lengths, d_order, n_utt, stream);
}

/* d_scratch: neither bank's correlogram needs any; the argument stays in the calls and is not looked at */
int sea_hw25_correlogram_batch(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                               const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc,
                               float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                               const int *d_order, int n_utt, void *stream)
{
    return correlogram<Bank25>(d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev,
                               d_pitch, d_pratio, d_mark, d_order, n_utt, stream);
}

int sea_hw64_correlogram_batch(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                               const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc,
                               float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                               const int *d_order, int n_utt, void *stream)
{
    return correlogram<Bank64>(d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc, d_cross_ev,
                               d_pitch, d_pratio, d_mark, d_order, n_utt, stream);
}

int sea_hw25_frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev,
                            float *d_cross_hc, float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                            const int *d_order, int n_utt, void *stream)
{
    return frontend_batch<Bank25>(d_in_f32, d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc,
                                  d_cross_ev, d_pitch, d_pratio, d_mark, d_order, n_utt, stream);
}

int sea_hw64_frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev,
                            float *d_cross_hc, float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                            const int *d_order, int n_utt, void *stream)
{
    return frontend_batch<Bank64>(d_in_f32, d_hout, d_hev, d_offsets, d_lengths, d_row_offsets, d_acf_hc, d_acf_ev, d_cross_hc,
                                  d_cross_ev, d_pitch, d_pratio, d_mark, d_order, n_utt, stream);
}

int sea_hw25_frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc,
                      float *cross_ev, int *pitch, float *pratio, float *mark)
{
    return frontend<Bank25>(in, L, hout, hev, acf_hc, acf_ev, cross_hc, cross_ev, pitch, pratio, mark);
}

int sea_hw64_frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc,
                      float *cross_ev, int *pitch, float *pratio, float *mark)
{
    return frontend<Bank64>(in, L, hout, hev, acf_hc, acf_ev, cross_hc, cross_ev, pitch, pratio, mark);
}

long long sea_hw25_pitch_scratch_bytes(long long total_rows, int n_utt) { return pitch_scratch_bytes<Bank25>(total_rows, n_utt); }
long long sea_hw64_pitch_scratch_bytes(long long total_rows, int n_utt) { return pitch_scratch_bytes<Bank64>(total_rows, n_utt); }

int sea_hw25_pitch_batch(const float *d_acf_hc, const float *d_cross_hc, const float *d_pratio_in, const float *d_mark_in,
                         const long long *d_lengths, const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio,
                         int *d_status, void *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    return pitch_batch<Bank25>(d_acf_hc, d_cross_hc, d_pratio_in, d_mark_in, d_lengths, d_row_offsets, d_pitch, d_grp, d_pratio,
                               d_status, d_stages, d_scratch, d_order, n_utt, stream);
}

int sea_hw64_pitch_batch(const float *d_acf_hc, const float *d_pratio_in, const float *d_mark_in, const long long *d_lengths,
                         const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio, int *d_status, void *d_stages,
                         void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    return pitch_batch<Bank64>(d_acf_hc, nullptr, d_pratio_in, d_mark_in, d_lengths, d_row_offsets, d_pitch, d_grp, d_pratio,
                               d_status, d_stages, d_scratch, d_order, n_utt, stream);
}

int sea_hw25_pitch(const float *x, long L, int *pitch, float *grp, float *pratio, int *status)
{
    return pitch_utterance<Bank25>(x, L, pitch, grp, pratio, status);
}

int sea_hw64_pitch(const float *x, long L, int *pitch, float *grp, float *pratio, int *status)
{
    return pitch_utterance<Bank64>(x, L, pitch, grp, pratio, status);
}

long long sea_hw25_am_scratch_bytes(long long total_padded_samples, int n_utt) { return am_layout<Bank25>(total_padded_samples, n_utt).end; }
long long sea_hw64_am_scratch_bytes(long long total_padded_samples, int n_utt) { return am_layout<Bank64>(total_padded_samples, n_utt).end; }

int sea_hw25_am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
                      const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
                      int *d_status, void *d_scratch, long long total_padded_samples, const int *d_order, int n_utt, void *stream)
{
    return am_batch<Bank25>(d_gout, d_pitch, d_offsets, d_lengths, d_row_offsets, d_amcrn, d_ratio, d_seng, d_ampatt, d_am, d_status,
                            0, d_scratch, total_padded_samples, d_order, n_utt, stream);
}

int sea_hw64_am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
                      const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
                      int *d_status, void *d_scratch, long long total_padded_samples, const int *d_order, int n_utt, void *stream)
{
    return am_batch<Bank64>(d_gout, d_pitch, d_offsets, d_lengths, d_row_offsets, d_amcrn, d_ratio, d_seng, d_ampatt, d_am, d_status,
                            0, d_scratch, total_padded_samples, d_order, n_utt, stream);
}

long long sea_hw25_finalseg_scratch_bytes(long long total_rows, int n_utt) { return finalseg_scratch_bytes<Bank25>(total_rows, n_utt); }
long long sea_hw64_finalseg_scratch_bytes(long long total_rows, int n_utt) { return finalseg_scratch_bytes<Bank64>(total_rows, n_utt); }

int sea_hw25_finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final,
                            int *d_status, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    return finalseg_batch<Bank25>(d_grp, d_amcrn, d_cross_ev, d_pratio, d_lengths, d_row_offsets, d_mask, d_grp_final, d_status, 0,
                                  d_stages, d_scratch, d_order, n_utt, stream);
}

int sea_hw64_finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final,
                            int *d_status, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    return finalseg_batch<Bank64>(d_grp, d_amcrn, d_cross_ev, d_pratio, d_lengths, d_row_offsets, d_mask, d_grp_final, d_status, 0,
                                  d_stages, d_scratch, d_order, n_utt, stream);
}

long long sea_hw25_ibm_scratch_bytes(long long total_padded_samples, long long total_rows, int n_utt)
{
    return ibm_layout<Bank25>(total_padded_samples, total_rows, n_utt).end;
}

long long sea_hw64_ibm_scratch_bytes(long long total_padded_samples, long long total_rows, int n_utt)
{
    return ibm_layout<Bank64>(total_padded_samples, total_rows, n_utt).end;
}

int sea_hw25_ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                       float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
                       long long total_rows, const int *d_order, int n_utt, void *stream)
{
    return ibm_batch<Bank25>(d_in_f32, d_offsets, d_lengths, d_row_offsets, d_mask, d_pitch, d_status, d_stages, d_scratch,
                             total_padded_samples, total_rows, d_order, n_utt, stream);
}

int sea_hw64_ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                       float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
                       long long total_rows, const int *d_order, int n_utt, void *stream)
{
    return ibm_batch<Bank64>(d_in_f32, d_offsets, d_lengths, d_row_offsets, d_mask, d_pitch, d_status, d_stages, d_scratch,
                             total_padded_samples, total_rows, d_order, n_utt, stream);
}

int sea_hw25_ibm(const float *x, long L, float *mask, int *pitch, int *status) { return ibm<Bank25>(x, L, mask, pitch, status); }
int sea_hw64_ibm(const float *x, long L, float *mask, int *pitch, int *status) { return ibm<Bank64>(x, L, mask, pitch, status); }
