/*
 * hw64_am_capi.hip -- the C ABI of the Hu-Wang estimator's AM labels and final grouping at 16 kHz on the 64-channel bank
 * (hw64_am_kernel.hip): sea_hw64_am_scratch_bytes, sea_hw64_am_batch, sea_hw64_finalseg_scratch_bytes, sea_hw64_finalseg_batch
 * and the whole estimator, sea_hw64_ibm_scratch_bytes, sea_hw64_ibm_batch, sea_hw64_ibm.  It mirrors hw25_am_capi.hip call
 * for call and argument for argument.  The batch calls are launches on one stream and nothing else: the lengths stay on the
 * device.
 */
#include "hw25_capi.h"

using namespace sea_capi;

namespace {

constexpr int kCh = SEA_HW64_NCHAN;

long long pos(long long v) { return v > 0 ? v : 0; }

long long up256(long long v) { return (v + 255) & ~255LL; }

/* The FFT works on `chunk` channels at a time, two complex buffers of 2 x the padded length each, 2048 bytes per padded
 * sample for all 64 channels: all of them while that stays under 256 MiB (131 072 padded samples), else eight launch groups
 * of eight channels. */
int am_chunk(long long total_padded_samples) { return pos(total_padded_samples) * 2 * kCh * 16 <= (256LL << 20) ? kCh : 8; }

/* the AM scratch: info [n_utt] ints | ampatt | am (hout's layout, used when the caller passes none) | fa | fb */
struct AmLayout {
    long long info, ampatt, am, fa, fb, end;
};
AmLayout am_layout(long long total, int n_utt)
{
    total = pos(total);
    const long long plane = up256(total * kCh * 4 + 64), fft = up256(total * 2 * am_chunk(total) * 8 + 64);
    AmLayout l;
    l.info = 0;
    l.ampatt = up256(4LL * pos(n_utt));
    l.am = l.ampatt + plane;
    l.fa = l.am + plane;
    l.fb = l.fa + fft;
    l.end = l.fb + fft;
    return l;
}

int am_launch(sea::Hw25AmArgs a, long long total, hipStream_t stream)
{
    const int n_utt = a.n_utt;
    const dim3 b64(64), b256(256);
    hipLaunchKernelGGL(sea::hw64_am_prepare_kernel, dim3(n_utt), b64, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sea::hw64_am_patt_kernel, dim3(n_utt, SEA_HW25_AM_PATT_GRID, kCh), b256, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.chunk = am_chunk(total);
    for (a.chan0 = 0; a.chan0 < kCh; a.chan0 += a.chunk) {
        const dim3 grid(n_utt, SEA_HW25_AM_FFT_GRID, a.chunk);
        for (a.inverse = 0; a.inverse < 2; ++a.inverse) {
            hipLaunchKernelGGL(sea::hw64_am_fft_head_kernel, grid, b256, 0, stream, a);
            HIP_TRY(hipGetLastError());
            /* the lengths are not known here: every stage up to the largest N is launched, and the workgroups of an
             * utterance whose N is smaller leave at once */
            for (a.stage = SEA_HW25_AM_LDS_LOG2 + 1; a.stage <= SEA_HW25_MAXLOG2; ++a.stage) {
                hipLaunchKernelGGL(sea::hw64_am_fft_stage_kernel, grid, b256, 0, stream, a);
                HIP_TRY(hipGetLastError());
            }
        }
        a.inverse = 0;
        hipLaunchKernelGGL(sea::hw64_am_norm_kernel, grid, b256, 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::hw64_am_rate_kernel, dim3(n_utt, SEA_HW25_AM_RATE_GRID), b64, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
             const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
             int *d_status, int status_or, void *d_scratch, long long total, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_gout || !d_pitch || !d_offsets || !d_lengths || !d_row_offsets || !d_amcrn || !d_status || !d_scratch)
        return fail("hw64_am: null pointer (only d_ratio, d_seng, d_ampatt, d_am and d_order may be null)");
    if (total <= 0) return fail("hw64_am: total_padded_samples=%lld", total);
    const void *outs[] = {d_amcrn, d_ratio, d_seng, d_ampatt, d_am, d_status};
    if (shared_buffer(outs, 6, {d_gout, d_pitch})) return fail("hw64_am: an output must not be an input or another output");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const AmLayout l = am_layout(total, n_utt);
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
    a.tables = c->hw25; /* am_a and am_beta: kaiserPara (0.01, ..) knows neither rate nor bank */
    a.tw = reinterpret_cast<const float2 *>(c->hw25_tw);
    a.n_utt = n_utt;
    return am_launch(a, total, (hipStream_t)stream);
}

int finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                   const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final, int *d_status,
                   int status_or, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_grp || !d_amcrn || !d_cross_ev || !d_pratio || !d_lengths || !d_row_offsets || !d_mask || !d_status || !d_scratch)
        return fail("hw64_finalseg: null pointer (only d_grp_final, d_stages and d_order may be null)");
    const void *outs[] = {d_mask, d_grp_final, d_stages, d_status};
    if (shared_buffer(outs, 4, {d_grp, d_amcrn, d_cross_ev, d_pratio}))
        return fail("hw64_finalseg: an output must not be an input or another output");
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
    hipLaunchKernelGGL(sea::hw64_finalseg_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* the whole estimator's scratch: hout | hev | gout | acf_hc | six frame planes (cross_hc, cross_ev, pratio_in, mark, grp,
 * pratio) | amcrn | the three stages' own scratch */
struct IbmLayout {
    long long hout, hev, gout, acf, fr, plane, amcrn, pitch, am, fin, end;
};
IbmLayout ibm_layout(long long total, long long rows, int n_utt)
{
    total = pos(total);
    rows = pos(rows) + 1;
    const long long stream = up256(total * kCh * 4 + 64);
    IbmLayout l;
    l.plane = up256(rows * kCh * 4);
    l.hout = 0;
    l.hev = stream;
    l.gout = 2 * stream;
    l.acf = 3 * stream;
    l.fr = l.acf + up256(rows * kCh * SEA_HW64_DELAYS * 4);
    l.amcrn = l.fr + 6 * l.plane;
    l.pitch = l.amcrn + l.plane;
    l.am = l.pitch + up256(sea_hw64_pitch_scratch_bytes(rows, n_utt));
    l.fin = l.am + up256(sea_hw64_am_scratch_bytes(total, n_utt));
    l.end = l.fin + up256(sea_hw64_finalseg_scratch_bytes(rows, n_utt));
    return l;
}

} // namespace

long long sea_hw64_am_scratch_bytes(long long total_padded_samples, int n_utt) { return am_layout(total_padded_samples, n_utt).end; }

int sea_hw64_am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
                      const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
                      int *d_status, void *d_scratch, long long total_padded_samples, const int *d_order, int n_utt, void *stream)
{
    return am_batch(d_gout, d_pitch, d_offsets, d_lengths, d_row_offsets, d_amcrn, d_ratio, d_seng, d_ampatt, d_am, d_status, 0,
                    d_scratch, total_padded_samples, d_order, n_utt, stream);
}

long long sea_hw64_finalseg_scratch_bytes(long long total_rows, int n_utt)
{
    (void)n_utt;
    return 4 * pos(total_rows) * SEA_HW64_FINAL_SCRATCH_WORDS + 64;
}

int sea_hw64_finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final,
                            int *d_status, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    return finalseg_batch(d_grp, d_amcrn, d_cross_ev, d_pratio, d_lengths, d_row_offsets, d_mask, d_grp_final, d_status, 0, d_stages,
                          d_scratch, d_order, n_utt, stream);
}

long long sea_hw64_ibm_scratch_bytes(long long total_padded_samples, long long total_rows, int n_utt)
{
    return ibm_layout(total_padded_samples, total_rows, n_utt).end;
}

long long sea_capi::hw64_ibm_gout_offset(long long total_padded_samples, long long total_rows, int n_utt)
{
    return ibm_layout(total_padded_samples, total_rows, n_utt).gout;
}

int sea_hw64_ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                       float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
                       long long total_rows, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_in_f32 || !d_offsets || !d_lengths || !d_row_offsets || !d_mask || !d_pitch || !d_status || !d_scratch)
        return fail("hw64_ibm: null pointer (only d_stages and d_order may be null)");
    const void *outs[] = {d_mask, d_pitch, d_status, d_stages};
    if (shared_buffer(outs, 4, {d_in_f32})) return fail("hw64_ibm: an output must not be the input or another output");
    if (total_padded_samples <= 0) return fail("hw64_ibm: total_padded_samples=%lld", total_padded_samples);
    const IbmLayout l = ibm_layout(total_padded_samples, total_rows, n_utt);
    char *scr = static_cast<char *>(d_scratch);
    auto f32 = [&](long long at) { return reinterpret_cast<float *>(scr + at); };
    float *hout = f32(l.hout), *hev = f32(l.hev), *gout = f32(l.gout), *acf = f32(l.acf);
    float *cross_hc = f32(l.fr), *cross_ev = f32(l.fr + l.plane), *pratio_in = f32(l.fr + 2 * l.plane), *mark = f32(l.fr + 3 * l.plane);
    float *grp = f32(l.fr + 4 * l.plane), *pratio = f32(l.fr + 5 * l.plane), *amcrn = f32(l.amcrn);
    /* globalPitch's Pitch goes to d_pitch first; pitchDtm's replaces it */
    if (sea_hw64_periphery_batch(d_in_f32, hout, hev, gout, d_offsets, d_lengths, d_order, n_utt, stream)) return 1;
    if (sea_hw64_correlogram_batch(hout, hev, d_offsets, d_lengths, d_row_offsets, acf, nullptr, cross_hc, cross_ev, d_pitch, pratio_in,
                                   mark, nullptr, d_order, n_utt, stream))
        return 1;
    if (sea_hw64_pitch_batch(acf, pratio_in, mark, d_lengths, d_row_offsets, d_pitch, grp, pratio, d_status, nullptr, scr + l.pitch,
                             d_order, n_utt, stream))
        return 1;
    if (am_batch(gout, d_pitch, d_offsets, d_lengths, d_row_offsets, amcrn, nullptr, nullptr, nullptr, nullptr, d_status, 1,
                 scr + l.am, total_padded_samples, d_order, n_utt, stream))
        return 1;
    return finalseg_batch(grp, amcrn, cross_ev, pratio, d_lengths, d_row_offsets, d_mask, nullptr, d_status, 1, d_stages, scr + l.fin,
                          d_order, n_utt, stream);
}

int sea_hw64_ibm(const float *x, long L, float *mask, int *pitch, int *status)
{
    if (L < 0) return fail("hw64_ibm: L=%ld", L);
    if (!status || (L > 0 && !x)) return fail("hw64_ibm: null pointer");
    if (L == 0) { /* no frame: nothing to compute, as a zero-length utterance of the batch form */
        *status = 0;
        return 0;
    }
    Hw25Single u;
    if (u.load(x, L, SEA_HW64_HOP)) return 1;
    const long long rows = u.rows;
    DevBuf<float> dmask;
    DevBuf<int> dint;
    DevBuf<char> dscr;
    HIP_TRY(dmask.alloc((size_t)rows * kCh));
    HIP_TRY(dint.alloc((size_t)rows + 1)); /* pitch | status */
    HIP_TRY(dscr.alloc((size_t)sea_hw64_ibm_scratch_bytes(u.Lp, rows, 1)));
    if (sea_hw64_ibm_batch(u.d_in, u.d_offsets, u.d_lengths, u.d_row_offsets, dmask.p, dint.p, dint.p + rows, nullptr, dscr.p, u.Lp,
                           rows, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(status, dint.p + rows, sizeof(int), hipMemcpyDeviceToHost));
    return u.rows_back(mask, dmask.p, kCh) || u.rows_back(pitch, dint.p, 1);
}
