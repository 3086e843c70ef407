/*
 * hw64_pitch_capi.hip -- the C ABI of the Hu-Wang estimator's initial grouping and pitch tracking at 16 kHz on the 64-channel
 * bank (hw64_pitch_kernel.hip): sea_hw64_pitch_scratch_bytes, sea_hw64_pitch_waves_per_utterance, sea_hw64_pitch_batch,
 * sea_hw64_pitch.  The batch call is eight launches on one stream and nothing else: the lengths stay on the device.  It mirrors
 * hw25_pitch_capi.hip without the cross array, which nothing reads on this bank.
 */
#include "hw25_capi.h"

using namespace sea_capi;

/* the scratch: segse [n_utt][2][400] ints first (its size needs n_utt alone), then SEA_HW64_SCRATCH_WORDS words per row;
 * utterance u's block starts at its first row, so the batch call needs no row total */
static long long segse_words(int n_utt) { return (long long)(n_utt > 0 ? n_utt : 0) * 2 * SEA_HW25_MAX_SEGMENTS; }

long long sea_hw64_pitch_scratch_bytes(long long total_rows, int n_utt)
{
    return 4 * (segse_words(n_utt) + (total_rows > 0 ? total_rows : 0) * SEA_HW64_SCRATCH_WORDS);
}

/* The frame kernels (hw64_pitch_max_kernel, hw64_pitch_frame_kernel): a fixed number of waves per utterance walks its frames,
 * about eight waves per CU over the batch (the utterances go on grid x).  The lengths stay on the device, so the number is the
 * same for every utterance. */
int sea_hw64_pitch_waves_per_utterance(int n_utt)
{
    DeviceCtx *c;
    if (n_utt <= 0 || ctx(&c)) return 0;
    const int waves = (8 * c->n_cu + n_utt - 1) / n_utt;
    return waves < 1 ? 1 : (waves > 1024 ? 1024 : waves);
}

static int pitch_launch(sea::Hw64PitchArgs a, int n_utt, hipStream_t stream)
{
    const int waves = sea_hw64_pitch_waves_per_utterance(n_utt);
    if (waves < 1) return 1;
    const dim3 per_frame(n_utt, waves), one_wave(n_utt), block(64);
    hipLaunchKernelGGL(sea::hw64_pitch_max_kernel, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sea::hw64_pitch_segment_kernel, one_wave, block, 0, stream, a); /* initGroup */
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_FIND | SEA_HW25_FRAME_TIMECRN; /* findPitch, timeCrn */
    a.stage = 0;
    hipLaunchKernelGGL(sea::hw64_pitch_frame_kernel, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.theta = 0.95f; /* reGroup (THETAP): the double constant converted to the float parameter */
    a.stage = 1;
    hipLaunchKernelGGL(sea::hw64_pitch_regroup_kernel, one_wave, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_FIND; /* findPitch */
    hipLaunchKernelGGL(sea::hw64_pitch_frame_kernel, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sea::hw64_pitch_track_kernel, one_wave, block, 0, stream, a); /* checkPitch .. linearEstimate */
    HIP_TRY(hipGetLastError());
    a.mode = SEA_HW25_FRAME_TIMECRN; /* timeCrn */
    hipLaunchKernelGGL(sea::hw64_pitch_frame_kernel, per_frame, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    a.theta = 0.85f; /* reGroup (THETAT) */
    a.stage = -1;
    hipLaunchKernelGGL(sea::hw64_pitch_regroup_kernel, one_wave, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_hw64_pitch_batch(const float *d_acf_hc, const float *d_pratio_in, const float *d_mark_in, const long long *d_lengths,
                         const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio, int *d_status, void *d_stages,
                         void *d_scratch, const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_acf_hc || !d_pratio_in || !d_mark_in || !d_lengths || !d_row_offsets || !d_pitch || !d_grp || !d_pratio || !d_status ||
        !d_scratch)
        return fail("hw64_pitch: null pointer (only d_stages and d_order may be null)");
    /* the kernels read the inputs after they have begun to write the outputs: no output may be an input or another output */
    const void *const outs[] = {d_pitch, d_grp, d_pratio, d_status, d_stages, d_scratch};
    if (shared_buffer(outs, 6, {d_acf_hc, d_pratio_in, d_mark_in, d_lengths, d_row_offsets, d_order}))
        return fail("hw64_pitch: every output must be a buffer of its own");
    sea::Hw64PitchArgs a{};
    a.acf = d_acf_hc;
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
    return pitch_launch(a, n_utt, (hipStream_t)stream);
}

int sea_hw64_pitch(const float *x, long L, int *pitch, float *grp, float *pratio, int *status)
{
    if (L <= 0) return fail("hw64_pitch: L=%ld", L);
    if (!x || !status) return fail("hw64_pitch: null pointer");
    Hw25Single u;
    if (u.load(x, L, SEA_HW64_HOP)) return 1;
    const long long rows = u.rows;
    const size_t fr = (size_t)rows * SEA_HW64_NCHAN;
    DevBuf<float> dho, dhe, dah, dfr;
    DevBuf<int> dp, dint;
    DevBuf<char> dscr;
    HIP_TRY(dho.alloc((size_t)u.Lp * SEA_HW64_NCHAN));
    HIP_TRY(dhe.alloc((size_t)u.Lp * SEA_HW64_NCHAN));
    HIP_TRY(dah.alloc(fr * SEA_HW64_DELAYS));
    HIP_TRY(dfr.alloc(fr * 6)); /* cross_hc | cross_ev | pratio_in | mark | grp | pratio */
    HIP_TRY(dp.alloc((size_t)rows));
    HIP_TRY(dint.alloc((size_t)rows + 1)); /* pitch | status */
    HIP_TRY(dscr.alloc((size_t)sea_hw64_pitch_scratch_bytes(rows, 1)));
    if (sea_hw64_frontend_batch(u.d_in, dho.p, dhe.p, u.d_offsets, u.d_lengths, u.d_row_offsets, dah.p, nullptr, dfr.p, dfr.p + fr,
                                dp.p, dfr.p + 2 * fr, dfr.p + 3 * fr, nullptr, nullptr, 1, nullptr))
        return 1;
    if (sea_hw64_pitch_batch(dah.p, dfr.p + 2 * fr, dfr.p + 3 * fr, u.d_lengths, u.d_row_offsets, dint.p, dfr.p + 4 * fr,
                             dfr.p + 5 * fr, dint.p + rows, nullptr, dscr.p, nullptr, 1, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(status, dint.p + rows, sizeof(int), hipMemcpyDeviceToHost));
    return u.rows_back(pitch, dint.p, 1) || u.rows_back(grp, dfr.p + 4 * fr, SEA_HW64_NCHAN) ||
           u.rows_back(pratio, dfr.p + 5 * fr, SEA_HW64_NCHAN);
}
