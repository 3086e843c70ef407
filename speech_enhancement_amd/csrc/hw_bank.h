/*
 * hw_bank.h -- the two banks of the Hu-Wang chain as the host text of its C ABI sees them (hw_bank_capi.hip, which states every
 * stage once as a function template on a bank; hw25_resynth_capi.hip, hw64_resynth_capi.hip): a traits type per bank, holding
 * what differs between the sea_hw25_* and the sea_hw64_* calls and nothing else, and the two launches of the resynthesis that
 * the resynthesis units share.
 */
#pragma once
#include "hw25_capi.h"

namespace sea_capi {

/* 25 channels at 8 kHz (hw25_*_kernel.hip) */
struct Bank25 {
    static constexpr const char *name = "hw25"; /* the messages' prefix */
    static constexpr int NCHAN = SEA_HW25_NCHAN, HOP = SEA_HW25_HOP, DELAYS = SEA_HW25_DELAYS;
    static constexpr int SCRATCH_WORDS = SEA_HW25_SCRATCH_WORDS, FINAL_SCRATCH_WORDS = SEA_HW25_FINAL_SCRATCH_WORDS;
    static constexpr int AM_SMALL_CHUNK = 5; /* the AM FFT's channels per launch group when all of them do not fit */
    /* the correlogram keeps a frame's ACFs in LDS: about eight workgroups per CU over the batch */
    static constexpr int CORR_PER_CU = 8, CORR_THREADS = 256;
    static constexpr bool PITCH_READS_CROSS = true;
    using Args = sea::Hw25Args;
    using PitchArgs = sea::Hw25PitchArgs;
    using ResynthArgs = sea::Hw25ResynthArgs;
    static const sea_hw25_tables *tables(const DeviceCtx &c) { return c.hw25; }
    static constexpr auto periphery = sea::hw25_periphery_kernel, lowpass = sea::hw25_lowpass_kernel,
                          correlogram = sea::hw25_correlogram_kernel;
    static constexpr auto pitch_max = sea::hw25_pitch_max_kernel, pitch_segment = sea::hw25_pitch_segment_kernel,
                          pitch_frame = sea::hw25_pitch_frame_kernel, pitch_regroup = sea::hw25_pitch_regroup_kernel,
                          pitch_track = sea::hw25_pitch_track_kernel;
    static constexpr auto am_prepare = sea::hw25_am_prepare_kernel, am_patt = sea::hw25_am_patt_kernel,
                          am_fft_head = sea::hw25_am_fft_head_kernel, am_fft_stage = sea::hw25_am_fft_stage_kernel,
                          am_norm = sea::hw25_am_norm_kernel, am_rate = sea::hw25_am_rate_kernel;
    static constexpr auto finalseg = sea::hw25_finalseg_kernel;
    static constexpr auto resynth = sea::hw25_resynth_kernel;
};

/* 64 channels at 16 kHz (hw64_*_kernel.hip) */
struct Bank64 {
    static constexpr const char *name = "hw64";
    static constexpr int NCHAN = SEA_HW64_NCHAN, HOP = SEA_HW64_HOP, DELAYS = SEA_HW64_DELAYS;
    static constexpr int SCRATCH_WORDS = SEA_HW64_SCRATCH_WORDS, FINAL_SCRATCH_WORDS = SEA_HW64_FINAL_SCRATCH_WORDS;
    static constexpr int AM_SMALL_CHUNK = 8;
    /* A workgroup holds 67.6 KB of LDS, so a CU runs two at a time: about four per CU over the batch lets the short utterances'
     * workgroups make room for the long ones'. */
    static constexpr int CORR_PER_CU = 4, CORR_THREADS = sea::kHw64CorrThreads;
    static constexpr bool PITCH_READS_CROSS = false; /* nothing reads the cross array on this bank */
    using Args = sea::Hw64Args;
    using PitchArgs = sea::Hw64PitchArgs;
    using ResynthArgs = sea::Hw64ResynthArgs;
    static const sea_hw64_tables *tables(const DeviceCtx &c) { return c.hw64; }
    static constexpr auto periphery = sea::hw64_periphery_kernel, lowpass = sea::hw64_lowpass_kernel,
                          correlogram = sea::hw64_correlogram_kernel;
    static constexpr auto pitch_max = sea::hw64_pitch_max_kernel, pitch_segment = sea::hw64_pitch_segment_kernel,
                          pitch_frame = sea::hw64_pitch_frame_kernel, pitch_regroup = sea::hw64_pitch_regroup_kernel,
                          pitch_track = sea::hw64_pitch_track_kernel;
    static constexpr auto am_prepare = sea::hw64_am_prepare_kernel, am_patt = sea::hw64_am_patt_kernel,
                          am_fft_head = sea::hw64_am_fft_head_kernel, am_fft_stage = sea::hw64_am_fft_stage_kernel,
                          am_norm = sea::hw64_am_norm_kernel, am_rate = sea::hw64_am_rate_kernel;
    static constexpr auto finalseg = sea::hw64_finalseg_kernel;
    static constexpr auto resynth = sea::hw64_resynth_kernel;
};

/* The batch launches of the resynthesis on device pointers and one stream, defined for both banks in hw_bank_capi.hip:
 * sea_hw25_resynth_batch and sea_hw25_enhance_batch are these on Bank25; on Bank64 they are internal, and the exported calls are
 * the host-pointer forms built on them (sea_hw64_resynth, sea_hw64_enhance, sea_hw64_*_utterances). */
template <class B>
int resynth_launch(const float *d_gout, const float *d_mask, const long long *d_offsets, const long long *d_lengths,
                   const long long *d_row_offsets, float threshold, float *d_out_f32, short *d_out_i16, const int *d_order, int n_utt,
                   hipStream_t stream);
/* the whole estimator, then the resynthesis of its own mask from the gOut it keeps in its scratch */
template <class B>
int enhance_launch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                   float *d_out_f32, short *d_out_i16, float *d_mask, int *d_pitch, int *d_status, void *d_scratch,
                   long long total_padded_samples, long long total_rows, const int *d_order, int n_utt, hipStream_t stream,
                   hipEvent_t before_resynth = nullptr, hipEvent_t after_resynth = nullptr); /* recorded around the resynthesis */

} // namespace sea_capi
