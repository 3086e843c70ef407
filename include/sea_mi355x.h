/*
 * sea_mi355x.h -- C ABI of libsea_mi355x.so, the MI355X (gfx950) engine for the per-frame
 * noise-suppression hot path of guokiddo1/speech_enhancement.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Three groups of entry points:
 *
 *  (1) DROP-INS with the reference's own names and signatures, so the reference's callers link
 *      against this library unchanged (host buffers in, host buffers out; the library does the
 *      H2D/D2H itself):
 *          etsi_denoise*            etsi/cpp/AdvFrontEnd.h:13-17  (AdvFrontEnd.c:125-329)
 *          rfft                     etsi/cpp/rfft.h:19            (rfft.c:45-180)
 *  (2) HANDLE-BASED equivalents of the FEParamsX plug-in slots (etsi/cpp/ParmInterface.h:120-178;
 *      wired in etsi/cpp/ParmInterface.c:58-82).  INTEGRATION.md shows the 4-line shims that
 *      install them into the reference's vtable:
 *          sea_ns_stream_*          DoNoiseSupAlloc/Init/DoNoiseSup/Delete  (NoiseSup.c:859-1440)
 *          sea_compceps_frame       DoCompCeps                              (CompCeps.c:309-318)
 *          sea_gammatone_filter     gammaToneFilter   resyth_64sub_ori/cpp/HuWang.h:49
 *          sea_resynth64            resynth()         resyth_64sub_ori/cpp/extractwav.h:4
 *                                                     (C form: the reference's takes asdk::CWave)
 *  (3) BATCH entry points on DEVICE pointers (HBM-resident data, caller's HIP stream): what the
 *      reference's only parallel harness -- a thread pool over files,
 *      function/20141106_speech_enhancement/aurora_speech_enhancement/aurora_speech_enhancement.cpp:82-230
 *      -- becomes on a GPU: one launch over a packed batch of utterances.
 *
 * Return convention follows the reference (AdvFrontEnd.c:205-209): 0 (FALSE) = success, non-zero
 * = fault; sea_last_error() describes the most recent fault on the calling thread.
 * There is NO CPU fallback: without a usable gfx950 device every call fails.
 */
#ifndef SEA_MI355X_H
#define SEA_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------------------------
 * (1) drop-ins
 * -------------------------------------------------------------------------------------------- */
/* etsi/cpp/AdvFrontEnd.h:13 -- 8 kHz-mode two-stage Wiener denoiser on i_frame samples.
 * p_denoised[0 .. 80*(i_frame/80)) is written (first 320 samples after the first non-zero frame
 * are 0: SURVEY F7/F8); the trailing i_frame%80 samples are left untouched, as in the reference. */
int etsi_denoise(short *p_data, short *p_denoised, long i_frame);
/* etsi/cpp/AdvFrontEnd.h:14 -- reference behaviour kept: runs etsi_denoise into a scratch buffer
 * and copies only on fault, i.e. never writes p_denoised on success. */
int etsi_denoise_synchronization(short *p_data, short *p_denoised, long i_frame);
/* etsi/cpp/AdvFrontEnd.h:16 -- the reference's 16 kHz-mode entry point reads 80 shorts past a heap
 * buffer per frame and nothing calls it; exported so callers link, it returns 1 (fault)
 * without touching p_denoised. */
int etsi_denoise_16k(short *p_data, short *p_denoised, long i_frame);
/* etsi/cpp/AdvFrontEnd.h:17 -- AdvFrontEnd.c:316-329 calls the 8 kHz-mode etsi_denoise (not the _16k one): the same
 * behaviour as etsi_denoise_synchronization, returns 0 and never writes p_denoised on success. */
int etsi_denoise_16k_synchronization(short *p_data, short *p_denoised, long i_frame);
/* etsi/cpp/rfft.h:19 -- in-place real split-radix FFT, output Re(0..n/2), Im(n/2-1..1), for every size the
 * reference's routine takes (etsi/cpp/rfft.c:45-180): n a power of two (here up to 16384) and any order m with
 * 2^m <= n -- incl. the 16 k-native variant's rfft (x, 512, 8), order 8 on length 512.  A size the routine cannot
 * take (or a missing device) leaves x untouched, prints the reason to stderr and sets sea_last_error(); nothing
 * abort()s the caller. */
void rfft(float *x, int n, int m);

/* ----------------------------------------------------------------------------------------------
 * library state
 * -------------------------------------------------------------------------------------------- */
int sea_init(int device);            /* device < 0: keep the current HIP device; >= 0: make it the calling thread's device */
int sea_device_count(void);          /* usable HIP devices (0 when there is none); one host thread per device is the
                                      * multi-GPU model: utterances are independent, nothing crosses between devices */
const char *sea_last_error(void);
const char *sea_version(void);
/* Device-resident constant tables, for callers that want to inspect them (tests). */
int sea_tables_host(float *sigWindow200, float *irWindow17, float *idct25x25, int *melStart25,
                    int *melLen25, float *melData25x16, float *hamming100, float *dct12x23,
                    int *ccStart23, int *ccLen23, float *ccData23x32);
int sea_gammatone_channels(float *cf64, float *bw64, float *midEar64);

/* ----------------------------------------------------------------------------------------------
 * (3) batch entry points, device pointers.  `stream` is a hipStream_t (NULL = default stream).
 * Utterance u occupies samples [offsets[u], offsets[u]+lengths[u]) of d_in / d_out / d_out_f32;
 * offsets must be multiples of 8 samples.
 * -------------------------------------------------------------------------------------------- */
/* NoiseSup over a batch (etsi_denoise semantics per utterance).
 *   d_out_f32    optional: float NoiseSup output (pre-cast), same indexing as d_out
 *   d_order      optional: launch order (utterance indices, longest first balances the tail; with more than one utterance per
 *                CU the kernels also set their issue priority from the frames each utterance has left relative to the FIRST
 *                utterance of this order, so that the utterances sharing a CU finish together -- results do not depend on it)
 *   d_first_out  optional: per utterance, frame index of the first output frame, -1 if none */
int sea_ns_denoise_batch(const short *d_in, short *d_out, float *d_out_f32,
                         const long long *d_offsets, const long long *d_lengths, const int *d_order,
                         int *d_first_out, int n_utt, void *stream);
/* rfft on [nframes][256] floats (d_out may equal d_in) */
int sea_rfft256_batch(const float *d_in, float *d_out, long long nframes, void *stream);
/* rfft (x, n, m) in place on [nframes][n] floats, any size the reference's routine takes (see rfft above); (256, 8)
 * goes to the streaming kernel, every other size to a one-workgroup-per-frame schedule walker */
int sea_rfft_batch(float *d_x, int n, int m, long long nframes, void *stream);
/* DoCompCeps on [nframes][201] floats (Data[-1..199]) -> [nframes][14] = c1..c12, c0, logE */
int sea_compceps_frames(const float *d_data201, float *d_coef14, long long nframes, void *stream);
/* CompCeps straight from the float NoiseSup stream of sea_ns_denoise_batch.  d_ceps_cum holds
 * n_utt+1 prefix sums of per-utterance capacities (>= lengths/80 - 6 each); cepstral frame j of
 * utterance u lands at d_ceps[(d_ceps_cum[u] + j) * 14]; d_n_ceps[u] receives the valid count and the rows behind
 * it up to the capacity are zeroed.  An utterance whose capacity is 0 owns no tile: its count is NOT written (zero-fill
 * d_n_ceps, as the Python layer does). */
int sea_compceps_batch(const float *d_den_f32, const long long *d_offsets, const long long *d_lengths,
                       const int *d_first_out, const long long *d_ceps_cum, long long total_frames,
                       float *d_ceps, int *d_n_ceps, int n_utt, void *stream);
/* sea_ns_denoise_batch picks one of several forms of the same kernel by batch size (all bit-identical):
 * 3 = six waves per utterance (up to 3 utterances per CU: shortest frame period), 6 = the same compiled so that four
 * workgroups co-reside on a CU (up to 4 per CU; round 4), 4 = four waves, lower register use (larger batches), 2 = four waves
 * (the form for up to 4 per CU until round 4; the time-slice launches run on it).
 * Removed after measurement (source at 24082b1; M frames/s on the configs[4] shard, against 465 for form 4 then):
 *   1 = one wave per utterance, the round-1 kernel: 190-219
 *   5 = two utterances per workgroup, lane-sparse phases packed: 434 (profiles/r04_ns_pair_form_experiment.txt)
 *   7 = one wave per utterance running every role in sequence: 363 (profiles/r04_ns_six_wave_dense.txt)
 * sea_ns_kernel_form(f) forces form f (0, 2, 3, 4 or 6) for later calls (0 = by batch size again; the SEA_NS_KERNEL
 * environment variable = pipe | pipe6 | pipe6d | big sets the initial value); any other f only reads.  Returns the previous
 * form. */
int sea_ns_kernel_form(int form);
/* The same for one TIME SLICE of every utterance: a batch may be cut along the time axis and run as one launch per
 * slice, so that a caller can upload slice k + 1 and download slice k - 1 while slice k is on the device
 * (sea_denoise_utterances does).  d_in / d_out / d_offsets / d_lengths describe THIS slice (each utterance's frames of
 * the slice, packed like a batch of their own); d_state holds sea_ns_slice_state_floats() floats per utterance --
 * utterance u of every slice is the same utterance -- and carries the recursion (DoNoiseSup's state, the pipeline's
 * sample rings, the DC filter, the zero-frame gate) from launch to launch; resume = 0 for the first slice.  The slices
 * of an utterance must be whole frames except the last; frame_base = the utterance's frames before this slice
 * (d_first_out, optional, is the absolute frame index of the first NoiseSup output).  Results are those of the one
 * launch: tests/test_gpu_parity.py::test_ns_time_slices_equal_one_launch. */
int sea_ns_denoise_batch_slice(const short *d_in, short *d_out, float *d_out_f32, const long long *d_offsets,
                               const long long *d_lengths, const int *d_order, int *d_first_out, float *d_state, int n_utt,
                               int frame_base, int resume, void *stream);
int sea_ns_slice_state_floats(void);

/* SURVEY 8(f) #3 -- the feature chain the reference keeps commented out (etsi/cpp/ParmInterface.c:274-311):
 * WaveProc -> CompCeps -> PostProc -> VAD, then FlushAdvProcess (:348-354).
 * Step 1: NoiseSup that also stores what the frame-dropping VAD votes over.  d_flags: one byte per
 * output frame fo of utterance u at [d_offsets[u]/8 + 10*fo] (buffer of total_padded_samples/8
 * bytes): bit 0 SpeechFoundVar, 1 SpeechFoundSpec, 2 SpeechFoundMel, 3 SpeechFoundVADNS
 * (NoiseSup.c:1255-1281, :1359-1365).  d_onset[u]: index of the first non-zero frame. */
int sea_ns_denoise_batch_fd(const short *d_in, short *d_out, float *d_out_f32,
                            const long long *d_offsets, const long long *d_lengths, const int *d_order,
                            int *d_first_out, unsigned char *d_flags, int *d_onset, int n_utt, void *stream);
/* Step 2: features.  d_ceps_cum / d_feat_cum: n_utt+1 prefix sums of per-utterance capacities
 * (>= lengths/80 - 6 cepstral frames, >= lengths/80 + 6 emitted frames).  d_feat_cc (and optionally
 * d_feat_pp) receive 14 floats per cepstral frame after WaveProc+CompCeps (after PostProc);
 * d_feat15 receives, per utterance and in emission order, the frames DoAdvProcess / FlushAdvProcess
 * would hand to the recogniser: c1..c12, c0, logE and the VAD flag (null vectors for the all-zero
 * lead, ParmInterface.c:314-329); d_n_feat[u] their number. */
int sea_afe_features_batch(const float *d_den_f32, const unsigned char *d_flags, const long long *d_offsets,
                           const long long *d_lengths, const int *d_first_out, const int *d_onset,
                           const long long *d_ceps_cum, long long total_ceps, float *d_feat_cc, float *d_feat_pp,
                           const long long *d_feat_cum, float *d_feat15, int *d_n_feat, int *d_n_ceps, int n_utt,
                           void *stream);
/* The 8 kHz feature chain in TIME SLICES: both steps over one slice of every utterance, cut as for sea_ns_denoise_batch_slice
 * (every buffer, d_offsets and d_lengths describe THIS slice, packed like a batch of its own; every slice of an utterance is a
 * multiple of 80 samples except its last, which may carry the ragged tail and may hold no whole frame at all; frame_base = the
 * utterance's frames before this slice; resume = 0 for the first slice, whose state is not read).
 * Step 1: sea_ns_denoise_batch_slice + what sea_ns_denoise_batch_fd stores.  d_flags: one byte per frame of THIS slice with an
 * output, at [d_offsets[u]/8 + 10*f], f the frame within the slice (buffer of the slice's total_padded_samples/8 bytes), bits as
 * sea_ns_denoise_batch_fd's; bytes of frames without an output are not written.  d_first_out and d_onset are ABSOLUTE frame
 * indices and, like d_out_f32, d_flags and d_state, required; d_onset is the first non-zero frame of 80 samples (the gate of
 * ParmInterface.c:244-251), while every frame so far was zero the frames so far (frame_base + the slice's frames), and after
 * all slices the one launch's value.  The state is sea_ns_denoise_batch_slice's, sea_ns_slice_state_floats () floats per
 * utterance: the seven speech measures and the onset ride in words of the frame loop's blob that the plain slice call leaves
 * alone -- run an utterance through one of the two calls, not a mixture.  Every other output is sea_ns_denoise_batch_slice's,
 * bit for bit.  One kernel form, the four-wave one, at every batch size. */
int sea_ns_denoise_batch_slice_fd(const short *d_in, short *d_out, float *d_out_f32, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int *d_first_out,
                                  unsigned char *d_flags, int *d_onset, float *d_state, int n_utt,
                                  int frame_base, int resume, void *stream);
/* Step 2: sea_afe_features_batch over what step 1 left of THIS slice (d_first_out / d_onset absolute, as that call leaves
 * them).  Every output describes the slice: d_feat_cc / d_feat_pp receive the cepstral frames that COMPLETE in it (frame j of
 * an utterance with first output f0 reads the float stream from sample 80 (f0 + j) - 1 and the flag of frame f0 + j + 2: it
 * completes with output frame f0 + j + 2), capacity per utterance >= the slice's frames; d_feat15 the frames EMITTED during it,
 * in emission order (a null vector per frame of the slice below the onset, then one row per completed cepstral frame once the
 * VAD's frame counter passes 10, then the flush), capacity >= the slice's frames + 6; d_n_feat[u] / d_n_ceps[u] the slice's
 * counts; rows behind the counts are left alone.  Concatenated over an utterance's slices all three are
 * sea_afe_features_batch's for the whole utterance, bit for bit, and the counts sum to its counts
 * (tests/test_gpu_afe_slices.py).  DoVADFlush runs only where d_final[u] (optional, one byte per utterance of the slice) is
 * non-zero: the utterance ends with this slice, which may hold just the ragged tail or nothing at all -- a stream whose end is
 * learnt late is flushed by an empty slice.  d_afe_state (required) holds sea_afe_slice_state_floats () floats per utterance,
 * separate from step 1's state and not read when resume == 0: the last three frames of the float stream, PostProc's weights,
 * the VAD's feature buffer, ring of seven and counters. */
int sea_afe_features_batch_slice(const float *d_den_f32, const unsigned char *d_flags, const long long *d_offsets,
                                 const long long *d_lengths, const int *d_first_out, const int *d_onset,
                                 const unsigned char *d_final, const long long *d_ceps_cum, long long total_ceps,
                                 float *d_feat_cc, float *d_feat_pp, const long long *d_feat_cum, float *d_feat15,
                                 int *d_n_feat, int *d_n_ceps, float *d_afe_state, int n_utt, int frame_base,
                                 int resume, void *stream);
int sea_afe_slice_state_floats(void);
/* The plain CompCeps (sea_compceps_batch: no WaveProc, 14 floats per frame) over one TIME SLICE of every utterance, after
 * sea_ns_denoise_batch_slice or sea_ns_denoise_batch_slice_fd on the same slice: d_den_f32, d_offsets, d_lengths, frame_base and
 * resume describe the slice exactly as that call left it; d_first_out is absolute.  Only the float stream and first_out are read
 * of the producer's outputs.  d_ceps receives the cepstral frames that COMPLETE in the slice (frame j of an utterance with first
 * output f0 reads the float stream from sample 80 (f0 + j) - 1 for 201 values: it completes with output frame f0 + j + 2), frame
 * jLo + r of the utterance in row d_ceps_cum[u] + r; d_ceps_cum holds n_utt + 1 prefix sums of per-utterance capacities >= the
 * slice's frames, total_frames = d_ceps_cum[n_utt]; d_n_ceps[u] is the slice's count, written for every utterance of every
 * slice, also one that holds only a ragged tail; rows behind the count are left alone.  d_cc_state (required) holds
 * sea_cc_slice_state_floats () floats per utterance, a blob of its own next to the producer's and not read when resume == 0: the
 * last three frames of the float stream.  Concatenated over an utterance's slices the rows are sea_compceps_batch's, bit for
 * bit, and the counts sum to its count (tests/test_gpu_ceps_slices.py).  Two launches on the stream: the tiles, which only read
 * the state, then one wave per utterance that writes the counts and the state. */
int sea_compceps_batch_slice(const float *d_den_f32, const long long *d_offsets, const long long *d_lengths,
                             const int *d_first_out, const long long *d_ceps_cum, long long total_frames,
                             float *d_ceps, int *d_n_ceps, float *d_cc_state, int n_utt, int frame_base,
                             int resume, void *stream);
int sea_cc_slice_state_floats(void);
/* The ETSI WIDEBAND (16 kHz) mode -- what AdvProcessAlloc (16000) switches on (etsi/cpp/ParmInterface.c:100-108), not the
 * defective wrapper etsi_denoise_16k: frames of 160 samples at 16 kHz, each split by the standard's 118-tap QMF pair into a
 * 0-4 kHz and a 4-8 kHz half (Do16kProcessing, etsi/cpp/16kHzProcessing.c:711-774).  The low half runs through the
 * two-stage Wiener filter exactly as an 8 kHz signal would; the high half becomes, per NoiseSup output frame, three
 * spectrally subtracted mel band energies and a 3 x 3 code against the low band's upper bands (NoiseSup.c:1216-1235,
 * :1307-1327), which sea_wb_compceps_batch merges into a 26-band cepstrum.
 *   d_in             packed int16 at 16 kHz, utterance u at [d_offsets[u], d_offsets[u] + d_lengths[u]) as above; the trailing
 *                    d_lengths[u] % 160 samples are ignored
 *   everything at the 8 kHz rate is indexed by HALF the offset: frame f (80 samples) of utterance u sits at
 *                    d_offsets[u] / 2 + 80 f, in buffers of total_padded_samples / 2 elements
 *   per-frame ROWS   frame f of utterance u owns row ceil (d_offsets[u] / 160) + f of buffers with
 *                    sea_wb_rows (total_padded_samples) rows; only frames with a NoiseSup output have their rows written
 *   d_out_lp         int16 low-band output, (short) truncation of the float one; zeros for every frame before the first
 *                    NoiseSup output (4 frames after the first non-zero input frame), as etsi_denoise writes them
 *   d_out_f32        optional: the float NoiseSup output, written where produced
 *   d_first_out      optional: per utterance, index of the first frame with an output, -1 if none
 *   d_onset          optional: per utterance, index of the first frame whose 160 raw samples are not all zero (the zero-frame
 *                    gate of ParmInterface.c:244-251 acts on the raw input; frames before it advance nothing), the frame
 *                    count if there is none
 *   d_hp_rows        optional, with d_code_rows: rows of 3 floats, the high-band energies after DoSpecSub16k (what
 *                    NoiseSup.c:1421-1422 appends to hpBands)
 *   d_code_rows      rows of 9 floats, CodeForBands16k (NoiseSup.c:1325)
 *   d_scratch        sea_wb_scratch_bytes (total_padded_samples, n_utt) bytes, 16-byte aligned.  After the call its first
 *                    total_padded_samples / 2 floats (rounded up to 8) hold the QMF low band and the next as many the high
 *                    band (shifted down to 0-4 kHz), indexed like the other 8 kHz-rate buffers, for every whole frame
 *   total_padded_samples  size of d_in in samples (the sum of the utterances' lengths, each rounded up to 8) */
int sea_wb_denoise_batch(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                         const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset, float *d_hp_rows,
                         float *d_code_rows, void *d_scratch, long long total_padded_samples, int n_utt, void *stream);
long long sea_wb_scratch_bytes(long long total_padded_samples, int n_utt);
long long sea_wb_rows(long long total_padded_samples);
/* The same for one TIME SLICE of every utterance, as sea_ns_denoise_batch_slice is for 8 kHz: a wideband batch may be cut
 * along the time axis and run slice by slice (sea_wb_denoise_utterances does), for audio that does not fit or has not all
 * arrived.  Every buffer, d_offsets, d_lengths, the rows, d_scratch and total_padded_samples describe THIS slice, packed like
 * a batch of its own with the conventions above; utterance u of every slice is the same utterance.  Every slice of an
 * utterance is a multiple of 160 samples except its last, which may carry the ragged tail and may hold no whole frame at all;
 * frame_base = the utterance's frames of 160 samples before this slice; resume = 0 for the first slice, whose state is not
 * read.  d_state (required) holds sea_wb_slice_state_floats () floats per utterance and carries everything from launch to
 * launch: the QMF delay line (the last 117 raw samples), the first non-zero frame, the frame loop's recursion as in
 * sea_ns_denoise_batch_slice, the last five frames of both QMF streams for the high band's windows, and DoSpecSub16k's
 * tracker.  d_first_out and d_onset (optional) are ABSOLUTE frame indices and have their one-launch meaning once all slices
 * of the utterance have run (until then d_onset is the frames so far while all were zero).  Every whole frame of the slice
 * gets its 80 d_out_lp samples, zeros where it has no output; rows and d_out_f32 are written for frames with an output only.
 * Results are bit for bit those of the one launch: tests/test_gpu_wb_slices.py.  The feature chain has a slice form of its own
 * with a state of its own (sea_wb_denoise_batch_slice_fd + sea_wb_afe_features_batch_slice below).  So has the plain cepstrum
 * without WaveProc, whose windows cross slice boundaries: sea_wb_compceps_batch_slice below carries the last three frames of the
 * float stream and the last two rows of either kind from slice to slice.  Neither the float stream nor the rows of earlier
 * slices need to be kept. */
int sea_wb_denoise_batch_slice(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                               const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                               float *d_hp_rows, float *d_code_rows, void *d_scratch, long long total_padded_samples,
                               float *d_state, int n_utt, int frame_base, int resume, void *stream);
int sea_wb_slice_state_floats(void);
/* The wideband CompCeps (CompCeps.c:392-402, :464-479, :488-530) on those outputs: 14 floats per cepstral frame (c1..c12, c0,
 * logE; 26-band DCT, logE after the high-band correction), the first after the third NoiseSup output.  d_ceps_cum /
 * d_ceps / d_n_ceps as for sea_compceps_batch, capacities >= d_lengths[u] / 160 - 6. */
int sea_wb_compceps_batch(const float *d_out_f32, const long long *d_offsets, const long long *d_lengths, const int *d_first_out,
                          const float *d_hp_rows, const float *d_code_rows, const long long *d_ceps_cum, long long total_frames,
                          float *d_ceps, int *d_n_ceps, int n_utt, void *stream);
/* The wideband CompCeps over one TIME SLICE, as sea_compceps_batch_slice is for 8 kHz (see there): d_out_f32, d_offsets, d_lengths,
 * d_hp_rows, d_code_rows, frame_base and resume describe the slice exactly as sea_wb_denoise_batch_slice (or _fd) left it, with
 * the wideband conventions above (the float stream at d_offsets[u] / 2, the rows at ceil (d_offsets[u] / 160) + f, frames of 160
 * input samples); d_first_out is absolute.  d_cc_state (required) holds sea_wb_cc_slice_state_floats () floats per utterance: the
 * last three frames of the float stream, the last two high-band rows and the last two code rows.  Concatenated over an
 * utterance's slices the rows are sea_wb_compceps_batch's, bit for bit, and the counts sum to its count
 * (tests/test_gpu_ceps_slices.py). */
int sea_wb_compceps_batch_slice(const float *d_out_f32, const long long *d_offsets, const long long *d_lengths,
                                const int *d_first_out, const float *d_hp_rows, const float *d_code_rows,
                                const long long *d_ceps_cum, long long total_frames, float *d_ceps, int *d_n_ceps,
                                float *d_cc_state, int n_utt, int frame_base, int resume, void *stream);
int sea_wb_cc_slice_state_floats(void);
/* The wideband FEATURE CHAIN -- what DoAdvProcess / FlushAdvProcess hand to a recogniser in the AdvProcessAlloc (16000) mode
 * once the block the reference keeps commented out runs (etsi/cpp/ParmInterface.c:274-311, :348-354): NoiseSup -> WaveProc ->
 * CompCeps -> PostProc -> frame-dropping VAD, as sea_ns_denoise_batch_fd + sea_afe_features_batch are for 8 kHz.
 * Step 1: sea_wb_denoise_batch that also stores what the frame-dropping VAD votes over.  d_flag_rows: ONE BYTE PER PER-FRAME
 * ROW (buffer of sea_wb_rows (total_padded_samples) bytes, the row convention of d_hp_rows): for a frame with a NoiseSup output,
 * bit 0 SpeechFoundVar, 1 SpeechFoundSpec, 2 SpeechFoundMel, 3 SpeechFoundVADNS as the first stage left them at that frame
 * (NoiseSup.c:1255-1281, :1359-1365); rows of other frames are not written.  d_out_f32, d_first_out, d_onset and d_flag_rows
 * are required here; every other output is bit for bit sea_wb_denoise_batch's. */
int sea_wb_denoise_batch_fd(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                            const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                            unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                            long long total_padded_samples, int n_utt, void *stream);
/* Step 2: features, with the meaning and the emission order of sea_afe_features_batch.  DoWaveProc (WaveProc.c:397-455) on the
 * low band's 200-sample frame, then the wideband DoCompCeps (CompCeps.c:392-402, :464-479, :488-530) with the frame's rows of
 * d_hp_rows / d_code_rows -> d_feat_cc; DoPostProc (PostProc.c:123-149) -> d_feat_pp (optional); DoVADProc (VAD.c:219-317) and
 * DoVADFlush (:342-433) -> d_feat15 = c1..c12, c0, logE and the VAD flag per emitted frame, the null vectors of the all-zero
 * lead first (ParmInterface.c:314-329: d_onset of them, the gate acts on the 160 raw samples, :244-251); d_n_feat[u] their
 * number, d_n_ceps[u] (optional) the cepstral frames.  d_ceps_cum / d_feat_cum: n_utt + 1 prefix sums of per-utterance
 * capacities >= d_lengths[u] / 160 - 6 cepstral and >= d_lengths[u] / 160 + 6 emitted frames; total_ceps = d_ceps_cum[n_utt]. */
int sea_wb_afe_features_batch(const float *d_out_f32, const unsigned char *d_flag_rows, const float *d_hp_rows,
                              const float *d_code_rows, const long long *d_offsets, const long long *d_lengths,
                              const int *d_first_out, const int *d_onset, const long long *d_ceps_cum, long long total_ceps,
                              float *d_feat_cc, float *d_feat_pp, const long long *d_feat_cum, float *d_feat15, int *d_n_feat,
                              int *d_n_ceps, int n_utt, void *stream);
/* The feature chain in TIME SLICES: both steps over one slice of every utterance, cut as for sea_wb_denoise_batch_slice.
 * Step 1: sea_wb_denoise_batch_slice that also stores the speech flags.  d_flag_rows: one byte per per-frame row of THIS
 * slice, in the row convention of d_hp_rows, written for frames with an output only.  d_out_f32, d_first_out, d_onset,
 * d_flag_rows, d_hp_rows and d_code_rows are required; everything else it writes is sea_wb_denoise_batch_slice's, bit for bit.
 * The state is that call's, sea_wb_slice_state_floats () floats per utterance (the speech measures ride in words of the frame
 * loop's blob that the plain slice call leaves alone: run an utterance through one of the two calls, not a mixture). */
int sea_wb_denoise_batch_slice_fd(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                                  unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                                  long long total_padded_samples, float *d_state, int n_utt, int frame_base, int resume,
                                  void *stream);
/* Step 2: sea_wb_afe_features_batch over what step 1 left of THIS slice (buffers, d_offsets, d_lengths, frame_base and resume as
 * there; d_first_out / d_onset absolute, as that call leaves them).  Every output describes the slice: d_feat_cc / d_feat_pp
 * receive the cepstral frames that COMPLETE in it (frame j of an utterance with first output f0 completes with output frame
 * f0 + j + 2), capacity per utterance >= the slice's frames; d_feat15 the frames EMITTED during it, in emission order, capacity
 * >= the slice's frames + 6 (a frame before the onset gives one null vector, a later one completes at most one cepstral frame,
 * the flush adds six); d_n_feat[u] / d_n_ceps[u] the slice's counts.  Concatenated over an utterance's slices all three are
 * sea_wb_afe_features_batch's for the whole utterance, bit for bit, and the counts sum to its counts
 * (tests/test_gpu_wb_afe_slices.py).  DoVADFlush runs only where d_final[u] (optional, one byte per utterance of the slice) is
 * non-zero: the utterance ends with this slice, which may hold just the ragged tail or nothing at all -- a stream whose end is
 * learnt late is flushed by an empty slice.  d_afe_state (required) holds sea_wb_afe_slice_state_floats () floats per utterance,
 * separate from step 1's state and not read when resume == 0: the last three frames of the float stream, the last two
 * high-band and code rows, PostProc's weights, the VAD's feature buffer, ring of seven and counters. */
int sea_wb_afe_features_batch_slice(const float *d_out_f32, const unsigned char *d_flag_rows, const float *d_hp_rows,
                                    const float *d_code_rows, const long long *d_offsets, const long long *d_lengths,
                                    const int *d_first_out, const int *d_onset, const unsigned char *d_final,
                                    const long long *d_ceps_cum, long long total_ceps, float *d_feat_cc, float *d_feat_pp,
                                    const long long *d_feat_cum, float *d_feat15, int *d_n_feat, int *d_n_ceps, float *d_afe_state,
                                    int n_utt, int frame_base, int resume, void *stream);
int sea_wb_afe_slice_state_floats(void);
/* one utterance from host memory, in the style of etsi_denoise: out_lp[0 .. 80 * (n / 160)) is written */
int sea_wb_denoise(const short *in, long n, short *out_lp);
/* the mode's tables as the library computed them (tests): the QMF pair, bands 1..3 of the high band's mel filter
 * (InitMelFBwindows (.., 80.0, 8000, 128, 5, 0)) and the 26-channel DCT (InitDCTMatrix (13, 26)) */
int sea_wb_tables_host(float *qmfLp118, float *qmfHp118, int *hpMelStart3, int *hpMelLen3, float *hpMelW3x64, float *dct12x26);
/* 64-band gammatone resynthesis over a batch.  mask rows (64 floats) of utterance u start at row
 * d_mask_offsets[u] and number (lengths[u]-320)/160+1.  d_inter is scratch of
 * sea_resynth_scratch_bytes(total padded samples of the batch, n_utt) bytes (the [time][64]
 * float intermediate between the two passes, ~256 B per sample: it is what 288 GB of HBM is
 * for).  binary: bit 0 selects the ideal-binary-mask variant (resyth_64sub_IBM); bit 1 the older
 * driver's frame count, lengths[u]/160 mask rows per utterance instead of (lengths[u]-320)/160+1
 * (1dnn_resynth/extractwav.cpp:67: one more frame, whose falling half covers the last hop). */
int sea_resynth64_batch(const short *d_in, short *d_out, const long long *d_offsets,
                        const long long *d_lengths, const float *d_mask,
                        const long long *d_mask_offsets, float *d_inter, const int *d_order,
                        int n_utt, int binary, void *stream);
long long sea_resynth_scratch_bytes(long long total_padded_samples, int n_utt);

/* ----------------------------------------------------------------------------------------------
 * (2) handle-based plug-in equivalents and host-buffer conveniences
 * -------------------------------------------------------------------------------------------- */
/* Many utterances at once from host memory -- what etsi/cpp/main.cpp:43-67 does per file and the batch tool
 * function/20141106_speech_enhancement/aurora_speech_enhancement/aurora_speech_enhancement.cpp:25-80 from a thread
 * pool.  A copy / compute pipeline (csrc/hostpipe.hip) over TIME SLICES of the list: slice k = the frames
 * [B_k, B_k+1) of every utterance that has them (SEA_HOST_SLICES slices of equal sample count, default 8), one launch
 * per slice with the recursion carried per utterance (sea_ns_denoise_batch_slice); a pool of SEA_HOST_THREADS (default
 * min(8, cores - 1)) host threads packs slice k+1 into pinned staging and unpacks slice k-1 while slice k's upload,
 * launch and download run on a stream each.  SEA_HOST_MODE=chunks: chunks of whole utterances of about
 * SEA_HOST_CHUNK_MB MB instead (default a third of the list).  out[u][0 .. 80*(lengths[u]/80)) is written, exactly as
 * etsi_denoise does; results do not depend on either cut. */
int sea_denoise_utterances(const short *const *in, short *const *out, const long *lengths, int n_utt);
int sea_host_threads(void); /* size of that pool */
int sea_host_last_slices(void); /* launches (time slices) the calling thread's last sea_denoise_utterances call in the
                                 * time-slice mode, or its last sea_wb_denoise_utterances / sea_wb_features_utterances /
                                 * sea_features_utterances / sea_denoise_ceps_utterances / sea_wb_denoise_ceps_utterances call,
                                 * was cut into; 0 before any */
/* The same pipeline for the ETSI wideband (16 kHz) mode (sea_wb_denoise_batch_slice per slice): in[u] holds lengths[u] int16
 * samples at 16 kHz; out_lp[u] receives the 80 * (lengths[u] / 160) low-band samples sea_wb_denoise_batch writes.  hp_rows and
 * code_rows are optional, both or neither; each non-NULL hp_rows[u] (with code_rows[u]) receives 3 (9) floats per frame of
 * 160 samples, the rows of sea_wb_denoise_batch, zeros for frames without an output.  A single long utterance is cut into
 * several launches like any list; results do not depend on the cut (tests/test_gpu_wb_slices.py). */
int sea_wb_denoise_utterances(const short *const *in, short *const *out_lp, float *const *hp_rows, float *const *code_rows,
                              const long *lengths, int n_utt);
/* The wideband FEATURES from host buffers, as sea_denoise_ceps_utterances is for 8 kHz: the same cut and pipeline, per slice
 * sea_wb_denoise_batch_slice_fd + sea_wb_afe_features_batch_slice.  feats[u] has room for lengths[u] / 160 + 6 rows of 15 floats
 * (c1..c12, c0, logE, the VAD flag) and receives sea_wb_afe_features_batch's rows for the utterance, n_feat[u] their number;
 * out_lp (optional, as a whole) as above.  Only the emitted rows and their counts travel back; the float stream, the flag bytes
 * and the high-band rows never leave the device.  Results do not depend on the cut (tests/test_gpu_wb_afe_slices.py). */
int sea_wb_features_utterances(const short *const *in, short *const *out_lp, float *const *feats, int *n_feat,
                               const long *lengths, int n_utt);
/* The 8 kHz FEATURES from host buffers -- the rows a recogniser consumes: the same cut and pipeline, per slice
 * sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice.  feats[u] has room for lengths[u] / 80 + 6 rows of 15 floats
 * (c1..c12, c0, logE, the VAD flag) and receives sea_afe_features_batch's rows for the utterance, n_feat[u] their number (an
 * utterance shorter than 80 samples gives DoVADFlush's six zero rows); out (optional, as a whole) as sea_denoise_utterances
 * writes it.  Only the emitted rows, their counts and out travel back; the float stream, the flag bytes and the cepstra before
 * PostProc never leave the device.  Results do not depend on the cut (tests/test_gpu_afe_slices.py). */
int sea_features_utterances(const short *const *in, short *const *out, float *const *feats, int *n_feat,
                            const long *lengths, int n_utt);
/* NoiseSup from PINNED staging the caller fills and reads -- no pack / unpack copies (csrc/hostpipe.hip).  For a caller that
 * produces its samples itself (a file reader) and consumes the results itself (a file writer):
 *   p = sea_packed_create();                          a reusable staging set (pinned, portable across devices)
 *   sea_packed_plan(p, lengths, n_utt);               lays the list out in time slices (as sea_denoise_utterances does inside)
 *   k = sea_packed_segments(p, u, in, out, count, max);   utterance u = k pieces in time order (k <= sea_packed_slices(p)):
 *                                                     write its samples into in[i][0 .. count[i]), i = 0..k-1
 *   sea_packed_denoise(p);                            on a thread bound to a device (sea_init): 0, or 1 = fault
 *   ... out[i][0 .. count[i]) is etsi_denoise's output for every whole frame of utterance u; the trailing lengths[u] % 80
 *   samples belong to no piece (etsi_denoise never writes them).  A set may be planned again after it has been read. */
typedef struct sea_packed sea_packed;
sea_packed *sea_packed_create(void);
void sea_packed_destroy(sea_packed *p);
int sea_packed_plan(sea_packed *p, const long *lengths, int n_utt);
int sea_packed_slices(const sea_packed *p);
int sea_packed_segments(const sea_packed *p, int u, short **in_seg, short **out_seg, long *count, int max_seg);
int sea_packed_denoise(sea_packed *p);
/* NoiseSup + CompCeps from host buffers, the chain ParmInterface.c:275-293 ran before its author commented it out
 * (SURVEY 8(d) Config 1: a 4-s utterance gives 800 NoiseSup frames, 796 outputs, 794 cepstral frames): out as above;
 * ceps[u] receives n_ceps[u] rows of 14 floats (c1..c12, c0, logE), capacity max(lengths[u]/80 - 6, 0) rows.  A list the slice
 * plan cuts (SEA_HOST_SLICES, default 8; small lists stay in one piece) runs sea_denoise_utterances' pipeline with
 * sea_ns_denoise_batch_slice + sea_compceps_batch_slice per slice, the float stream sized for one slice; a list in one piece
 * runs one launch each.  SEA_HOST_CEPS_PIPELINE=0 keeps the one launch for every list.  Results do not depend on the cut
 * (tests/test_gpu_ceps_slices.py); sea_host_last_slices () reports it. */
int sea_denoise_ceps_utterances(const short *const *in, short *const *out, float *const *ceps, int *n_ceps,
                                const long *lengths, int n_utt);
/* The same for the wideband (16 kHz) mode: sea_wb_denoise_utterances' cut and pipeline, per slice sea_wb_denoise_batch_slice +
 * sea_wb_compceps_batch_slice.  out_lp (optional, as a whole) as there; ceps[u] receives n_ceps[u] rows of 14 floats,
 * sea_wb_compceps_batch's, capacity max(lengths[u]/160 - 6, 0) rows.  Only out_lp, the cepstral rows and their counts travel
 * back: the float stream and the high-band and code rows are sized for one slice and never leave the device. */
int sea_wb_denoise_ceps_utterances(const short *const *in, short *const *out_lp, float *const *ceps, int *n_ceps,
                                   const long *lengths, int n_utt);

/* DoCompCeps(Data, Coef, This): Data[-1] must be valid (host pointers) */
int sea_compceps_frame(const float *Data, float *Coef14);

/* resynth(): in/out L samples, mask [F][64] with F=(L-320)/160+1 (host pointers) */
int sea_resynth64(const short *in, long L, const float *mask, int F, int binary, short *out);
/* many utterances at once from host memory (masks[u] is [F_u][64]): the same pipeline; a chunk is also bounded by
 * its share of the HBM scratch budget (60 % of the free HBM over four streams; SEA_RESYNTH_SCRATCH_MB overrides) */
int sea_resynth_utterances(const short *const *in, const long *lengths, const float *const *masks, int binary,
                           short *const *out, int n_utt);
/* subbband() (enhancement_extract_test/cpp/extractwav.cpp:40-101): gammatone + Meddis hair cell
 * (resyth_64sub_ori/cpp/extractwav.cpp:212-257) + (short) cast -> 64 int16 streams.
 * Host form: out is [64][L].  Batch form (device pointers): utterance u's streams form a [64][pitch]
 * block at d_out + d_offsets[u]*64 with pitch = lengths[u] rounded up to 8; d_out holds 64x the
 * packed input size. */
int sea_subband64(const short *in, long L, short *out);
int sea_subband64_batch(const short *d_in, short *d_out, const long long *d_offsets, const long long *d_lengths,
                        const int *d_order, int n_utt, void *stream);
/* SURVEY 8(f) #2 -- the ideal-ratio-mask TARGET of make_single_IBM (enhancement_extract_test/cpp/show_IBM.cpp:105-169):
 * from the 64 subband streams of the clean and of the noise signal (two sea_subband64 outputs), frames of 320
 * samples every 160, 512-point power spectrum, first 64 bins summed, IRM = pure / (pure + noise); one row of 64
 * floats per frame = the mask matrix sea_resynth64 takes (and sea_mask_text_write prints).  The reference's
 * spectrum routine, asdk::SpecInfo, is absent third-party code: its analysis window is the `window` parameter here
 * (0 rectangular, 1 Hamming, 2 Hanning) and parity is unpinned.  Host form: streams [64][L], irm [F][64],
 * F = (L-320)/160+1.  Batch form: blocks as sea_subband64_batch writes them; utterance u's rows start at
 * d_row_offsets[u] (the d_mask_offsets of sea_resynth64_batch). */
int sea_irm_target(const short *pure64, const short *noise64, long L, int window, float *irm);
int sea_irm_target_batch(const short *d_pure64, const short *d_noise64, const long long *d_offsets,
                         const long long *d_lengths, const long long *d_row_offsets, float *d_irm, int window,
                         int n_utt, void *stream);
/* The training-set builder (enhancement_extract_subband_linux/cpp/main.cpp:91-274; csrc/mix_kernel.hip).
 * addnoise() (extractwav.cpp:6-35) per utterance, as g++ on x86-64 compiles it: two float sums of x * x over the clean signal
 * and the noise stretch, every step one correctly rounded float addition IN ORDER (sum = (float)((double)sum + (double)(x * x)));
 * gain = sqrt ((pure / noise) / snr_lin) in float; scaled[i] = (short)((float)noise[i] * gain), where the conversion is DEFINED
 * as int32 truncating toward zero with the low 16 bits kept and 0 for a NaN or a product of magnitude >= 2^31; noisy[i] = low 16
 * bits of clean[i] + scaled[i].  Silent noise gives gain inf, scaled noise 0 and noisy = clean; silent clean gives gain 0.
 * The reference cannot be compiled (its file includes the absent Wave.h): parity unpinned, semantics pinned to a restatement.
 * Batch form (device pointers): d_clean / d_offsets / d_lengths a packed batch (offsets multiples of 8); d_noise_src all noise
 * recordings back to back, utterance u's stretch starting at sample d_noise_start[u] (gathered on the device); d_snr_lin[u] =
 * (float)pow (10.0, db / 10.0) with db an int; d_noise_scaled / d_noisy laid out like d_clean (the pad samples become 0);
 * d_sums [n_utt][2] = (pure, noise) and d_gain [n_utt], either may be NULL.  The second launch reads the sums the first wrote:
 * without d_sums they live in a buffer of the calling host thread that only grows (allocated at the first such call and when a
 * larger batch comes), so calls WITHOUT d_sums from one thread must not overlap on the device -- keep them on one stream, or
 * pass d_sums, which also keeps the call free of any allocation.  Host form: one utterance, host pointers, the
 * outputs optional. */
int sea_addnoise_batch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
                       const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy,
                       float *d_sums, float *d_gain, int n_utt, void *stream);
int sea_addnoise(const short *clean, const short *noise, long L, int db, short *noise_scaled, short *noisy, float *sums2,
                 float *gain);
/* The mix, then sea_subband64_batch of the clean and of the SCALED noise (and of the noisy signal when d_sub_noisy is given),
 * then sea_irm_target_batch (clean, scaled noise), all on `stream`.  The subband buffers are the caller's, 64x the packed size
 * each; with d_sums given nothing is allocated inside (without it: the per-thread buffer and its rule above).  Every utterance
 * needs 320 samples: the lengths are read back first (one stream synchronisation) and a shorter one makes the call return
 * non-zero before anything is launched.  This is the one device-pointer call that waits for its stream; on a stream that is
 * being captured into a graph it returns non-zero at once, before the read-back, and leaves the capture valid. */
int sea_trainset_batch(const short *d_clean, const long long *d_offsets, const long long *d_lengths, const short *d_noise_src,
                       const long long *d_noise_start, const float *d_snr_lin, short *d_noise_scaled, short *d_noisy,
                       float *d_sums, float *d_gain, short *d_sub_clean, short *d_sub_noise, short *d_sub_noisy,
                       const long long *d_row_offsets, float *d_irm, int window, const int *d_order, int n_utt, void *stream);
/* The same from host memory: utterance u is mixed with noises[rec[u]][off[u] .. off[u] + lengths[u]) at db[u] dB.  Outputs:
 * noisy[u] (lengths[u] samples) and irm[u] ([(L-320)/160+1][64]) are required; noise_scaled, sub_clean, sub_noise and
 * sub_noisy are optional as a whole (NULL) and per utterance, the subband blocks [64][L] as sea_subband64 writes them; the
 * noisy subbands are computed only when sub_noisy is given.  L < 320, a recording index out of range, off < 0 or
 * off + L > noise_lengths[rec] return non-zero before the device is touched.  The recordings go up once per call; the list
 * runs in chunks of whole utterances whose device footprint (per sample 6 B of audio and 128 B per subband set, two
 * sets or three; 256 B per mask row) stays within 60 % of the free HBM (SEA_TRAINSET_SCRATCH_MB overrides); results do not depend on the cut.
 * sea_trainset_last_chunks () reports the calling thread's last cut. */
int sea_trainset_utterances(const short *const *clean, const long *lengths, int n_utt, const short *const *noises,
                            const long *noise_lengths, int n_noise, const int *rec, const long *off, const int *db, int window,
                            short *const *noisy, float *const *irm, short *const *noise_scaled, short *const *sub_clean,
                            short *const *sub_noise, short *const *sub_noisy);
int sea_trainset_last_chunks(void);
/* RECORDINGS, not utterances: how the reference's batch tool cuts a long recording for NoiseSup (BufferDenoise,
 * function/20141106_speech_enhancement/aurora_speech_enhancement/aurora_speech_enhancement.cpp:25-80) and where the stitched
 * result lies in the chunks' outputs (csrc/recording_plan.h).  Host arithmetic, no device needed.  The chunks
 * are independent NoiseSup chains, each from a fresh state -- so their stitched result is NOT etsi_denoise's on the whole
 * recording -- and can run as the utterances of one sea_denoise_utterances / sea_ns_denoise_batch call.
 * chunk = B is a multiple of 80 and at least 320 (the tool's is 1 440 000, 3 minutes at 8 kHz); with T = S / B and R = S % B the
 * chunks are x[0:S] when T = 0, else x[0:B], x[iB-320 : iB+B] for i = 1..T-1 and x[TB-320 : TB+R] (it exists when R = 0 too).
 * sea_recording_plan returns their number (0 for a recording shorter than 320 samples, which the tool skips; -1 and
 * sea_last_error () for a bad chunk) and fills, for the first max_chunks of them and where the pointer is given, chunk_src
 * (first sample in the recording), chunk_len and chunk_off: the chunk's offset, a multiple of 8, in a LAYOUT that holds the
 * chunks one after the other, each padded to 8 samples -- sea_recording_layout_samples () samples = S + 320 T and the pad. */
long long sea_recording_plan(long samples, long chunk, long long *chunk_src, long long *chunk_len, long long *chunk_off,
                             long long max_chunks);
long long sea_recording_layout_samples(long samples, long chunk);
/* The stitch: index[k], for t = first + k, is where des[t] lies in the chunks' etsi_denoise outputs laid out as above (zeroed
 * first: etsi_denoise never writes a chunk's trailing len % 80 samples), or -1 where des[t] is 0 -- the last 320 samples.
 * des[t] = out[chunk_off[i] + t + 320 + (i > 0 ? 320 : 0) - i B] with i = (t + 320) / B. */
int sea_recording_stitch_map(long samples, long chunk, long first, long count, long long *index);
/* The front half of the Hu-Wang mask estimator createIBM() (function/20141106_speech_enhancement/aurora_etsi_test/
 * HuWang.cpp:41-76) on its 25-channel 8 kHz gammatone bank: AudiPeriph (gammatone + Meddis hair cell, hOut in float), lowPass
 * (hEv), computeACF, crossCorr, globalPitch, timeCrn (corrHc) and the initial labelling of Grp (csrc/hw25_kernel.hip,
 * DESIGN.md section 5.11).  Parity: bit for bit against the reference's own functions compiled on a CPU
 * (tests/golden/hw25_golden.npz).  initGroup and pitchDtm follow below (sea_hw25_pitch_*), then computeAM, finalSeg and the
 * whole estimator (sea_hw25_am_batch, sea_hw25_finalseg_batch, sea_hw25_ibm*), and last resynthesis (sea_hw25_resynth*,
 * sea_hw25_enhance*): audio in, enhanced audio out.
 * Samples are floats on the int16 scale, as createIBM takes them.  Batch forms (device pointers): d_in_f32 holds the packed
 * batch, utterance u at d_offsets[u] (multiples of 8; the stretch up to the next multiple of 8 past its length must be
 * readable); d_hout / d_hev hold 25x the packed size, utterance u's [25][pitch] block at d_offsets[u] * 25, pitch =
 * lengths[u] rounded up to 8 (the padding is not written).  Utterance u has sea_hw25_frames (lengths[u]) = lengths[u] / 80
 * rows starting at d_row_offsets[u]: d_cross_hc / d_cross_ev / d_pratio / d_mark [rows][25] floats (mark is 0 or 1),
 * d_pitch [rows] ints (16..100), d_acf_hc / d_acf_ev [rows][25][101] floats -- large (2 x 10100 B per row), so optional:
 * a null pointer is not written.  d_order (launch order, optional) as elsewhere.  sea_hw25_scratch_bytes is what d_scratch
 * must hold; the present form keeps a frame's ACFs in LDS and needs none (0 bytes, d_scratch may be null).
 * sea_hw25_frontend_batch is the two batch calls as one launch group on `stream`.  sea_hw25_frontend: one utterance from
 * host memory; hout / hev [25][L], the frame outputs as above with rows = L / 80; every output pointer may be null.
 * Every sea_hw25_*_batch call refuses what its sea_hw64_* namesake refuses, before anything is launched: a null required
 * pointer, and an output that is an input (d_offsets, d_lengths, d_row_offsets and d_order included) or another output. */
int sea_hw25_tables_host(float *cf25, float *bw25, float *midEar25, float *gain25, float *f1_25, float *f2_25, int *winsize25,
                         float *lp91, float *hair10 /* ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0 */);
long long sea_hw25_frames(long long length);
long long sea_hw25_scratch_bytes(long long total_padded_samples, int n_utt);
int sea_hw25_periphery_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int n_utt, void *stream);
int sea_hw25_correlogram_batch(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                               const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc,
                               float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                               const int *d_order, int n_utt, void *stream);
int sea_hw25_frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev,
                            float *d_cross_hc, float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                            const int *d_order, int n_utt, void *stream);
int sea_hw25_frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc,
                      float *cross_ev, int *pitch, float *pratio, float *mark);
/* createIBM():79-87 on the same bank: initGroup (HuWang.cpp:639-702, with segmentation / search / relationship:466-637) and
 * pitchDtm (:795-824: findPitch, sumAuto, pitchCrn, checkPitch, leftDevelope, rightDevelope, linearEstimate, timeCrn, reGroup,
 * relationship2) -- the pitch contour of the dominant voiced source and the units grouped with it (csrc/hw25_pitch_kernel.hip,
 * DESIGN.md section 5.12).  Parity: bit for bit, every stage, against the reference's own functions compiled on a CPU
 * (tests/golden/hw25_pitch_golden.npz).
 * Inputs are rows as sea_hw25_correlogram_batch writes them and are not modified: d_acf_hc [rows][25][101], d_cross_hc,
 * d_pratio_in, d_mark_in [rows][25]; utterance u has lengths[u] / 80 rows from d_row_offsets[u].  (d_cross_hc is read because
 * the reference's leftDevelope / rightDevelope count `number2` over forty channels on this bank of 25: channels 25..39 of a
 * frame are, by the layout of its arrays, the frame's cross and pRatio and the next frame's acf and marks.  That is
 * reproduced, see below for the last frame.)  Outputs: d_pitch [rows] ints, Pitch after linearEstimate (0 = unvoiced, else
 * 16..100); d_grp [rows][25] floats in {-1, 0, +1}, Grp after reGroup (THETAT); d_pratio [rows][25], pRatio after the last
 * timeCrn (finalSeg reads it); d_status [n_utt] ints, bits 0..15 the segment count, flags above.  d_stages (optional, null:
 * not written): utterance u's block of SEA_HW25_STAGE_WORDS words per row starts at word d_row_offsets[u] *
 * SEA_HW25_STAGE_WORDS: [5][rows_u] ints, Pitch after findPitch #1, findPitch #2, checkPitch, leftDevelope, rightDevelope; then
 * [2][rows_u][25] floats, Grp after initGroup and after reGroup (THETAP).  d_scratch must hold sea_hw25_pitch_scratch_bytes
 * (total_rows, n_utt) bytes, total_rows being the extent of the row space (the largest d_row_offsets[u] + rows_u); d_order as
 * elsewhere.  The lengths stay on the device, nothing synchronises with the host, every launch is on `stream`.
 * No output buffer may overlap an input or another output (the inputs are read after the first outputs are written); equal
 * pointers are rejected.
 * Where the reference is undefined, this is defined:
 *  - no segment (always so with fewer than 3 rows): relationship writes Seg[0] of an empty array.  Here: segment count 0,
 *    pitch, grp, pratio (and the stages) all 0;
 *  - more than 400 segments: segMark[MAX_NUMBER_SEGMENT] overflows.  Here: SEA_HW25_TOO_MANY_SEGMENTS is set, bits 0..15 hold
 *    the count (at most 65535), pitch, grp, pratio (and the stages) all 0;
 *  - leftDevelope / rightDevelope read chan_mark uninitialised on their first step when the neighbouring frame has no pitch
 *    (no streak of three consistent frames).  Here chan_mark starts at zeros, and SEA_HW25_CHANMARK_UNSET is set when it was
 *    read before it was computed;
 *  - on the LAST frame of an utterance the fifteen channels 25..39 of `number2` lie past the reference's arrays.  Here they
 *    are not counted.
 * sea_hw25_pitch: one utterance from host memory; runs the front half itself with the ACF in a device buffer of its own;
 * pitch [L / 80], grp and pratio [L / 80][25], status [1]; pitch, grp and pratio may be null. */
enum {
    SEA_HW25_MAX_SEGMENTS = 400, /* MAX_NUMBER_SEGMENT */
    SEA_HW25_STAGE_WORDS = 55,   /* per row: 5 ints and 2 x 25 floats */
    SEA_HW25_TOO_MANY_SEGMENTS = 1 << 16,
    SEA_HW25_CHANMARK_UNSET = 1 << 17
};
long long sea_hw25_pitch_scratch_bytes(long long total_rows, int n_utt);
int sea_hw25_pitch_batch(const float *d_acf_hc, const float *d_cross_hc, const float *d_pratio_in, const float *d_mark_in,
                         const long long *d_lengths, const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio,
                         int *d_status, void *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream);
int sea_hw25_pitch(const float *x, long L, int *pitch, float *grp, float *pratio, int *status);
/* The rest of createIBM() on the same bank: computeAM (HuWang.cpp:1146-1317: amPatt, hilbert, computeAMRate, sinModel, with
 * kaiserPara / kaiserBandPass / bessi0 / fft:1553-1677), finalSeg (:1321-1494: reSegmentation, develope) and the binarisation
 * :99-106 (csrc/hw25_am_kernel.hip).  After it sea_hw25_ibm (x) is createIBM (x).
 * Parity (tests/golden/hw25_am_golden.npz, the reference's own functions compiled on a CPU): gOut, the AM pattern before and
 * after its normalisation and sEng bit for bit.  sinModel calls cosf, sinf and atanf on data; the C library's are not correctly
 * rounded and cannot be reproduced, so each is evaluated in double and rounded to float: ratio = error / sEng agrees to the
 * fixture's ratio_tol, and the label, every stage of finalSeg and the mask are equal wherever no ratio lies within that band of
 * THETAE = 0.20 (the fixture has no such unit).
 * sea_hw25_periphery_gout_batch is sea_hw25_periphery_batch with one more output: d_gout, gammaToneFilter's output before the
 * hair cell, in d_hout's layout (null: not written, exactly sea_hw25_periphery_batch).
 * sea_hw25_am_batch: inputs d_gout and d_pitch [rows] (sea_hw25_pitch_batch's; 0 = unvoiced, else 16..100), not modified.
 * Outputs d_amcrn [rows][25] floats 0 / 1, AmCrn; optional (null: not written) d_ratio and d_seng [rows][25] (error / sEng, 0
 * where sinModel does not run; sEng) and d_ampatt, d_am in d_gout's layout (amPatt's output; the same over its envelope).
 * d_status [n_utt]: flags only.  d_scratch must hold sea_hw25_am_scratch_bytes (total_padded_samples, n_utt) bytes, the same
 * total_padded_samples (the extent of the packed sample space: the largest d_offsets[u] + lengths[u] rounded up to 8) being
 * passed to the call: it decides whether the FFT (two complex buffers of 2 x the padded length per channel) runs over all 25
 * channels at once or in five groups of five channels.
 * sea_hw25_finalseg_batch: inputs d_grp and d_pratio (sea_hw25_pitch_batch's outputs), d_amcrn, d_cross_ev [rows][25], not
 * modified.  Outputs d_mask [rows][25] floats 0 / 1; d_status [n_utt] flags; optional d_grp_final [rows][25] in {-1, 0, 1}, Grp
 * before the binarisation, and d_stages: utterance u's [SEA_HW25_FINAL_STAGES][rows_u][25] floats at float d_row_offsets[u] *
 * SEA_HW25_FINAL_STAGES * 25, Grp after the relabelling that follows each reSegmentation (three), after develope (m, -1) with
 * its relabelling, and after develope (m, 1).  d_scratch: sea_hw25_finalseg_scratch_bytes (total_rows, n_utt).
 * sea_hw25_ibm_batch: the whole chain from packed float audio, one launch group on `stream`: d_mask [rows][25], d_pitch [rows],
 * d_status [n_utt] (sea_hw25_pitch_batch's status with the flags of the two later stages), d_stages optional as above;
 * d_scratch: sea_hw25_ibm_scratch_bytes (total_padded_samples, total_rows, n_utt), with the same totals passed to the call.
 * sea_hw25_ibm: one utterance from host memory; mask [L / 80][25], pitch [L / 80] (either may be null), status [1].  L = 0 is
 * an utterance without a frame: nothing is written but status = 0 (the batch forms take such an utterance too); L < 0 fails.
 * The lengths stay on the device, nothing synchronises with the host, every launch is on `stream`; no output may be an input
 * or another output (equal pointers are rejected).
 * Where the reference is undefined, or this differs, it is defined:
 *  - more than 150000 samples (MAX_SIG_LENGTH; the reference's Input[] overflows): SEA_HW25_AM_TOO_LONG, the AM outputs all 0,
 *    and in sea_hw25_ibm_batch the mask all 0.  No FFT runs;
 *  - a pitch above 100 (sea_hw25_pitch_batch never writes one): SEA_HW25_AM_BAD_PITCH, treated the same way;
 *  - reSegmentation finds more than 400 segments (segMark[MAX_NUMBER_SEGMENT] overflows, as in initGroup):
 *    SEA_HW25_FINAL_TOO_MANY_SEGMENTS, the mask (grp_final, the stages) all 0;
 *  - fewer than 3 rows: the mask (grp_final, the stages) is all 0 and no flag is set; with no segment upstream grp is all 0,
 *    no frame is voiced, and the mask is all 0 by the reference's own logic.
 * resynthesis (:1498) follows below (sea_hw25_resynth_*, sea_hw25_enhance_*). */
enum {
    SEA_HW25_FINAL_STAGES = 5,
    SEA_HW25_FINAL_TOO_MANY_SEGMENTS = 1 << 18,
    SEA_HW25_AM_TOO_LONG = 1 << 19,
    SEA_HW25_AM_BAD_PITCH = 1 << 20
};
int sea_hw25_periphery_gout_batch(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int n_utt, void *stream);
/* a = -20 log10 (delta) and beta of kaiserPara (0.01, ..), N of computeAM:1156 at L = 2^7 .. 2^17, and fft's twiddles u of every
 * stage (n_twiddles = 2^18 - 1 (re, im) pairs, period p's p values from entry p - 1); every pointer may be null */
int sea_hw25_am_tables_host(float *a_beta2, int *n_at_pow2_11, float *twiddles, int n_twiddles);
long long sea_hw25_am_scratch_bytes(long long total_padded_samples, int n_utt);
int sea_hw25_am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
                      const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
                      int *d_status, void *d_scratch, long long total_padded_samples, const int *d_order, int n_utt, void *stream);
long long sea_hw25_finalseg_scratch_bytes(long long total_rows, int n_utt);
int sea_hw25_finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final,
                            int *d_status, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream);
long long sea_hw25_ibm_scratch_bytes(long long total_padded_samples, long long total_rows, int n_utt);
int sea_hw25_ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                       float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
                       long long total_rows, const int *d_order, int n_utt, void *stream);
int sea_hw25_ibm(const float *x, long L, float *mask, int *pitch, int *status);
/* resynthesis() on the same bank (HuWang.cpp:1498-1549; csrc/hw25_resynth_kernel.hip): the mask applied
 * to gOut, enhanced audio out.  The same loop is the body of resynth (`mark > 0`, (short) cast to a WAV) and resynth_test
 * (`mark > 0.5`) in function_2/20141106_speech_enhancement/wav_extract/extractwav.cpp, hence the threshold and the int16 output.
 * Per channel c = 0..24 in order: gOut[c] / midEarCoeff[c] reversed in time, gammaToneFilter again, / midEarCoeff[c], reversed
 * back; times the overlap-add weight of the frames whose unit is set (mask > threshold; NaN and -0.0 > 0 are not set); the 25
 * products added in channel order from +0.0f, every channel multiplied and added whatever its weight (an Inf or NaN sample
 * under a weight of 0 gives NaN, as in the reference).  The window is not a raised cosine: WINDOW = 200 and OFFSET = 80, so a
 * set frame f adds up80[o] on [80 (f - 1), 80 f) -- not for f = 0 -- and down120[j], j = 0..119, on [80 f, 80 f + 120), whose
 * last 40 values rise again.  sea_hw25_resynth_tables_host: up80, down120 in double, and w640[o * 8 + bits], the float weight at
 * position o = 0..79 of a hop, bit 0 / 1 / 2 of `bits`: frame k - 1 / k / k + 1 (k = the sample's index / 80) exists and is set;
 * the terms are added in that order, each a double sum rounded to float, as the reference's `weight[..] +=`.  Every pointer
 * may be null.
 * Where the reference is undefined, this is defined: the reference's frame loop writes weight[] up to index 80 F + 39 of L
 * (F = L / 80), past the array when L % 80 < 40 and the last row has a unit set, onto the heap.  Here contributions at indices
 * >= L are dropped.  Parity: bit for bit against the reference's own resynthesis() compiled on a CPU
 * (tests/golden/hw25_resynth_golden.npz) on inputs where every channel's largest set frame f has 80 f + 119 < L; elsewhere
 * against the numpy model that is pinned to that fixture (tests/hw25_resynth_model.py).
 * sea_hw25_resynth_batch: d_gout as sea_hw25_periphery_gout_batch writes it and d_mask [rows][25] (utterance u's lengths[u] / 80
 * rows from d_row_offsets[u]) are not modified.  Outputs are packed as the input audio is: utterance u's lengths[u] samples at
 * d_offsets[u], the padding up to the next multiple of 8 not written; d_out_f32 floats, d_out_i16 their (short) conversion as
 * the x86-64 build performs it (truncation toward zero to int32, low 16 bits; NaN or a magnitude of 2^31 and more give 0).
 * Either output may be null, not both.  No scratch.  An utterance shorter than 80 samples has no frame and yields zeros.
 * sea_hw25_enhance_batch: sea_hw25_ibm_batch followed by the resynthesis (threshold 0) of its own mask from the gOut it keeps
 * in its scratch, one launch group on `stream`: d_mask, d_pitch, d_status as sea_hw25_ibm_batch writes them, d_scratch of
 * sea_hw25_ibm_scratch_bytes (total_padded_samples, total_rows, n_utt).  An utterance whose status zeroes the mask yields zeros.
 * n_utt <= 0 returns 0; null or equal pointers return non-zero before anything is launched.
 * sea_hw25_resynth / sea_hw25_enhance: one utterance from host memory (up to 150000 samples as sea_hw25_ibm); mask [F][25] with
 * F = L / 80 (anything else fails); out_f32 [L]; sea_hw25_enhance's mask and pitch may be null.  L = 0 is no work.
 * sea_hw25_resynth_text_write: one "%f\n" line per sample, byte for byte the file that resynthesis() writes (:1543-1544). */
int sea_hw25_resynth_tables_host(float *w640, double *up80, double *down120);
int sea_hw25_resynth_batch(const float *d_gout, const float *d_mask, const long long *d_offsets, const long long *d_lengths,
                           const long long *d_row_offsets, float threshold, float *d_out_f32, short *d_out_i16, const int *d_order,
                           int n_utt, void *stream);
int sea_hw25_enhance_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                           float *d_out_f32, short *d_out_i16, float *d_mask, int *d_pitch, int *d_status, void *d_scratch,
                           long long total_padded_samples, long long total_rows, const int *d_order, int n_utt, void *stream);
int sea_hw25_resynth(const float *x, long L, const float *mask, long F, float threshold, float *out_f32);
int sea_hw25_enhance(const float *x, long L, float *out_f32, float *mask, int *pitch, int *status);
int sea_hw25_resynth_text_write(const char *path, const float *out, long L);
/* The front half of createIBM() at 16 kHz on 64 channels: the same HuWang.cpp:41-76 at the constants of resyth_64sub_IBM/cpp/
 * HuWang.h (SAMPLING_FREQUENCY 16000, NUMBER_CHANNEL 64, MINCF 50, MAXCF 8000, WINDOW 320, OFFSET 160, MAX_DELAY 201, MIN_DELAY
 * 32), the bank of sea_subband64_batch / sea_resynth64_batch / sea_irm_target_batch (csrc/hw64_kernel.hip, DESIGN.md section
 * 5.16).  Parity: bit for bit against the reference's own functions compiled on a CPU against that header
 * (tests/golden/hw64_*.npz).  initGroup and pitchDtm follow below (sea_hw64_pitch_*), then computeAM, finalSeg and the whole
 * estimator (sea_hw64_am_batch, sea_hw64_finalseg_batch, sea_hw64_ibm*), then resynthesis() from host memory (sea_hw64_resynth*,
 * sea_hw64_enhance*): of the reference's chain only resynthesis() is NOT built at 16 kHz as a call on device pointers.
 * The calls mirror the sea_hw25_* front-half calls argument for argument, with 64 / 201 / 160 for 25 / 101 / 80: d_hout / d_hev
 * (and d_gout, the gammatone output before the hair cell; null: not written) hold 64x the packed size, utterance u's
 * [64][pitch] block at d_offsets[u] * 64; utterance u has sea_hw64_frames (lengths[u]) = lengths[u] / 160 rows from
 * d_row_offsets[u]: d_cross_hc / d_cross_ev / d_pratio / d_mark [rows][64], d_pitch [rows] (32..200), d_acf_hc / d_acf_ev
 * [rows][64][201] -- 51 456 B per row and stream, optional: a null pointer is not written.  d_scratch is not read and may be
 * null.  Null pointers and an output that is an input or another output are refused before anything is launched; n_utt <= 0
 * returns 0; the lengths stay on the device and nothing synchronises with the host.  sea_hw64_workgroups_per_utterance: how
 * many workgroups the correlogram launch gives every utterance of a batch of n_utt on the current device (workgroup g takes
 * the frames g, g + G, ..); 0 on error. */
int sea_hw64_tables_host(float *cf64, float *bw64, float *midEar64, float *gain64, float *f1_64, float *f2_64, int *winsize64,
                         float *lp181, float *hair10 /* ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0 */);
long long sea_hw64_frames(long long length);
int sea_hw64_workgroups_per_utterance(int n_utt);
int sea_hw64_periphery_batch(const float *d_in_f32, float *d_hout, float *d_hev, float *d_gout, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int n_utt, void *stream);
int sea_hw64_correlogram_batch(const float *d_hout, const float *d_hev, const long long *d_offsets, const long long *d_lengths,
                               const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev, float *d_cross_hc,
                               float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                               const int *d_order, int n_utt, void *stream);
int sea_hw64_frontend_batch(const float *d_in_f32, float *d_hout, float *d_hev, const long long *d_offsets,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_acf_hc, float *d_acf_ev,
                            float *d_cross_hc, float *d_cross_ev, int *d_pitch, float *d_pratio, float *d_mark, void *d_scratch,
                            const int *d_order, int n_utt, void *stream);
int sea_hw64_frontend(const float *in, long L, float *hout, float *hev, float *acf_hc, float *acf_ev, float *cross_hc,
                      float *cross_ev, int *pitch, float *pratio, float *mark);
/* createIBM():79-87 on the same bank: initGroup and pitchDtm as sea_hw25_pitch_* has them (see there for the functions, the
 * outputs' meaning, d_stages' layout, d_scratch, d_order and the status word), at 64 channels, 201 delays and a hop of 160
 * (csrc/hw64_pitch_kernel.hip).  Parity: bit for bit, every stage, against the reference's own functions
 * compiled on a CPU against resyth_64sub_IBM/cpp/HuWang.h (tests/golden/hw64_pitch_golden.npz).
 * Inputs are the rows sea_hw64_correlogram_batch wrote and are not modified: d_acf_hc [rows][64][201], d_pratio_in, d_mark_in
 * [rows][64]; utterance u has lengths[u] / 160 rows from d_row_offsets[u].  There is NO d_cross_hc argument: the 25-band call
 * reads it only because leftDevelope / rightDevelope bound their chan_mark test and their number2 loop by the literal 40, which
 * on a bank of 25 reaches fifteen ghost channels in the arrays behind the frame's acf.  On this bank of 64 the same literal
 * stays inside the frame: channels 40..63 never enter chan_mark (so never chan_mark2, number or the Developes' sumAuto) and are
 * not counted in number2.  That is reproduced; a port with 64 in place of 40 computes other pitches.
 * Outputs: d_pitch [rows] ints (0 = unvoiced, else 32..200), d_grp and d_pratio [rows][64] floats, d_status [n_utt] ints with
 * the segment count in bits 0..15, SEA_HW25_TOO_MANY_SEGMENTS and SEA_HW25_CHANMARK_UNSET.  d_stages (optional): utterance u's
 * block of SEA_HW64_STAGE_WORDS words per row at word d_row_offsets[u] * SEA_HW64_STAGE_WORDS, [5][rows_u] ints then
 * [2][rows_u][64] floats, laid out as SEA_HW25_STAGE_WORDS.  d_scratch must hold sea_hw64_pitch_scratch_bytes (total_rows,
 * n_utt) bytes.  Null pointers (other than d_stages and d_order) and an output that is an input or another output are refused
 * before anything is launched; n_utt <= 0 returns 0; the lengths stay on the device, nothing synchronises with the host, every
 * launch is on `stream`.
 * The reference's undefined cases are defined as for sea_hw25_pitch_batch: no segment (always so with fewer than 3 rows):
 * segment count 0 and all outputs 0; more than 400 segments: SEA_HW25_TOO_MANY_SEGMENTS, the count, all outputs 0; chan_mark
 * read before it is set: it starts at zeros and SEA_HW25_CHANMARK_UNSET is set.  The fourth case there (ghost channels past
 * the arrays on an utterance's last frame) does not exist on this bank.
 * sea_hw64_pitch_waves_per_utterance: how many waves the two frame-walking kernels (the maximum and the findPitch / timeCrn
 * kernel) give every utterance of a batch of n_utt on the current device (wave g takes the frames g, g + G, ..); 0 on error.
 * sea_hw64_pitch: one utterance from host memory; runs the front half itself; pitch [L / 160], grp and pratio [L / 160][64],
 * status [1]; pitch, grp and pratio may be null. */
enum { SEA_HW64_STAGE_WORDS = 133 /* per row: 5 ints and 2 x 64 floats */ };
long long sea_hw64_pitch_scratch_bytes(long long total_rows, int n_utt);
int sea_hw64_pitch_waves_per_utterance(int n_utt);
int sea_hw64_pitch_batch(const float *d_acf_hc, const float *d_pratio_in, const float *d_mark_in, const long long *d_lengths,
                         const long long *d_row_offsets, int *d_pitch, float *d_grp, float *d_pratio, int *d_status, void *d_stages,
                         void *d_scratch, const int *d_order, int n_utt, void *stream);
int sea_hw64_pitch(const float *x, long L, int *pitch, float *grp, float *pratio, int *status);
/* createIBM():89-106 on the same bank: computeAM, finalSeg and the binarisation as sea_hw25_am_batch, sea_hw25_finalseg_batch and
 * sea_hw25_ibm* have them (see there for the functions, the outputs' meaning, the optional outputs, d_scratch, the status bits
 * and the parity of ratio), at 64 channels and a hop of 160 (csrc/hw64_am_kernel.hip).  After it
 * sea_hw64_ibm (x) is createIBM (x) compiled against resyth_64sub_IBM/cpp/HuWang.h.  Each call mirrors its sea_hw25_* namesake
 * argument for argument, with 64 / 160 for 25 / 80: d_gout, d_ampatt and d_am in sea_hw64_periphery_batch's layout, the frame
 * arrays [rows][64], utterance u's lengths[u] / 160 rows from d_row_offsets[u], d_stages utterance u's [SEA_HW25_FINAL_STAGES]
 * [rows_u][64] floats at float d_row_offsets[u] * SEA_HW25_FINAL_STAGES * 64.  What the constants change: WINDOW is 320, exactly
 * two hops, so frame f's window is [160 (f - 1), 160 (f + 1)); sinModel's frequency is 16000 / pitch; d_pitch holds 0 or
 * 32..200, and a pitch of 201 or more is SEA_HW25_AM_BAD_PITCH; amPatt's filter has up to 1119 taps.  The FFT's two complex
 * buffers take 2048 bytes per padded sample for 64 channels: all channels at once while that stays under 256 MiB (up to 131 072
 * padded samples), else eight groups of eight channels; total_padded_samples alone decides, and
 * sea_hw64_am_scratch_bytes shows which.  The status bits and the cases where the reference is undefined (more than
 * 150000 samples, no voiced frame, fewer than three rows, a length of 0, more than 400 segments) are those of the 25-band calls;
 * the refusals too: null pointers, and an output that is an input or another output, the status array included.  Nothing
 * synchronises with the host and every launch is on `stream`.
 * Parity (tests/golden/hw64_am_golden.npz, the reference's own functions compiled on a CPU against the 64-band header): gOut,
 * the AM pattern before and after its normalisation, sEng, AmCrn, every stage of finalSeg and the mask bit for bit; ratio to the
 * fixture's ratio_tol, and no unit of the fixture within that band of THETAE. */
long long sea_hw64_am_scratch_bytes(long long total_padded_samples, int n_utt);
int sea_hw64_am_batch(const float *d_gout, const int *d_pitch, const long long *d_offsets, const long long *d_lengths,
                      const long long *d_row_offsets, float *d_amcrn, float *d_ratio, float *d_seng, float *d_ampatt, float *d_am,
                      int *d_status, void *d_scratch, long long total_padded_samples, const int *d_order, int n_utt, void *stream);
long long sea_hw64_finalseg_scratch_bytes(long long total_rows, int n_utt);
int sea_hw64_finalseg_batch(const float *d_grp, const float *d_amcrn, const float *d_cross_ev, const float *d_pratio,
                            const long long *d_lengths, const long long *d_row_offsets, float *d_mask, float *d_grp_final,
                            int *d_status, float *d_stages, void *d_scratch, const int *d_order, int n_utt, void *stream);
long long sea_hw64_ibm_scratch_bytes(long long total_padded_samples, long long total_rows, int n_utt);
int sea_hw64_ibm_batch(const float *d_in_f32, const long long *d_offsets, const long long *d_lengths, const long long *d_row_offsets,
                       float *d_mask, int *d_pitch, int *d_status, float *d_stages, void *d_scratch, long long total_padded_samples,
                       long long total_rows, const int *d_order, int n_utt, void *stream);
int sea_hw64_ibm(const float *x, long L, float *mask, int *pitch, int *status);
/* resynthesis() on the same bank (HuWang.cpp:1498-1549 against resyth_64sub_IBM/cpp/HuWang.h; csrc/hw64_resynth_kernel.hip,
 * DESIGN.md section 5.19): the mask applied to gOut, enhanced 16 kHz audio out, which closes the chain at this bank.  Per channel
 * c = 0..63 in order, as sea_hw25_resynth* describes it: gOut[c] / midEarCoeff[c] reversed in time, gammaToneFilter again, /
 * midEarCoeff[c], reversed back; times the overlap-add weight of the frames whose unit is set (mask > threshold; NaN and -0.0 > 0
 * are not set); the 64 products added in channel order from +0.0f, every channel multiplied and added whatever its weight.
 * What the constants change: WINDOW = 320 is exactly two hops of 160, so the window IS a raised cosine: a set frame f adds
 * up160[o] on [160 (f - 1), 160 f) -- not for f = 0 -- and down160[o] on [160 f, 160 f + 160), and nothing after that.  The
 * largest index frame F - 1 writes is 160 F - 1 <= L - 1 (F = L / 160): the reference never leaves its arrays, no contribution
 * is dropped, and the reference pins every case.  The samples [160 F, L) have weight 0.
 * sea_hw64_resynth_tables_host: up160[n] = 0.5 (1 + cos (n pi / 160 + pi)) and down160[n] = 0.5 (1 + cos (n pi / 160)) in double,
 * and w640[o * 4 + bits], the float weight at position o = 0..159 of a hop, bit 0 / 1 of `bits`: frame k / k + 1 (k = the
 * sample's index / 160) exists and is set; the terms are added in that order, each a double sum rounded to float, as the
 * reference's `weight[..] +=`.  Every pointer may be null.
 * Every call here takes HOST pointers.  The batch launches on device pointers and a stream exist inside the library only; their
 * exported forms (sea_hw64_resynth_batch, sea_hw64_enhance_batch) are left to a change that also gives them their rows in the
 * table of caller's-stream tests.
 * sea_hw64_resynth / sea_hw64_enhance: one utterance, the prototypes of their sea_hw25_* namesakes: mask [F][64] with F = L / 160
 * (anything else fails); out_f32 [L]; sea_hw64_enhance's mask and pitch may be null, its status word is sea_hw64_ibm's.  L = 0 is
 * no work (status 0); L < 160 has no frame and gives zeros; more than 150000 samples: the status zeroes the mask, as in
 * sea_hw64_ibm, and the audio is zeros.  Each is the list form below on a list of one.
 * sea_hw64_resynth_utterances: n_utt utterances in[u] of lengths[u] float samples (on the int16 scale) with masks[u]
 * [lengths[u] / 160][64] (may be null where that is no row) -> out_f32[u] floats and out_i16[u], their (short) conversion as the
 * x86-64 build performs it (see sea_hw25_resynth_batch); either output array may be null as a whole, not both.  Runs the
 * periphery with gOut and then the resynthesis.
 * sea_hw64_enhance_utterances: createIBM followed by the resynthesis (threshold 0) of its own mask, from the gOut that
 * sea_hw64_ibm_batch keeps in its scratch: out_f32 / out_i16 as above; optional (null as a whole, or per utterance) masks[u]
 * [lengths[u] / 160][64] and pitch[u] [lengths[u] / 160]; status [n_utt], sea_hw64_ibm's words.
 * Both cut the list, in order and greedily, into chunks that fit HBM; every chunk is one launch group with an LPT launch order
 * of its own, and the device buffers are sized once for the largest chunk.  A chunk of n utterances with s samples (each
 * length rounded up to 8) and r rows grows while W + 10 s + 260 r + 32 n stays within the budget, W = sea_hw64_ibm_scratch_bytes
 * (s, r, n), for the resynthesis alone 768 s (the three [64][pitch] planes); an utterance that exceeds the budget alone gets a
 * chunk to itself.  The budget is 60 % of the HBM that is free at the call; SEA_HW64_ENHANCE_SCRATCH_MB (MiB) overrides it.
 * The results do not depend on the cut.  sea_hw64_enhance_plan: that cut for a given budget, without touching a device: returns
 * the number of chunks (0 for n_utt <= 0, -1 for a null or negative length) and, where cuts is not null, writes that many + 1
 * ints: the first utterance of every chunk, then n_utt.  sea_hw64_enhance_last_chunks: how many chunks the calling thread's
 * last list call completed.  sea_hw64_enhance_last_resynth_ms: the device time of that call's resynthesis launches alone, in ms,
 * summed over its chunks (a pair of device events around each launch): the launch is internal, so it cannot be timed from outside.
 * sea_hw25_resynth_text_write writes the reference's text file for either bank. */
int sea_hw64_resynth_tables_host(float *w640, double *up160, double *down160);
int sea_hw64_resynth(const float *x, long L, const float *mask, long F, float threshold, float *out_f32);
int sea_hw64_enhance(const float *x, long L, float *out_f32, float *mask, int *pitch, int *status);
int sea_hw64_resynth_utterances(const float *const *in, const long *lengths, const float *const *masks, float threshold,
                                float *const *out_f32, short *const *out_i16, int n_utt);
int sea_hw64_enhance_utterances(const float *const *in, const long *lengths, int n_utt, float *const *out_f32, short *const *out_i16,
                                float *const *masks, int *const *pitch, int *status);
int sea_hw64_enhance_plan(const long *lengths, int n_utt, long long budget_bytes, int resynth_only, int *cuts);
int sea_hw64_enhance_last_chunks(void);
double sea_hw64_enhance_last_resynth_ms(void);
/* gammaToneFilter(input, output, fChan, sigLength) for channel `chan` of the 64-band bank */
int sea_gammatone_filter(const float *input, float *output, int chan, long sigLength);

/* DoNoiseSupAlloc / DoNoiseSupInit / DoNoiseSup / DoNoiseSupDelete on a device-resident state */
typedef struct sea_ns_stream sea_ns_stream;
sea_ns_stream *sea_ns_stream_alloc(void);
void sea_ns_stream_init(sea_ns_stream *s);
/* consumes 80 float samples, returns 1 (TRUE) when out80 was produced, 0 during the latency */
int sea_ns_stream_push(sea_ns_stream *s, const float *in80, float *out80);
void sea_ns_stream_delete(sea_ns_stream *s);
/* batched form on device pointers: n_streams independent streams x nframes frames of 80 floats,
 * [stream][frame][80]; d_state holds sea_ns_state_floats() floats per stream and carries the
 * recursion from call to call (reset != 0 starts from the DoNoiseSupInit state). */
int sea_ns_streams_push(const float *d_in, float *d_out, int *d_produced, float *d_state, int n_streams,
                        int nframes, int reset, void *stream);
int sea_ns_state_floats(void);
/* the same, additionally reporting what the reference's batch plug-in shape hands back per frame
 * (esti_denoise_out of function/20141106_speech_enhancement/aurora_etsi/NoiseSupExports.h:19-27, filled by
 * etsi_denoise_mapping_func_Wiener): d_flags[stream][frame] bit 0 SpeechFoundVar, 1 Spec, 2 Mel,
 * 3 VADNS; d_frame_counter[stream][frame] = FrameCounter after the tick.  In that API's terms:
 * sea_init ~ ..._global_init, one state blob ~ ..._thread_init, one call ~ ..._func_Wiener on
 * dataNum = 80*nframes samples (this engine implements the etsi/ arithmetic, 80-sample frames). */
int sea_ns_streams_push_fd(const float *d_in, float *d_out, int *d_produced, unsigned char *d_flags,
                           int *d_frame_counter, float *d_state, int n_streams, int nframes, int reset, void *stream);

/* The 16 k-native NoiseSup variant (function/20141106_speech_enhancement/aurora_etsi/NoiseSup.cpp:1140-1407,
 * NoiseSup.h:36-53 -- 160-sample frames, window 480, NS_FFT_LENGTH 512 transformed with NS_FFT_ORDER 8, 25 gammatone-
 * shaped windows) on device pointers: n_streams independent streams x nframes frames, d_in / d_out
 * [stream][frame][160]; d_state holds sea_ns16k_state_floats() floats per stream (reset != 0: thread_init's state).
 * The frame gate of func_Wiener (:1160-1171) is applied inside.  Per frame: d_produced = outData was written;
 * d_flags (optional) bit 0 SpeechFoundVar, 1 Spec, 2 Mel, 3 VADNS and d_frame_counter (optional) = pFrameCounter, both 0
 * where the first stage did not run; d_wiener (optional) [stream][frame][25] = the gains func_Wiener prints, written
 * where produced.  Parity: see oracle/ns16k_oracle.c (transform / windows / IDCT pinned against the reference's own
 * rfft.cpp + MelProc.cpp compiled here, the frame loop unpinned). */
int sea_ns16k_streams_push(const float *d_in, float *d_out, int *d_produced, unsigned char *d_flags, int *d_frame_counter,
                           float *d_wiener, float *d_state, int n_streams, int nframes, int reset, void *stream);
int sea_ns16k_state_floats(void);
/* its host-side tables as the reference's init code lays them out (for checks against the oracle) */
int sea_ns16k_tables_host(float *sigWindow480, float *irWindow17, int *gammaStart25, float *gamma25x128, float *idct25x25);
/* and its table-driven transform schedule (the pipelined kernel's tables are built from it) run on the host, in place on
 * 512 floats: rfft (x, 512, 8) */
void sea_ns16k_fft_host(float *x512);

/* The reference's batch plug-in symbols (function/20141106_speech_enhancement/aurora_etsi/NoiseSupExports.h:35-42;
 * INSTANCE / PINSTANCE / int32s of the absent aurora/aurora_include.h = void*, void**, int), as adapters over
 * sea_init / one state blob per thread instance / sea_ns16k_streams_push (csrc/mapping.hip).  in_ins points to
 * {float *inData; int dataNum}, out_ins to {float *outData; int *pSpeechFoundVar, *pSpeechFoundSpec, *pSpeechFoundMel,
 * *pSpeechFoundVADNS, *pFrameCounter} (NoiseSupExports.h:14-27).  With sm_glb_res == NULL (the reference's caller,
 * resyth_64sub_ori/cpp/aurora_etsi_test.cpp:20) they run the 16 k-native variant the reference builds behind these
 * names: one call consumes dataNum / 160 frames, zero frames are skipped (aurora_etsi/NoiseSup.cpp:1160-1171), and
 * the FILE* argument of func_Wiener, when not NULL, receives the line of 25 gains per second-stage frame (:1319-1328).
 * sm_glb_res is ignored whatever it points to, as the reference ignores it (NoiseSup.cpp:913-922).  Extension, opt-in
 * through the environment only: SEA_MAPPING_8K=1 at global_init selects the etsi/ arithmetic on 80-sample frames
 * instead (sea_ns_streams_push_fd; nothing is printed).
 * global_init / thread_init return 1 on success, func_Wiener / func return 0. */
int etsi_denoise_mapping_global_init(void **sm_glb_pins, void *sm_glb_res);
int etsi_denoise_mapping_thread_init(void **sm_thd_pins, void *sm_glb_ins);
int etsi_denoise_mapping_func_Wiener(void *sm_glb_ins, void *sm_thd_ins, void *in_ins, void *out_ins, void *fp_Wiener);
int etsi_denoise_mapping_func(void *sm_glb_ins, void *sm_thd_ins, void *in_ins, void *out_ins);
void etsi_denoise_mapping_thread_release(void **sm_thd_pins);
void etsi_denoise_mapping_global_release(void **sm_glb_pins);

/* ----------------------------------------------------------------------------------------------
 * The DNN mask estimator: noisy audio -> 64 subband streams -> cochleagram -> feed-forward network -> mask rows ->
 * resynthesis (csrc/dnn_kernel.hip, csrc/dnn_capi.hip).  Host pointers only.  Every operation is
 * stated, and the plain-C model tests/dnn_model_driver.c reproduces every result bit for bit as values (-0 equals +0):
 *
 * Cochleagram: 20 ms frames every 10 ms on the int16 streams sea_subband64 writes.  For f < F = (L - 320) / 160 + 1 and c < 64:
 * E = the sum of s_c[160 f + n]^2 over n < 320 as an exact integer, y = (float)(E + 1) (one round-to-nearest conversion),
 * feats[f][c] = sea_lnf (y) of csrc/dnn_math.h (within 1 ulp of ln y; silence gives 0).  The rows are the mask rows of
 * sea_resynth64 with binary bit 1 clear.
 *
 * Network: context C = 0..15, K0 = 64 (2 C + 1), 1..8 layers, every dimension 1..4096, dims[0] == K0.  Input row f of an
 * utterance, for d = -C..C: x0[(d + C) 64 + c] = (feats[clamp (f + d, 0, F - 1)][c] + shift[k]) * scale[k], a float add, then a
 * float multiply (Kaldi's Splice, AddShift, Rescale); the splice never crosses an utterance.  Layer l: acc = b[j], then for k
 * ascending acc = fmaf (x[k], W[j][k], acc), W[l] row-major [out][in] as torch.nn.Linear.weight; then act[l]: 0 identity,
 * 1 the sigmoid 1.0f / (1.0f + sea_expf (-z)) (sea_expf clamps its argument to +-88), 2 z > 0 ? z : 0.
 *
 * sea_dnn_create: copies the weights to the current device once; NULL (sea_last_error says why) for a context outside 0..15,
 * dims[0] != K0, a dimension outside 1..4096, an unknown activation or a value of shift, scale, W or b that is not finite.
 * The model is used on the device it was created on.
 * sea_cochleagram64: sub64 [64][L] as sea_subband64 writes it -> feats [F][64]; L < 320 fails.
 * sea_cochleagram_utterances: sea_subband64 and the cochleagram of every utterance of a list; feats[u] [F_u][64].
 * sea_dnn_forward: feats[u] [n_rows[u]][64] -> out[u] [n_rows[u]][dims[n_layers]]; an utterance may have no row (its
 * pointers may be NULL, its output is not touched).  Features that are not finite are accepted: the operations above are
 * IEEE's on them too (a NaN through the rectifier is 0, through the sigmoid a NaN), such a value reaches the 2 C + 1 rows
 * around it within its utterance and no other row, and the C model gives the same class value for value (a NaN where a NaN
 * is, payload and sign free; otherwise the same value).
 * sea_dnn_enhance_utterances: the whole chain for a list of 16 kHz int16 utterances, on the device on one stream: subbands,
 * cochleagram, the layers, the fused resynthesis kernel with the network's output as its mask (so dims[n_layers] must be 64),
 * int16 audio out [lengths[u]]; masks (NULL as a whole or per utterance: not wanted) receives the network's output
 * [F_u][64].  binary: bit 0 as in sea_resynth64 (a unit is kept where its mask value passes the reference's threshold);
 * bit 1 is refused, the cochleagram has (L - 320) / 160 + 1 rows.  Any utterance shorter than 320 samples makes the call
 * return non-zero before the device is touched; no output is written.
 * The three list calls run in chunks of whole utterances in list order, a chunk's device footprint held to 60 % of the HBM
 * that is free (SEA_DNN_SCRATCH_MB overrides the budget; per padded sample 4 B of audio, 128 B of subbands and the
 * resynthesis scratch, per row 256 B of features, 256 B of mask and two activation rows); sea_dnn_last_chunks: how many chunks
 * the last such call of this thread ran.  Results do not depend on the cut.  There is no CPU fallback.
 * sea_dnn_last_stage_ms: the device time in ms of a stage (SEA_DNN_STAGE_*) of this thread's last
 * sea_dnn_enhance_utterances, between events on its stream, summed over the chunks; 0 for a layer the network does not have,
 * -1 for an unknown stage.  For measurement (tools/bench_extra.py --what dnn).
 * -------------------------------------------------------------------------------------------- */
typedef struct sea_dnn sea_dnn;
sea_dnn *sea_dnn_create(int context, const float *shift, const float *scale, int n_layers, const int *dims,
                        const float *const *W, const float *const *b, const int *act);
void sea_dnn_destroy(sea_dnn *m);
int sea_cochleagram64(const short *sub64, long L, float *feats);
int sea_cochleagram_utterances(const short *const *in, const long *lengths, int n_utt, float *const *feats);
int sea_dnn_forward(const sea_dnn *m, const float *const *feats, const int *n_rows, int n_utt, float *const *out);
int sea_dnn_enhance_utterances(const sea_dnn *m, const short *const *in, const long *lengths, int n_utt, int binary,
                               short *const *out, float *const *masks);
int sea_dnn_last_chunks(void);
enum {
    SEA_DNN_STAGE_SUBBAND = 0,
    SEA_DNN_STAGE_COCHLEAGRAM = 1,
    SEA_DNN_STAGE_SPLICE = 2,
    SEA_DNN_STAGE_LAYER0 = 3, /* layer l is SEA_DNN_STAGE_LAYER0 + l, l < 8 */
    SEA_DNN_STAGE_RESYNTH = 11,
    SEA_DNN_STAGE_ALL = 12, /* from before the subbands to after the resynthesis */
    SEA_DNN_STAGE_COUNT = 13
};
double sea_dnn_last_stage_ms(int stage);

/* ----------------------------------------------------------------------------------------------
 * Objective scores: enhanced audio against clean audio, an estimated mask against the ideal one (csrc/score_kernel.hip,
 * csrc/score_capi.hip).  Host pointers only.  With int16 audio every energy is an exact integer and
 * the logarithm is sea_lnf of csrc/dnn_math.h, so the plain-C model tests/score_model_driver.c reproduces every result bit
 * for bit.
 *
 * sea_score_utterances: ref[u] and est[u] hold lengths[u] samples (0 .. 2^31 - 1), hop is 80 (8 kHz) or 160 (16 kHz), a frame
 * is 2 hop samples every hop: F = L < 2 hop ? 0 : (L - 2 hop) / hop + 1 (at hop 160 the rows of the cochleagram and the
 * masks).  sums[u] = {Srr, See, Sre}: the sums of ref^2, est^2 and ref est (signed) over ALL L samples.  Per frame f < F, over
 * samples hop f .. hop f + 2 hop - 1: srr, see, sre likewise and n = srr - 2 sre + see; a frame with srr == 0 is skipped,
 * otherwise d = (sea_lnf ((float)(srr + 1)) - sea_lnf ((float)(n + 1))) * 0x1.15f2cep+2f (one conversion each, a float
 * subtract, a float multiply by the float nearest 10 / ln 10), clamped to [-10, 35].  seg_frames[u]: the frames used.
 * seg_sum[u]: p[l] = the sum over i ascending of (double) d[64 i + l] (a skipped frame adds nothing), then the sum of p[l] over
 * l = 0..63 ascending.  frame_db: NULL, or per utterance NULL or [F] floats that receive d, a skipped frame the bit pattern
 * 0x7fc00000.  SNR, SI-SDR and the segmental SNR follow from these on the host (speech_enhancement_amd/scores.py).
 * sea_mask_score_utterances: est[u] and ideal[u] [n_rows[u]][64]; a unit is on iff value > threshold, strictly (a NaN is off);
 * counts[u] = {n11, n10, n01, n00}, the units with est on / ideal on, est on / ideal off, est off / ideal on, both off.
 * Both return non-zero, with a sea_last_error message and before any device call, for n_utt < 0, a hop other than 80 or 160, a
 * threshold that is not finite, a NULL argument (frame_db excepted), a negative length or row count, a length above
 * 2^31 - 1, or a NULL buffer of an utterance that has samples or rows; the scalars are looked at first, then n_utt == 0
 * returns 0 whatever the pointers.  An utterance without samples or rows may have NULL buffers; its outputs are zeros.
 * Lists run in chunks of whole utterances in list order, a chunk's device footprint held to 60 % of the HBM that is free
 * (SEA_SCORE_SCRATCH_MB overrides the budget); sea_score_last_chunks: how many chunks the last such call of this thread ran.
 * Results do not depend on the cut.  There is no CPU fallback.
 * sea_score_last_stage_ms: the device time in ms of a kernel (SEA_SCORE_STAGE_*) in this thread's last call that ran it,
 * between events, summed over the chunks; -1 for an unknown stage.  For measurement (tools/bench_extra.py --what score).
 * -------------------------------------------------------------------------------------------- */
int sea_score_utterances(const short *const *ref, const short *const *est, const long *lengths, int n_utt, int hop,
                         long long *sums, double *seg_sum, int *seg_frames, float *const *frame_db);
int sea_mask_score_utterances(const float *const *est, const float *const *ideal, const int *n_rows, int n_utt, float t_est,
                              float t_ideal, long long *counts);
int sea_score_last_chunks(void);
enum {
    SEA_SCORE_STAGE_FRAMES = 0, /* score_frames_kernel */
    SEA_SCORE_STAGE_FINISH = 1, /* score_finish_kernel */
    SEA_SCORE_STAGE_MASK = 2,   /* mask_score_kernel */
    SEA_SCORE_STAGE_COUNT = 3
};
double sea_score_last_stage_ms(int stage);

/* ----------------------------------------------------------------------------------------------
 * STOI, the short-time objective intelligibility measure of Taal, Hendriks, Heusdens and Jensen (2011), of enhanced against
 * clean int16 audio (csrc/stoi_kernel.hip, csrc/stoi_capi.hip; the contract, operation by operation, is DESIGN.md section
 * 5.24, and the plain-C model tests/stoi_model_driver.c reproduces every result bit for bit).  Host pointers only.
 *
 * sea_stoi_utterances: ref[u] and est[u] hold lengths[u] samples (0 .. 2^31 - 1) at `rate` 16000 or 8000.  Both are resampled
 * to 10 kHz (L10 = ceil (5 L / q) samples, q = 8 or 4); frames are 256 samples every 128, F = L10 < 256 ? 0 :
 * (L10 - 256) / 128 + 1; the frames of the reference more than 40 dB below its loudest are removed from both signals, M are
 * kept; the kept frames are overlap-added and cut into M frames again, each gives 15 third-octave magnitudes; every run of 30
 * frames is a segment, S = max (M - 29, 0), and every (segment, band) a term d in [-1, 1].
 * frames_kept[u] = {F, M}; stoi_terms[u] = 15 S; stoi_sum[u]: p[l] = the sum over i ascending of (double) d[64 i + l] over the
 * flat index i = 15 s + j, then the sum of p[l] over l = 0..63 ascending.  d_out: NULL, or per utterance NULL or [S][15] floats
 * that receive d.  The figure is stoi_sum / stoi_terms, on the host (speech_enhancement_amd/scores.py).
 * Returns non-zero, with a sea_last_error message and before any device call, for n_utt < 0, a rate other than 16000 or
 * 8000, a NULL argument (d_out excepted), a negative length, a length above 2^31 - 1, or a NULL buffer of an utterance that
 * has samples; the scalars are looked at first, then n_utt == 0 returns 0 whatever the pointers.  An utterance without
 * samples may have NULL buffers; its outputs are zeros.  Lists run in chunks of whole utterances in list order, a chunk's
 * device footprint held to 60 % of the HBM that is free (SEA_SCORE_SCRATCH_MB overrides the budget); sea_stoi_last_chunks:
 * how many chunks the last call of this thread ran.  Results do not depend on the cut.  There is no CPU fallback.
 * sea_stoi_last_stage_ms: the device time in ms of a kernel (SEA_STOI_STAGE_*) in this thread's last call, between events,
 * summed over the chunks; -1 for an unknown stage.  For measurement (tools/bench_extra.py --what stoi).
 * -------------------------------------------------------------------------------------------- */
int sea_stoi_utterances(const short *const *ref, const short *const *est, const long *lengths, int n_utt, int rate,
                        double *stoi_sum, long long *stoi_terms, int *frames_kept, float *const *d_out);
int sea_stoi_last_chunks(void);
enum {
    SEA_STOI_STAGE_RESAMPLE = 0, /* stoi_resample_kernel */
    SEA_STOI_STAGE_ENERGY = 1,   /* stoi_energy_kernel */
    SEA_STOI_STAGE_COMPACT = 2,  /* stoi_compact_kernel */
    SEA_STOI_STAGE_BAND = 3,     /* stoi_band_kernel */
    SEA_STOI_STAGE_SEGMENT = 4,  /* stoi_segment_kernel */
    SEA_STOI_STAGE_FINISH = 5,   /* stoi_finish_kernel */
    SEA_STOI_STAGE_COUNT = 6
};
double sea_stoi_last_stage_ms(int stage);

/* ----------------------------------------------------------------------------------------------
 * Training that network: minibatch SGD with momentum on Kaldi nnet1's MSE, 1/2 sum e^2 (csrc/dnn_train_kernel.hip,
 * csrc/dnn_train_capi.hip).  Host pointers only, one internal stream.  The plain-C model
 * tests/dnn_train_model_driver.c reproduces every value bit for bit (-0 equals +0).  All operations are float, individually
 * rounded, never contracted; every chain starts from +0.  One step on the rows idx[0 .. B - 1] of the training set, 1 <= B <= 4096:
 *   x0[m] = the network's input row of global row idx[m] (the splice is clamped to that row's utterance); a_0 = x0 and
 *   a_l = layer l of the inference contract above, every a_l kept
 *   e = a_n - t[idx[m]];  r[m]: acc = fmaf (e[m][j], e[m][j], acc), j ascending;  p[l] = sum over i ascending of (double) r[64 i + l],
 *   loss = 0.5 * sum over l = 0..63 ascending of p[l], in double
 *   delta_n = e d(a_n);  d: sigmoid a * (1 - a) (a subtract, a multiply) and delta = e * d (one more multiply); ReLU
 *   delta = a > 0 ? e : 0; identity delta = e
 *   G_l[j][k]: acc = fmaf (delta_l[m][j], a_(l-1)[m][k], acc), m ascending 0 .. B - 1, one chain
 *   g_l[j]: acc = acc + delta_l[m][j], m ascending
 *   for l = n .. 2: E[m][k]: acc = fmaf (delta_l[m][j], W_l[j][k], acc), j ascending, W as before this step's update;
 *   delta_(l-1) = E d(a_(l-1)) by the rules above
 *   every weight and bias: v = mu * v + g (a multiply, an add), w = w - eta * v (a multiply, a subtract)
 * eta multiplies the gradient SUMMED over the minibatch, as in nnet1: a rate lr meant for the mean gradient is eta = lr / B.
 * The update is in place in the sea_dnn's device storage (its tile padding is never written), so the handle serves
 * sea_dnn_forward and sea_dnn_enhance_utterances at once.  What happens once a value stops being finite is not pinned.
 *
 * sea_dnn_trainer_create: uploads the training set once (feats[u] [n_rows[u]][64], targets[u] [n_rows[u]][dims[n_layers]]),
 * allocates the step's buffers for minibatches of at most max_batch rows and zeroes the momentum.  NULL (sea_last_error says
 * why) for a null argument, max_batch outside 1..4096, n_utt < 1, a negative n_rows[u] or no row at all -- all before the
 * device is touched -- and for a set that does not fit 60 % of the free device memory.  The model must outlive the trainer.
 * sea_dnn_trainer_run: cuts order[0 .. n_order - 1] (global rows, any length, repeats allowed) into consecutive minibatches of
 * `batch` rows, the last one shorter, runs the steps back to back and writes losses[ceil (n_order / batch)].  update = 0 is
 * evaluation: forward and loss only, no state touched.  Returns 0; 2 if any step's loss is not finite; 1, before the device is
 * touched, for a null argument, batch outside 1..4096 or above max_batch, n_order < 1, an index outside the set, eta not finite
 * or mu not in [0, 1) (the checks that need only the arguments come before any use of the trainer).
 * sea_dnn_trainer_read: the last step's values, what = SEA_DNN_TRAIN_*: ACT a_layer [B][dims[layer]], layer 0..n (B the last
 * step's rows); DELTA delta_layer [B][dims[layer]], WGRAD G_layer [dims[layer]][dims[layer - 1]], BGRAD g_layer, WMOM / BMOM the
 * momentum of W_layer / b_layer, layer 1..n.  After an evaluation only ACT is of that step.  An unknown what or layer is refused.
 * sea_dnn_get_params: the model's weights as dense [out][in] arrays and its biases, from the device.
 * sea_dnn_trainer_stage_ms: the device time in ms of a stage (SEA_DNN_TRAIN_STAGE_*) of the last step of the last run, between
 * events on the trainer's stream; 0 for a stage that step did not have, -1 for an unknown stage.  For measurement.
 * -------------------------------------------------------------------------------------------- */
typedef struct sea_dnn_trainer sea_dnn_trainer;
enum { SEA_DNN_TRAIN_ACT = 0, SEA_DNN_TRAIN_DELTA = 1, SEA_DNN_TRAIN_WGRAD = 2, SEA_DNN_TRAIN_BGRAD = 3, SEA_DNN_TRAIN_WMOM = 4,
       SEA_DNN_TRAIN_BMOM = 5 };
enum {
    SEA_DNN_TRAIN_STAGE_GATHER = 0,
    SEA_DNN_TRAIN_STAGE_FORWARD0 = 1, /* layer l (1..n) is SEA_DNN_TRAIN_STAGE_FORWARD0 + l - 1 */
    SEA_DNN_TRAIN_STAGE_DELTA = 9,    /* the output delta and the loss */
    SEA_DNN_TRAIN_STAGE_DGRAD0 = 10,  /* delta_l -> delta_(l-1), l = 2..n, is SEA_DNN_TRAIN_STAGE_DGRAD0 + l - 1 */
    SEA_DNN_TRAIN_STAGE_WGRAD0 = 18,  /* G_l and g_l, l = 1..n, is SEA_DNN_TRAIN_STAGE_WGRAD0 + l - 1 */
    SEA_DNN_TRAIN_STAGE_UPDATE = 26,
    SEA_DNN_TRAIN_STAGE_ALL = 27,
    SEA_DNN_TRAIN_STAGE_COUNT = 28
};
sea_dnn_trainer *sea_dnn_trainer_create(sea_dnn *m, const float *const *feats, const float *const *targets, const int *n_rows,
                                        int n_utt, int max_batch);
void sea_dnn_trainer_destroy(sea_dnn_trainer *t);
int sea_dnn_trainer_run(sea_dnn_trainer *t, const long long *order, long long n_order, int batch, float eta, float mu, int update,
                        double *losses);
int sea_dnn_trainer_read(const sea_dnn_trainer *t, int what, int layer, float *out);
int sea_dnn_get_params(const sea_dnn *m, float *const *weights, float *const *biases);
double sea_dnn_trainer_stage_ms(const sea_dnn_trainer *t, int stage);

/* ----------------------------------------------------------------------------------------------
 * device self-tests of the places where a kernel takes a cheaper route than the reference's
 * literal arithmetic (each proven or guarded, see csrc/sea_device.h, csrc/ns_core.h and DESIGN.md section 3)
 * -------------------------------------------------------------------------------------------- */
/* all 2^32 floats s: (float)((double)s * (1/sqrt2)) vs (float)((double)s / sqrt2); count of differences */
int sea_selftest_pi4(unsigned long long *n_mismatch);
/* the resynthesis kernels' 3-instruction division by the per-channel middle-ear gain: every float
 * inside its domain (2^-100 <= |a| <= 2^100) x all 64 divisors against the IEEE quotient.
 * out2[0] = mismatches, out2[1] = patterns tested per divisor */
int sea_selftest_div(unsigned long long *out2);
/* the NoiseSup gain / noise-tracking divisions inside their per-frame guarded domain (csrc/ns_core.h, ns_div:
 * the compiler's IEEE sequence without v_div_scale / v_div_fixup, reciprocal shared per denominator) against
 * plain division on 2^30 pseudo-random + edge-mantissa operand pairs spanning the domain, and the double
 * reciprocal of the noise update.  out4[0] = pairs tested, out4[1] = float mismatches, out4[2] = double;
 * out4[3] = mismatches of the lean correctly rounded square root used in the same domain (ns_sqrt_fast: the
 * sqrtf expansion without its tiny-argument scaling) against sqrtf over EVERY float in [2^-96, 2^126] and 0 */
int sea_selftest_nsdiv(unsigned long long *out4);
/* DC-offset recurrence on ncases frames of 80 differences (host pointers): output and whether the
 * exact double path had to be taken */
int sea_selftest_dc(const float *dif, const float *y0, float *out, int *fellback, int ncases);
/* the kernels' own double-precision natural log (positive normal arguments) on n floats (host pointers) */
int sea_selftest_log(const float *x, double *ln_out, int n);
/* the guard around that log (csrc/ns_core.h, ns_near_float_boundary): both call sites round a double expression
 * of the log to float (NoiseSup.c:391, :607); when the expression lands within a few ulps of a float rounding
 * boundary the log is redone in double-double arithmetic (site 2: through the fdlibm log10 formula glibc uses).
 *   sea_selftest_log_dd     the double-double log itself on n doubles (host pointers): hi + lo
 *   sea_selftest_log_sites  both complete sites on n floats: site1 = VAD frame log-energy of frameSum = x
 *                           (x >= 64), site2 = averSNR of x (x > 1e-5); NaN outside a site's range
 *   sea_selftest_log_guard  sweeps EVERY float argument of site 1 (every finite float >= 64) or 2 (every float > 1e-5) through
 *                           the fast AND the slow form: stats8 = {arguments, guard hits, hits where the slow form
 *                           changed the float, hits recorded, arguments outside the guard window on which the two
 *                           forms disagree (must be 0), 0, 0, 0}; hits3 receives up to cap triples (argument, fast
 *                           float, returned float) */
int sea_selftest_log_dd(const double *x, double *hi, double *lo, int n);
int sea_selftest_log_sites(const float *x, float *site1, float *site2, int n);
int sea_selftest_log_guard(int site, unsigned long long *stats8, float *hits3, int cap);
/* the lane form of both sites (csrc/ns_core.h, ns_log_lanes_request / ns_log_lanes_take: one logarithm per lane, the site chosen per
 * lane, one ballot for the guard), which the dense six-wave kernel runs on the VAD sums of two beats at once, against the two
 * complete sites above, bit for bit, on EVERY float argument either site can see.  A wave takes two neighbouring arguments per pass;
 * all_vad = 0: as site 1 in lanes 0, 1 and as site 2 in lanes 2, 3 (four different logarithms per pass), all_vad != 0: as site 1 alone.
 * stats8 = {arguments of site 1, of site 2, guard hits of site 1, of site 2, results or guard flags that differ from the complete
 * site's for site 1, for site 2 (both must be 0), passes that went through the slow branch, 0} */
int sea_selftest_log_lanes(int all_vad, unsigned long long *stats8);
/* the same three logarithm forms as the kernels that take the caller's floats instantiate them (sea_ns_stream_push, sea_ns_streams_push,
 * sea_ns_streams_push_fd, sea_ns16k_streams_push, sea_compceps_frames): the exponent field is tested first, +Inf gives +Inf, a NaN
 * (and -Inf) gives NaN, as libm's log does; every other argument goes the way of sea_selftest_log_sites.  n floats of any bit
 * pattern (host pointers): site1 / site2 as in sea_selftest_log_sites without its range selection, logf = (float)log((double)x) */
int sea_selftest_log_nonfinite(const float *x, float *site1, float *site2, float *logf, int n);
/* host pipelines (csrc/hostpipe.hip): from the nth hipEventQuery of the process on, every query reports a device fault
 * (0: off).  The pipelines must then return 1 -- the reference's fault code -- instead of polling for ever. */
int sea_selftest_hostpipe_fault(long long nth_query);
/* the 16 k-native variant's pieces that the reference's own rfft.cpp + MelProc.cpp pin (tests/golden/aurora_golden.npz), run on
 * the device by the very functions the pipelined kernel calls (host pointers): rfft (x, 512, 8) of nfft frames from both of the
 * transform wave's work areas ([nfft][512] each), DoGamma of ngain vectors of 129 gains ([ngain][25]) and rows 0..8 of
 * DoGammaIDCT of those ([ngain][9], before the filter window) */
int sea_selftest_ns16k_pieces(const float *frames512, int nfft, float *fft512_a, float *fft512_b, const float *gains129, int ngain,
                              float *gamma25, float *idct9);

#ifdef __cplusplus
}
#endif
#endif
