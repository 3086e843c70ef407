/*
 * sea_kernels.h -- kernel argument blocks and launch prototypes (internal to the library).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sea_tables.h"

namespace sea {

/* Batch of utterances packed in one int16 buffer.  offsets[u] (in samples, multiple of 8) locates
 * utterance u in `in`, `out` and `out_f32`; lengths[u] is its sample count. */
struct NsBatchArgs {
    const int16_t *in;
    int16_t *out;
    float *out_f32;            /* optional: float NoiseSup output stream, same indexing as out */
    const long long *offsets;
    const long long *lengths;
    const int *order;          /* optional: block b processes utterance order[b] (longest first) */
    int *first_out;            /* optional: per utterance, frame index of the first NS output (-1: none) */
    const sea_ns_tables *tables;
    int n_utt;
    /* frame-dropping VAD inputs (ns_denoise_pipe_fd_kernel only): */
    unsigned char *flags_out;  /* per output frame fo of utterance u, at [offsets[u]/8 + 10*fo]: bit 0 SpeechFoundVar,
                                * 1 Spec, 2 Mel, 3 VADNS of the tick that produced the frame */
    int *onset_out;            /* per utterance: index of the first non-zero frame (number of frames if none) */
    int prio_row;              /* > 0: workgroups [k * prio_row, (k+1) * prio_row) get issue priority 3 - k - prio_base (four-wave form only) */
    int prio_base;             /* rows to skip: a later chunk of a batch launched in pieces (hostpipe.hip) starts below the first */
    /* An utterance processed in TIME SLICES, one launch per slice (four-wave forms): state != nullptr
     * makes every workgroup store its recursion at the end of the launch -- kNsPipeStateFloats floats at state + u * that --
     * and, with resume != 0, start from what the previous slice stored instead of DoNoiseSupInit's state.  in / out /
     * offsets / lengths describe the slice; frame_base = frames of the utterance before this slice (first_out is absolute). */
    float *state;
    int resume;
    int frame_base;
    int perm6;                 /* six-wave form: wave -> role map, three bits per wave, wave 0 lowest (0: the kernel's default) */
};
/* [2 x 640 stage buffers as 8-slot rings][12 x 64 per-lane spectra: noise, den, previous PSD of (lane, 64) x 2 stages]
 * [8 frame energies][8 denSigSE1 sums][8 speech-flag words][40 scalars] */
constexpr int kNsPipeStateFloats = 2 * 640 + 12 * 64 + 3 * 8 + 40;

/* The ETSI wideband (16 kHz) mode (wb_kernel.hip; include/sea_mi355x.h, sea_wb_denoise_batch).  Utterance u occupies
 * samples [offsets[u], offsets[u] + lengths[u]) of `in` at 16 kHz; everything at the 8 kHz rate (the two QMF streams,
 * the low-band outputs) sits at offsets[u] / 2, frame f of 80 samples at offsets[u] / 2 + 80 f. */
struct WbQmfArgs {
    const int16_t *in;
    const long long *offsets;
    const long long *lengths;
    float *lp, *hp;            /* QMF low band / high band shifted down to 0-4 kHz */
    int *onset;                /* per utterance, preset to INT_MAX: atomicMin of the indices of the non-zero frames */
    const sea_wb_tables *tables;
    int n_utt;
};
__global__ void wb_qmf_kernel(WbQmfArgs a); /* blockIdx.x = utterance, blockIdx.y strides over its frames */
constexpr int kWbQmfThreads = 128;
/* the low-band frame loop: a pipelined NoiseSup form with a FLOAT intake (the QMF low band) and no zero-frame gate --
 * frames before onset[u] advance nothing, every later one runs (ns_pipe_kernel.hip) */
struct NsWbArgs {
    NsBatchArgs b;             /* in unused; out / out_f32 / first_out / onset_out as for the int16 forms, at the 8 kHz rate */
    const float *in_f32;       /* WbQmfArgs::lp */
    const int *onset;          /* WbQmfArgs::onset (values beyond the frame count: no non-zero frame) */
};
__global__ void ns_denoise_pipe_wb_kernel(NsWbArgs a);     /* transform address tables in VGPRs, four workgroups per CU */
/* + the speech flags of the frame-dropping VAD: b.flags_out holds ONE BYTE PER PER-FRAME ROW (row ceil(offsets[u] / 160) + f,
 * as WbHbArgs below), bits as NsBatchArgs::flags_out; b.onset_out is the plain form's */
__global__ void ns_denoise_pipe_wb_fd_kernel(NsWbArgs a);
/* the high band's features per output frame: rows of 3 band energies and of 9 code values; the row of frame f of utterance
 * u is ceil(offsets[u] / 160) + f */
struct WbHbArgs {
    const float *lp, *hp;      /* the QMF streams */
    const long long *offsets;
    const long long *lengths;
    const int *onset;          /* WbQmfArgs::onset */
    float *hp_rows;            /* [rows][3] */
    float *code_rows;          /* [rows][9] */
    const sea_ns_tables *ns;   /* transform schedule and Hanning window */
    const sea_wb_tables *wb;
    int n_utt;
};
__global__ void wb_hb_kernel(WbHbArgs a);      /* blockIdx.x = utterance, blockIdx.y strides over its output frames; one wave */
__global__ void wb_specsub_kernel(WbHbArgs a); /* one lane per utterance */

/* The wideband mode in TIME SLICES (include/sea_mi355x.h, sea_wb_denoise_batch_slice): what one utterance carries from the
 * launches of one slice to those of the next, kWbSliceStateFloats floats at state + u * that, integers as their bit patterns:
 *   [0, kNsPipeStateFloats)   the low-band frame loop's blob, laid out and carried as NsBatchArgs::state
 *   kWbStQmf   117 floats     the QMF delay line: the last 117 raw input samples before the next slice's first frame
 *   kWbStOnset   1 int        ABSOLUTE index of the first non-zero frame (kWbNoOnset while there has been none); once found,
 *                             no later slice replaces it
 *   kWbStLp    400 floats     the last five frames of the QMF low band (the high band's window of output frame F starts at
 *                             sample 60 of low-band frame F - 5) ...
 *   kWbStHp    400 floats     ... and of the QMF high band (read from frame F - 4 on); both are SHIFTED by the slice's frames,
 *                             so a slice of a single frame keeps the four before it
 *   kWbStSub     8 floats     DoSpecSub16k's tracker: noise[3], meanEn, nbSpeech (int), hangOver (int), the count of
 *                             second-stage frames so far (int), one unused
 * A slice's launches only READ the parts beyond the frame loop's blob (with resume != 0; nothing is read of a first slice's
 * state); its last launch, wb_slice_end_kernel, writes them all, so the workgroups that stride over a slice's frames never
 * race with a store.  Each slice's kernels find the onset among the slice's own frames in the scratch, as absolute indices,
 * and every reader takes the smaller of that and the carried one. */
constexpr int kWbStQmf = kNsPipeStateFloats;
constexpr int kWbStOnset = kWbStQmf + 117;
constexpr int kWbStLp = kWbStOnset + 3; /* 16-byte aligned */
constexpr int kWbStHp = kWbStLp + 5 * 80;
constexpr int kWbStSub = kWbStHp + 5 * 80;
constexpr int kWbSliceStateFloats = kWbStSub + 8;
constexpr int kWbNoOnset = 0x7f7f7f7f; /* what the scratch's onset is preset to: beyond any frame count */
struct WbSliceArgs {
    WbQmfArgs q;               /* the slice's input, packed like a batch of its own; q.onset: the scratch's, ABSOLUTE indices */
    float *hp_rows;            /* optional, with code_rows: the slice's rows */
    float *code_rows;
    const sea_ns_tables *ns;
    float *state;              /* [n_utt][kWbSliceStateFloats] */
    int frame_base;            /* frames of 160 samples of every utterance before this slice */
    int resume;                /* 0: first slice, the state is not read */
};
__global__ void wb_qmf_slice_kernel(WbSliceArgs a);   /* as wb_qmf_kernel; the delay line of frame 0 comes from the state */
__global__ void ns_denoise_pipe_wb_slice_kernel(NsWbArgs a); /* b.state with the stride kWbSliceStateFloats; onset absolute */
/* + the speech flags, one byte per per-frame row of the SLICE (b.flags_out); the measures' seven floats ride in the blob's
 * scalars 14..20, which the plain slice form leaves alone */
__global__ void ns_denoise_pipe_wb_fd_slice_kernel(NsWbArgs a);
__global__ void wb_hb_slice_kernel(WbSliceArgs a);    /* as wb_hb_kernel; frames before the slice come from the state */
__global__ void wb_slice_end_kernel(WbSliceArgs a);   /* one workgroup of 128 per utterance: DoSpecSub16k over the slice's rows, then
                                                       * the state's wideband parts for the next slice */

/* B independent streams, nframes frames of 80 floats each, state blobs of kNsStateFloats floats */
constexpr int kNsStateFloats = 2 * 320 + 12 * 64 + 32;
struct NsStreamArgs {
    const float *in;           /* [B][nframes][80] */
    float *out;                /* [B][nframes][80], written where produced */
    int *produced;             /* [B][nframes] */
    float *state;              /* [B][kNsStateFloats] */
    const sea_ns_tables *tables;
    int nframes;
    int reset;                 /* 1: start from DoNoiseSupInit state instead of loading */
    unsigned char *flags;      /* optional [B][nframes]: bit 0 SpeechFoundVar, 1 Spec, 2 Mel, 3 VADNS of the tick */
    int *frame_counter;        /* optional [B][nframes]: FEParamsX::FrameCounter after the tick */
};

/* the 16 k-native variant (ns16k_pipe_kernel.hip): B independent streams, nframes frames of 160 floats each */
constexpr int kNs16StateFloats = 2 * SEA16_BUF + 6 * 132 + 32;
struct Ns16StreamArgs {
    const float *in;           /* [B][nframes][160] */
    float *out;                /* [B][nframes][160], written where produced */
    int *produced;             /* [B][nframes]: the second stage ran (outData was written) */
    unsigned char *flags;      /* optional [B][nframes]: bit 0 SpeechFoundVar, 1 Spec, 2 Mel, 3 VADNS; 0 where the first stage did not run */
    int *frame_counter;        /* optional [B][nframes]: pFrameCounter, 0 where the first stage did not run */
    float *wiener;             /* optional [B][nframes][25]: the gains func_Wiener prints, written where produced */
    float *state;              /* [B][kNs16StateFloats] */
    const sea_ns16k_tables *tables;
    int nframes;
    int reset;
    int n_streams;
};

struct CepsArgs {
    const float *den_f32;      /* float NoiseSup stream written by sea_ns_denoise_batch */
    const long long *offsets;  /* as above */
    const long long *lengths;
    const int *first_out;
    const long long *ceps_cum; /* n_utt+1 prefix sums of the per-utterance frame capacity */
    float *ceps;               /* [ceps_cum[n_utt]][14] */
    int *n_ceps;               /* optional: valid cepstral frames per utterance */
    const sea_cc_tables *tables;
    int n_utt;
};

/* the wideband CompCeps: the 8 kHz one on the low band's float stream + the decoded / subtracted high bands, 26-band DCT */
struct WbCepsArgs {
    CepsArgs c;                /* den_f32 at offsets[u] / 2; lengths in 16 kHz samples; first_out in frames of 160 */
    const float *hp_rows, *code_rows;
    const sea_wb_tables *wb;
};
__global__ void compceps_wb_kernel(WbCepsArgs a);

/* WaveProc -> CompCeps -> PostProc -> VAD (+ flush) on the float NoiseSup stream */
struct AfeArgs {
    const float *den_f32;          /* float NoiseSup stream (ns_denoise_pipe_fd_kernel) */
    const unsigned char *flags;    /* its speech flags, [offsets[u]/8 + 10*fo] */
    const long long *offsets;
    const long long *lengths;
    const int *first_out;          /* frame index of the first NoiseSup output, -1: none */
    const int *onset;              /* index of the first non-zero frame */
    const long long *ceps_cum;     /* n_utt+1 prefix sums of cepstral-frame capacities (>= lengths/80 - 6) */
    float *feat_cc;                /* [ceps_cum[n_utt]][14]: after WaveProc + CompCeps */
    float *feat_pp;                /* optional, same shape: after PostProc */
    const long long *feat_cum;     /* n_utt+1 prefix sums of emitted-frame capacities (>= lengths/80 + 6) */
    float *feat15;                 /* [feat_cum[n_utt]][15]: emitted feature frames + VAD flag */
    int *n_feat;                   /* emitted frames per utterance */
    int *n_ceps;                   /* optional */
    const sea_cc_tables *tables;
    int n_utt;
};

/* the same chain in the wideband mode: a.den_f32 at offsets[u] / 2, a.lengths in 16 kHz samples, a.first_out / a.onset in frames
 * of 160 (capacities >= lengths/160 - 6 and >= lengths/160 + 6), a.flags one byte per per-frame row (NsWbArgs above) */
struct WbAfeArgs {
    AfeArgs a;
    const float *hp_rows, *code_rows; /* WbHbArgs: read by afe_wb_ceps_kernel as compceps_wb_kernel reads them */
    const sea_wb_tables *wb;
};
__global__ void afe_wb_ceps_kernel(WbAfeArgs a); /* WaveProc + the 26-band CompCeps */
__global__ void afe_wb_vad_kernel(AfeArgs a);    /* PostProc + frame-dropping VAD + flush on frames of 160 samples */

/* The wideband feature chain over one TIME SLICE (afe_slice_kernel.hip, AfeSliceRate<true>; include/sea_mi355x.h,
 * sea_wb_afe_features_batch_slice).  Every buffer of w describes the slice as sea_wb_denoise_batch_slice_fd leaves it; first_out
 * and onset are absolute.  Cepstral frame j of an utterance with first output f0 completes with output frame f0 + j + 2, so the
 * frames that complete in a slice [fb, fb + n) are j in [max(0, fb - f0 - 2), fb + n - f0 - 2).  What one utterance carries,
 * kWbAfeStateFloats floats at state + u * that, integers as their bit patterns:
 *   kAfStF32   240 floats   the last three frames of the low band's float stream (a frame reads from sample 80 (f0 + j) - 1 on:
 *                           two frames and one sample before the slice), SHIFTED by the slice's frames as kWbStLp is
 *   kAfStHp    2 x 3        the high-band rows of the last two frames ...
 *   kAfStCode  2 x 9        ... and their code rows (frame j reads the rows of frame f0 + j, not f0 + j + 2)
 *   kAfStRing  7 x 16       DoVADProc's ring of feature frames, column 14 the speech flag
 *   kAfStLane  2 x 16       weightLMS[12] | FeatureBuffer[15]
 *   kAfStScal  8 ints       focus, hangOver, hCount, vCount, frameCounter, cepstral frames so far, null vectors so far, flushed
 *                           The last three are DIAGNOSTIC ONLY, kept for whoever inspects a state: no kernel decides anything by
 *                           them.  Where a slice starts follows from frame_base, first_out and onset alone, and a caller that
 *                           sets d_final twice for an utterance gets DoVADFlush's six rows twice.
 * afe_wb_ceps_slice_kernel strides over the slice's tiles and only READS the state; afe_wb_vad_slice_kernel, one wave per
 * utterance, writes all of it after its reads. */
constexpr int kAfStF32 = 0;
constexpr int kAfStKeep = 3 * 80;
constexpr int kAfStHp = kAfStF32 + kAfStKeep;
constexpr int kAfStCode = kAfStHp + 8;
constexpr int kAfStRing = kAfStCode + 24;
constexpr int kAfStLane = kAfStRing + 7 * 16;
constexpr int kAfStScal = kAfStLane + 2 * 16;
constexpr int kWbAfeStateFloats = kAfStScal + 8;
struct WbAfeSliceArgs {
    WbAfeArgs w;                /* w.a.flags / w.hp_rows / w.code_rows: the slice's rows; w.a.n_feat / n_ceps: the slice's counts */
    const unsigned char *final; /* optional, per utterance: non-zero = DoVADFlush after this slice */
    float *state;               /* [n_utt][kWbAfeStateFloats] */
    int frame_base;
    int resume;
};
__global__ void afe_wb_ceps_slice_kernel(WbAfeSliceArgs s); /* WaveProc + the 26-band CompCeps of the frames completing in the slice */
__global__ void afe_wb_vad_slice_kernel(WbAfeSliceArgs s);  /* nulls, PostProc + VAD, flush where final; then the state */

/* The 8 kHz feature chain over one TIME SLICE (afe_slice_kernel.hip, AfeSliceRate<false>; include/sea_mi355x.h,
 * sea_afe_features_batch_slice): the same kernel text as the wideband slice form above, without the high-band and code rows.
 * Every buffer of a describes the slice as sea_ns_denoise_batch_slice_fd leaves it (den_f32 at offsets[u], the flag byte of the slice's frame f at offsets[u]/8 + 10 f);
 * first_out and onset are absolute.  What one utterance carries, kAfeStateFloats floats at state + u * that, integers as their
 * bit patterns:
 *   kAf8StF32   240 floats  the last three frames of the float stream, SHIFTED by the slice's frames (kAfStKeep of them)
 *   kAf8StRing  7 x 16      DoVADProc's ring of feature frames, column 14 the speech flag
 *   kAf8StLane  2 x 16      weightLMS[12] | FeatureBuffer[15]
 *   kAf8StScal  8 ints      focus, hangOver, hCount, vCount, frameCounter, then cepstral frames so far, null vectors so far,
 *                           flushed: the last three DIAGNOSTIC ONLY, as in the wideband state
 * afe_ceps_slice_kernel strides over the slice's tiles and only READS the state; afe_vad_slice_kernel, one wave per utterance
 * and the slice's last launch, writes all of it after its reads. */
constexpr int kAf8StF32 = 0;
constexpr int kAf8StRing = kAf8StF32 + kAfStKeep;
constexpr int kAf8StLane = kAf8StRing + 7 * 16;
constexpr int kAf8StScal = kAf8StLane + 2 * 16;
constexpr int kAfeStateFloats = kAf8StScal + 8;
struct AfeSliceArgs {
    AfeArgs a;                  /* a.flags: the slice's bytes; a.n_feat / a.n_ceps: the slice's counts */
    const unsigned char *final; /* optional, per utterance: non-zero = DoVADFlush after this slice */
    float *state;               /* [n_utt][kAfeStateFloats] */
    int frame_base;
    int resume;
};
__global__ void afe_ceps_slice_kernel(AfeSliceArgs s); /* WaveProc + CompCeps of the frames completing in the slice */
__global__ void afe_vad_slice_kernel(AfeSliceArgs s);  /* nulls, PostProc + VAD, flush where final; then the state */

/* The plain CompCeps (no WaveProc) over one TIME SLICE, both rates (cc_slice_kernel.hip; include/sea_mi355x.h,
 * sea_compceps_batch_slice / sea_wb_compceps_batch_slice).  c.den_f32 / c.offsets / c.lengths (and the rows) describe the slice as
 * the matching *_denoise_batch_slice call leaves it; c.first_out is absolute; c.ceps_cum / c.ceps / c.n_ceps are the slice's
 * (capacity per utterance >= the slice's frames).  The frames that complete in a slice are afe_slice_span's.  What one utterance
 * carries, kCcStateFloats (8 kHz) or kWbCcStateFloats (wideband) floats at state + u * that:
 *   kCcStF32   240 floats   the last three frames of the float stream, SHIFTED by the slice's frames (kAfStKeep of them; a tile
 *                           reads at most two frames and one sample before the slice)
 *   kCcStHp    2 x 3        wideband: the high-band rows of the last two frames ...
 *   kCcStCode  2 x 9        ... and their code rows
 * The tile kernels stride over the slice's tiles with many workgroups per utterance and only READ the state;
 * compceps_carry_slice_kernel, one wave per utterance and the slice's last launch, writes the counts and the state. */
constexpr int kCcStF32 = 0;
constexpr int kCcStateFloats = kCcStF32 + kAfStKeep;
constexpr int kCcStHp = kCcStateFloats;
constexpr int kCcStCode = kCcStHp + 8;
constexpr int kWbCcStateFloats = kCcStCode + 24;
struct CcSliceArgs {
    CepsArgs c;
    const float *hp_rows, *code_rows; /* wideband: the slice's rows (WbHbArgs); nullptr at 8 kHz */
    const sea_wb_tables *wb;
    float *state;               /* [n_utt][stride] */
    int stride;                 /* kCcStateFloats or kWbCcStateFloats */
    int frame_base;
    int resume;
};
__global__ void compceps_slice_kernel(CcSliceArgs s);       /* the 8 kHz tiles of the frames completing in the slice */
__global__ void compceps_wb_slice_kernel(CcSliceArgs s);    /* the wideband ones */
__global__ void compceps_carry_slice_kernel(CcSliceArgs s); /* counts, then the state; hp_rows != nullptr: the wideband state */

struct ResynthArgs {
    const int16_t *in;
    int16_t *out;
    const long long *offsets;      /* samples, multiple of 8 */
    const long long *lengths;
    const float *mask;             /* rows of 64 floats */
    const long long *mask_offsets; /* in rows */
    float *inter;                  /* intermediate [sum(lengths padded)][64] floats */
    const int *order;
    const sea_gt_tables *tables;
    int n_utt;
    int binary;
};

/* subbband(): utterance u's 64 int16 streams form a [64][pitch] block at out + offsets[u]*64,
 * pitch = lengths[u] rounded up to 8 samples */
struct SubbandArgs {
    const int16_t *in;
    int16_t *out;
    const long long *offsets;
    const long long *lengths;
    const int *order;
    const sea_gt_tables *tables;
    int n_utt;
};

/* IRM target from the subband streams of the clean and the noise signal (irm_kernel.hip) */
struct IrmArgs {
    const int16_t *pure, *noise;   /* [64][pitch] blocks at offsets[u] * 64, pitch = lengths[u] rounded up to 8 */
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;  /* first mask row of utterance u; rows = (lengths[u] - 320) / 160 + 1 */
    float *irm;                    /* [rows][64] */
    const sea_fft_tables *fft;
    int n_utt;
    int window;                    /* 0 rectangular, 1 Hamming, 2 Hanning */
};
__global__ void irm_target_kernel(IrmArgs a); /* per-lane codelet, lane = (polyphase component, frame) */

/* The Hu-Wang estimator's front half on the 25-channel 8 kHz bank (hw25_kernel.hip).  in: packed float samples on the int16
 * scale, utterance u at in + offsets[u] (offsets multiples of 8, `pitch` floats readable); hout / hev: utterance u's
 * [25][pitch] block at offsets[u] * 25, pitch = lengths[u] rounded up to 8; the frame outputs are rows, utterance u's
 * lengths[u] / 80 rows starting at row_offsets[u]: acf_* [rows][25][101] (either may be null: not written), cross_*, pratio,
 * mark [rows][25], pitch [rows]. */
struct Hw25Args {
    const float *in;
    float *hout, *hev;
    float *gout; /* the periphery kernel: gOut in hout's layout, or null: not written */
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *acf_hc, *acf_ev;
    float *cross_hc, *cross_ev;
    int *pitch;
    float *pratio, *mark;
    const int *order;
    const sea_hw25_tables *tables;
    int n_utt;
};
__global__ void hw25_periphery_kernel(Hw25Args a);   /* grid n_utt x 64 threads */
__global__ void hw25_lowpass_kernel(Hw25Args a);     /* grid (n_utt, 25) x 256 */
__global__ void hw25_correlogram_kernel(Hw25Args a); /* grid (n_utt, G) x 256: workgroup (u, g) takes frames g, g + G, ... */

/* The same front half at 16 kHz on the 64-channel bank (hw64_kernel.hip).  Hw25Args's layout at 64 channels: hout / hev / gout
 * hold utterance u's [64][pitch] block at offsets[u] * 64; utterance u has lengths[u] / 160 rows from row_offsets[u]: acf_*
 * [rows][64][201] (either may be null: not written), cross_*, pratio, mark [rows][64], pitch [rows]. */
struct Hw64Args {
    const float *in;
    float *hout, *hev;
    float *gout; /* the periphery kernel: gOut in hout's layout, or null: not written */
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *acf_hc, *acf_ev;
    float *cross_hc, *cross_ev;
    int *pitch;
    float *pratio, *mark;
    const int *order;
    const sea_hw64_tables *tables;
    int n_utt;
};
constexpr int kHw64CorrThreads = 512;                 /* seven waves of (stream, delay) lanes and one that follows them */
__global__ void hw64_periphery_kernel(Hw64Args a);   /* grid n_utt x 64 threads */
__global__ void hw64_lowpass_kernel(Hw64Args a);     /* grid (n_utt, 64) x 256 */
__global__ void hw64_correlogram_kernel(Hw64Args a); /* grid (n_utt, G) x 512: workgroup (u, g) takes frames g, g + G, ... */

/* The Hu-Wang estimator's initial grouping and pitch tracking (hw25_pitch_kernel.hip).  Rows as Hw25Args has them: acf
 * [rows][25][101], cross, pratio_in, mark_in [rows][25] are the front half's and only read; pitch [rows], grp and pratio
 * [rows][25], status [n_utt] are written.  stages (or null): utterance u's block of SEA_HW25_STAGE_WORDS words per row at
 * row_offsets[u] * SEA_HW25_STAGE_WORDS, [5][F] ints then [2][F][25] floats.  Scratch: rowscr, utterance u's block of
 * SEA_HW25_SCRATCH_WORDS words per row at row_offsets[u] * SEA_HW25_SCRATCH_WORDS; segse [n_utt][2][400] ints. */
struct Hw25PitchArgs {
    const float *acf, *cross, *pratio_in, *mark_in;
    const long long *lengths;
    const long long *row_offsets;
    int *pitch;
    float *grp, *pratio;
    int *status;
    int *stages;
    int *rowscr, *segse;
    const int *order;
    int n_utt;
    int mode;    /* frame kernel: SEA_HW25_FRAME_FIND | SEA_HW25_FRAME_TIMECRN */
    int stage;   /* the stage slot the launch fills (frame kernel: Pitch 0 / 1; regroup kernel: Grp 1, or -1 for none) */
    float theta; /* regroup kernel */
};
#define SEA_HW25_SCRATCH_WORDS 76 /* per row: lab, key, mraw [25] and buf */
#define SEA_HW25_FRAME_FIND 1
#define SEA_HW25_FRAME_TIMECRN 2
__global__ void hw25_pitch_max_kernel(Hw25PitchArgs a);     /* grid (n_utt, G) x 64: wave (u, g) takes frames g, g + G, ... */
__global__ void hw25_pitch_segment_kernel(Hw25PitchArgs a); /* grid n_utt x 64 */
__global__ void hw25_pitch_frame_kernel(Hw25PitchArgs a);   /* grid (n_utt, G) x 64 */
__global__ void hw25_pitch_regroup_kernel(Hw25PitchArgs a); /* grid n_utt x 64 */
__global__ void hw25_pitch_track_kernel(Hw25PitchArgs a);   /* grid n_utt x 64 */

/* The same stage at 16 kHz on the 64-channel bank (hw64_pitch_kernel.hip).  Hw25PitchArgs's layout at 64 channels and 201
 * delays, without cross, which nothing reads on this bank: acf [rows][64][201], pratio_in, mark_in [rows][64] only read; pitch
 * [rows], grp and pratio [rows][64], status [n_utt] written; utterance u has lengths[u] / 160 rows from row_offsets[u].  stages
 * (or null): SEA_HW64_STAGE_WORDS words per row, [5][F] ints then [2][F][64] floats.  Scratch: rowscr, SEA_HW64_SCRATCH_WORDS
 * words per row; segse [n_utt][2][400] ints. */
struct Hw64PitchArgs {
    const float *acf, *pratio_in, *mark_in;
    const long long *lengths;
    const long long *row_offsets;
    int *pitch;
    float *grp, *pratio;
    int *status;
    int *stages;
    int *rowscr, *segse;
    const int *order;
    int n_utt;
    int mode;    /* frame kernel: SEA_HW25_FRAME_FIND | SEA_HW25_FRAME_TIMECRN */
    int stage;   /* as Hw25PitchArgs */
    float theta; /* regroup kernel */
};
#define SEA_HW64_SCRATCH_WORDS 193 /* per row: lab, key, mraw [64] and buf */
__global__ void hw64_pitch_max_kernel(Hw64PitchArgs a);     /* grid (n_utt, G) x 64: wave (u, g) takes frames g, g + G, ... */
__global__ void hw64_pitch_segment_kernel(Hw64PitchArgs a); /* grid n_utt x 64 */
__global__ void hw64_pitch_frame_kernel(Hw64PitchArgs a);   /* grid (n_utt, G) x 64 */
__global__ void hw64_pitch_regroup_kernel(Hw64PitchArgs a); /* grid n_utt x 64 */
__global__ void hw64_pitch_track_kernel(Hw64PitchArgs a);   /* grid n_utt x 64 */

/* The Hu-Wang estimator's AM labels (hw25_am_kernel.hip): computeAM:1146-1317.  gout, ampatt, am: hout's layout; pitch [rows]
 * ints; amcrn, ratio, seng [rows][25] (ratio, seng or null).  ampatt and am are never null here: the caller's buffers or
 * scratch.  fa / fb: the FFT's two complex buffers, utterance u's [chunk][2 * pitch] block at offsets[u] * chunk * 2 (2^N is at
 * most twice the length); one launch group handles the channels chan0 .. chan0 + chunk - 1.  info [n_utt]: N, or -1 when the
 * utterance skips the stage (all outputs zero: fewer than 3 rows, no voiced frame, too long, a pitch above 100). */
struct Hw25AmArgs {
    const float *gout;
    const int *pitch;
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *amcrn, *ratio, *seng;
    float *ampatt, *am;
    float2 *fa, *fb;
    int *info;
    int *status;
    const int *order;
    const sea_hw25_tables *tables;
    const float2 *tw;
    int n_utt;
    int status_or; /* status[u] |= flags instead of = flags */
    int chan0, chunk;
    int stage;   /* hw25_am_fft_stage_kernel: the stage n (twoPeriod = 2^n) of the launch */
    int inverse; /* the FFT kernels: 0 forward (from ampatt into fa), 1 inverse (from fa, hilbert's doubling and zeroing
                  * applied on the way, into fb) */
};
#define SEA_HW25_AM_LDS_LOG2 12 /* the stages 1..12 run on 4096 points in LDS, the rest over global memory */
#define SEA_HW25_AM_PATT_GRID 8  /* workgroups per (utterance, channel) that walk its blocks of five frames */
#define SEA_HW25_AM_FFT_GRID 8   /* workgroups per (utterance, channel) in the FFT and normalisation kernels */
#define SEA_HW25_AM_RATE_GRID 8  /* workgroups per utterance that walk its (frame, channel) units */
__global__ void hw25_am_prepare_kernel(Hw25AmArgs a);   /* grid n_utt x 64 */
__global__ void hw25_am_patt_kernel(Hw25AmArgs a);      /* grid (n_utt, PATT_GRID, 25) x 256 */
__global__ void hw25_am_fft_head_kernel(Hw25AmArgs a);  /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw25_am_fft_stage_kernel(Hw25AmArgs a); /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw25_am_norm_kernel(Hw25AmArgs a);      /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw25_am_rate_kernel(Hw25AmArgs a);      /* grid (n_utt, RATE_GRID) x 64 */

/* finalSeg:1321-1494 and the binarisation :99-106 (hw25_am_kernel.hip).  grp, amcrn, cross_ev, pratio [rows][25] are only
 * read; mask [rows][25] 0 / 1; grp_final (or null) [rows][25] in {-1, 0, 1}; stages (or null): utterance u's [5][F][25] floats
 * at row_offsets[u] * 125; rowscr: SEA_HW25_FINAL_SCRATCH_WORDS ints per row. */
struct Hw25FinalArgs {
    const float *grp, *amcrn, *cross_ev, *pratio;
    const long long *lengths;
    const long long *row_offsets;
    float *mask, *grp_final, *stages;
    int *status;
    int *rowscr;
    const int *order;
    int n_utt;
    int status_or;
};
#define SEA_HW25_FINAL_SCRATCH_WORDS 150 /* per row: lab, key, lo, hi, m, g [25] */
__global__ void hw25_finalseg_kernel(Hw25FinalArgs a); /* grid n_utt x 64 */

/* The same two stages at 16 kHz on the 64-channel bank (hw64_am_kernel.hip).  Hw25AmArgs and Hw25FinalArgs as they are, at 64
 * channels, a hop of 160 and a pitch of at most 200: gout, ampatt, am in hw64_periphery_kernel's layout; amcrn, ratio, seng,
 * grp, cross_ev, pratio, mask, grp_final [rows][64]; stages [5][F][64] floats at row_offsets[u] * 320; tables: the 25-band
 * tables, of which only am_a and am_beta are read (kaiserPara (0.01, ..) knows neither rate nor bank); tw: the same twiddles. */
__global__ void hw64_am_prepare_kernel(Hw25AmArgs a);   /* grid n_utt x 64 */
__global__ void hw64_am_patt_kernel(Hw25AmArgs a);      /* grid (n_utt, PATT_GRID, 64) x 256 */
__global__ void hw64_am_fft_head_kernel(Hw25AmArgs a);  /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw64_am_fft_stage_kernel(Hw25AmArgs a); /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw64_am_norm_kernel(Hw25AmArgs a);      /* grid (n_utt, FFT_GRID, chunk) x 256 */
__global__ void hw64_am_rate_kernel(Hw25AmArgs a);      /* grid (n_utt, RATE_GRID) x 64 */
#define SEA_HW64_FINAL_SCRATCH_WORDS 384 /* per row: lab, key, lo, hi, m, g [64] */
__global__ void hw64_finalseg_kernel(Hw25FinalArgs a);  /* grid n_utt x 64 */

/* resynthesis:1498-1549 on the same bank (hw25_resynth_kernel.hip).  gout: hout's layout, only read; mask [rows][25], utterance
 * u's lengths[u] / 80 rows from row_offsets[u], a unit set where mask > threshold; out_f32 / out_i16 (either may be null):
 * the packed sample space of the input audio, utterance u's lengths[u] samples at offsets[u]. */
struct Hw25ResynthArgs {
    const float *gout;
    const float *mask;
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *out_f32;
    short *out_i16;
    const int *order;
    const sea_hw25_tables *tables;
    float threshold;
    int n_utt;
};
__global__ void hw25_resynth_kernel(Hw25ResynthArgs a); /* grid n_utt x 64 */

/* The same at 16 kHz on the 64-channel bank (hw64_resynth_kernel.hip).  Hw25ResynthArgs's fields with the 64-band tables: gout
 * in hw64_periphery_kernel's layout, only read; mask [rows][64], utterance u's lengths[u] / 160 rows from row_offsets[u]. */
struct Hw64ResynthArgs {
    const float *gout;
    const float *mask;
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *out_f32;
    short *out_i16;
    const int *order;
    const sea_hw64_tables *tables;
    float threshold;
    int n_utt;
};
__global__ void hw64_resynth_kernel(Hw64ResynthArgs a); /* grid n_utt x 64 */

__global__ void subband_kernel(SubbandArgs a);
__global__ void ns_denoise_pipe_kernel(NsBatchArgs a);
__global__ void ns_denoise_pipe_big_kernel(NsBatchArgs a); /* lower-register form for > 4 utterances per CU */
__global__ void ns_denoise_pipe_fd_kernel(NsBatchArgs a);
__global__ void ns_denoise_pipe_slice_kernel(NsBatchArgs a);     /* time slices: state in / out (NsBatchArgs::state) */
__global__ void ns_denoise_pipe_big_slice_kernel(NsBatchArgs a);
/* + the speech flags of the slice's output frames and the gate's onset as an absolute index: the measures' seven floats ride
 * in the blob's scalars 14..20 and the onset in scalar 21, which the plain slice forms leave alone */
__global__ void ns_denoise_pipe_fd_slice_kernel(NsBatchArgs a);
__global__ void ns_denoise_pipe6_kernel(NsBatchArgs a);    /* six waves per utterance (ns_pipe6_kernel.hip) */
__global__ void ns_denoise_pipe6_dense_kernel(NsBatchArgs a);
__global__ void ns_denoise_pipe6_fd_kernel(NsBatchArgs a); /* + speech flags for the frame-dropping VAD */
__global__ void ns_stream_kernel(NsStreamArgs a);
__global__ void ns16k_pipe_kernel(Ns16StreamArgs a); /* four pipelined waves per stream, two streams per workgroup */
constexpr int kNs16PipeStreamsPerGroup = 2;
__global__ void ns16k_selftest_kernel(const sea_ns16k_tables *t, const float *frames, int nfft, float *outA, float *outB, const float *gains,
                                      int ngain, float *gamma25, float *idct9);
__global__ void ns_stream_fd_kernel(NsStreamArgs a);
__global__ void selftest_pi4_kernel(unsigned long long *mismatches);
__global__ void selftest_dc_kernel(const float *dif, const float *y0, float *out, int *fellback, int ncases);
__global__ void selftest_log_kernel(const float *x, double *out, int n);
__global__ void selftest_log_dd_kernel(const double *x, double *hi, double *lo, int n);
__global__ void selftest_log_sites_kernel(const float *x, float *site1, float *site2, int n);
__global__ void selftest_log_nonfinite_kernel(const float *x, float *site1, float *site2, float *lg, int n);
__global__ void selftest_log_guard_kernel(int site, unsigned long long *stats, float *hits, int cap);
template <bool ALLVAD>
__global__ void selftest_log_lanes_kernel(unsigned long long *stats);
__global__ void selftest_nsdiv_kernel(unsigned long long *out, int iters);
__global__ void selftest_div_kernel(const sea_gt_tables *t, unsigned long long *mismatches);
__global__ void rfft256_kernel(const float *in, float *out, long long nframes, const sea_fft_tables *t);
__global__ void rfft_any_kernel(float *x, const unsigned *sched, long long nframes);
__global__ void compceps_kernel(CepsArgs a);
__global__ void afe_ceps_kernel(AfeArgs a); /* WaveProc + CompCeps, one wave per cepstral frame */
__global__ void afe_vad_kernel(AfeArgs a);  /* PostProc + frame-dropping VAD + flush, one wave per utterance */
__global__ void compceps_frames_kernel(const float *data201, float *coef14, long long nframes,
                                       const sea_cc_tables *t);
__global__ void resynth_fused_kernel(ResynthArgs a); /* both passes of an utterance in one workgroup */
__global__ void gammatone_kernel(const float *in, float *out, int chan, long long L, const sea_gt_tables *t);

} // namespace sea
