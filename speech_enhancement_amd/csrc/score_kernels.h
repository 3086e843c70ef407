/*
 * score_kernels.h -- the kernels of the objective scores (score_kernel.hip) and their argument blocks (score_capi.hip);
 * DESIGN.md section 5.23.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sea {

/* A wave owns 63 half-frames (lane 63 only fetches the first half-frame of the next wave's tile for frame 62), a workgroup of
 * four waves 252; a mask tile is 64 rows of 64 units. */
constexpr int kScoreWaveHalves = 63, kScoreWaves = 4, kScoreTileHalves = kScoreWaveHalves * kScoreWaves;
constexpr int kMaskTileRows = 64;

/* What both score kernels read.  Utterance u of a chunk: lengths[u] samples of ref and est from sample offsets[u] (a multiple
 * of 8: 16-byte loads) of the two staged buffers; H = lengths[u] / hop whole half-frames, F = max (H - 1, 0) frames;
 * frame_offsets[u + 1] - frame_offsets[u] = F; tile_cum[u + 1] - tile_cum[u] = ceil (H / 252) workgroup items. */
struct ScoreArgs {
    const int16_t *ref, *est;
    const long long *offsets;       /* [n_utt] */
    const long long *lengths;       /* [n_utt] */
    const long long *frame_offsets; /* [n_utt + 1] */
    const long long *tile_cum;      /* [n_utt + 1] */
    float *frame_db;                /* [frame_offsets[n_utt]]: the clamped d of a frame, 0x7fc00000 where the reference is silent */
    long long *partials;            /* [4 tile_cum[n_utt]][3]: Srr, See, Sre over the half-frames a wave owns */
    long long *sums;                /* [n_utt][3] */
    double *seg_sum;                /* [n_utt] */
    int *seg_frames;                /* [n_utt] */
    int n_utt;
    int hop;
};
template <int HOP>
__global__ void score_frames_kernel(ScoreArgs a); /* grid tile_cum[n_utt], 256 threads */
__global__ void score_finish_kernel(ScoreArgs a); /* grid n_utt, one wave */

/* Utterance u: rows row_offsets[u] .. row_offsets[u + 1] - 1 of est and ideal [rows][64]; tile_cum[u + 1] - tile_cum[u] =
 * ceil (rows / 64) workgroup items.  counts [n_utt][4] (n11, n10, n01, n00; est on / ideal on) must be zero at the launch. */
struct MaskScoreArgs {
    const float *est, *ideal;
    const long long *row_offsets; /* [n_utt + 1] */
    const long long *tile_cum;    /* [n_utt + 1] */
    unsigned long long *counts;
    float t_est, t_ideal;
    int n_utt;
};
__global__ void mask_score_kernel(MaskScoreArgs a); /* grid tile_cum[n_utt], 256 threads */

} // namespace sea
