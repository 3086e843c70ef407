/*
 * stoi_kernels.h -- the kernels of the short-time objective intelligibility measure (stoi_kernel.hip) and their argument block
 * (stoi_capi.hip); DESIGN.md section 5.24.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sea {

constexpr int kStoiBands = 15, kStoiSegment = 30, kStoiBins = 212, kStoiBin0 = 7;
/* the band kernel: a workgroup takes 64 kept frames of one signal and all bins; the 212 bins are seven tiles of 32 (the last
 * 12 padded with zero columns), each tile 32 cosine and 32 sine columns: 448 basis rows of 256 */
constexpr int kStoiTileRows = 64, kStoiBinTiles = 7, kStoiBasisRows = kStoiBinTiles * 64, kStoiTileK = 16;
constexpr int kStoiItems = 256; /* samples, frames or terms per workgroup of the one-thread-per-item kernels */

/* Utterance u of a chunk: lengths[u] int16 samples of ref and est from offsets[u] of the staged buffers; its L10 resampled
 * floats from x_offsets[u] (a multiple of 4) of either half of x10; F = frame_cum[u + 1] - frame_cum[u] frames; at most
 * seg_cum[u + 1] - seg_cum[u] = max (F - 29, 0) segments.  The *_tiles tables are the prefix tables of the flat item lists:
 * ceil (L10 / 256), ceil (F / 256), ceil (F / 64) and ceil (15 max (F - 29, 0) / 256) items per utterance. */
struct StoiArgs {
    const int16_t *ref, *est;
    const long long *offsets;    /* [n_utt] */
    const long long *lengths;    /* [n_utt] */
    const long long *x_offsets;  /* [n_utt + 1] */
    const long long *frame_cum;  /* [n_utt + 1] */
    const long long *seg_cum;    /* [n_utt + 1] */
    const long long *x_tiles;    /* [n_utt + 1] */
    const long long *e_tiles;    /* [n_utt + 1] */
    const long long *band_tiles; /* [n_utt + 1] */
    const long long *seg_tiles;  /* [n_utt + 1] */
    float *x10;                  /* [2][x_offsets[n_utt]]: ref, then est */
    float *energy;               /* [frame_cum[n_utt]]: e[f] of the reference */
    uint32_t *emax;              /* [n_utt]: the bits of max e; zero at the launch of stoi_energy_kernel */
    int *keep;                   /* [frame_cum[n_utt]]: the kept frames of utterance u from frame_cum[u], ascending */
    int *kept;                   /* [n_utt]: M */
    float *bands;                /* [2][frame_cum[n_utt]][15]: X, then Y; rows frame_cum[u] .. + M - 1 are written */
    const float *basis;          /* [448][256]: stoi_basis_kernel */
    float *d;                    /* [seg_cum[n_utt]][15]: the terms of utterance u from 15 seg_cum[u] */
    double *stoi_sum;            /* [n_utt] */
    int n_utt;
    int rate;
};

__global__ void stoi_basis_kernel(float *basis);      /* grid 448, 256 threads */
__global__ void stoi_resample_kernel(StoiArgs a);     /* grid (x_tiles[n_utt], 2), 256 threads */
__global__ void stoi_energy_kernel(StoiArgs a);       /* grid e_tiles[n_utt], 256 threads */
__global__ void stoi_compact_kernel(StoiArgs a);      /* grid n_utt, 256 threads */
__global__ void stoi_band_kernel(StoiArgs a);         /* grid (band_tiles[n_utt], 2), 256 threads */
__global__ void stoi_segment_kernel(StoiArgs a);      /* grid seg_tiles[n_utt], 256 threads */
__global__ void stoi_finish_kernel(StoiArgs a);       /* grid n_utt, one wave */

} // namespace sea
