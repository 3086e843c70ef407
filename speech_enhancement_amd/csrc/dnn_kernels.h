/*
 * dnn_kernels.h -- the kernels of the DNN mask estimator (dnn_kernel.hip) and their internal launches (dnn_capi.hip);
 * DESIGN.md section 5.21.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sea {

/* Cochleagram of the 64 int16 subband streams subband_kernel writes ([64][pitch] per utterance at offsets[u] * 64, pitch =
 * lengths[u] rounded up to 8): feats[row_offsets[u] + f][c] = sea_lnf ((float)(1 + sum of the 320 squares of frame f)),
 * f < (lengths[u] - 320) / 160 + 1.  An utterance shorter than 320 samples has no row. */
struct CochleagramArgs {
    const int16_t *sub;
    const long long *offsets;
    const long long *lengths;
    const long long *row_offsets;
    float *feats; /* [rows][64] */
    int n_utt;
};
__global__ void cochleagram64_kernel(CochleagramArgs a); /* a workgroup per (utterance, channel): grid n_utt * 64 */

/* The network's input: x0[row][(d + C) * 64 + c] = (feats[clamp (f + d) of row's utterance][c] + shift[k]) * scale[k] */
struct DnnSpliceArgs {
    const float *feats;           /* [rows][64] */
    const long long *row_offsets; /* [n_utt + 1]: utterance u's rows are row_offsets[u] .. row_offsets[u + 1] - 1 */
    const float *shift, *scale;   /* [64 (2 C + 1)] */
    float *x0;                    /* [rows][ldx] */
    int ldx;
    int context;
    int n_utt;
};
__global__ void dnn_splice_kernel(DnnSpliceArgs a); /* a workgroup per row */

/* One layer: y[m][n] = act (b[n] + sum over k ascending of x[m][k] w[n][k]), every product one fmaf into the sum */
constexpr int kDnnTileM = 128, kDnnTileN = 128, kDnnTileK = 32;
struct DnnLayerArgs {
    const float *x; /* [M][ldx], ldx a multiple of 4; columns K .. ldx - 1 hold anything */
    const float *w; /* [N rounded up to kDnnTileN][Kp] with zeros beyond N and K; Kp = K rounded up to kDnnTileK */
    const float *b; /* [N] */
    float *y;       /* [M][ldy] */
    long long M;
    int N, K, Kp, ldx, ldy, act;
};
__global__ void dnn_layer_kernel(DnnLayerArgs a); /* grid (M tiles, N tiles), 256 threads */

} // namespace sea

struct sea_dnn {
    int device = 0;
    int context = 0, n_layers = 0;
    int dims[9] = {};
    int act[8] = {};
    int ld = 0; /* row pitch of the activation buffers: the largest dimension rounded up to 4 */
    float *d_shift = nullptr, *d_scale = nullptr;
    float *d_w[8] = {}, *d_b[8] = {};
};

namespace sea_capi {

int cochleagram64_launch(const short *d_sub64, const long long *d_offsets, const long long *d_lengths,
                         const long long *d_row_offsets, float *d_feats, int n_utt, hipStream_t stream);
/* d_row_offsets [n_utt + 1]; d_act0 and d_act1 [rows][m->ld] floats each; d_out [rows][dims[n_layers]]; marks (or null):
 * 1 + n_layers events, recorded after the splice and after every layer */
int dnn_forward_launch(const sea_dnn *m, const float *d_feats, const long long *d_row_offsets, int n_utt, long long rows,
                       float *d_act0, float *d_act1, float *d_out, hipStream_t stream, const hipEvent_t *marks = nullptr);

} // namespace sea_capi
