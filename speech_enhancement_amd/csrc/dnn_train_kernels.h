/*
 * dnn_train_kernels.h -- the kernels of one SGD step of the DNN mask estimator (dnn_train_kernel.hip) and the trainer object
 * (dnn_train_capi.hip); DESIGN.md section 5.22.  The forward pass is dnn_layer_kernel of dnn_kernels.h, unchanged.
 */
#pragma once
#include "dnn_kernels.h"

namespace sea {

/* Item 1: minibatch row m is global row idx[m] of the training set:
 * x0[m][k] = (feats[clamp within idx[m]'s utterance][k & 63] + shift[k]) * scale[k], as dnn_splice_kernel computes that row */
struct DnnGatherArgs {
    const float *feats;           /* [rows][64] */
    const long long *row_offsets; /* [n_utt + 1] */
    const long long *idx;         /* [B]: every value within 0 .. rows - 1 (checked on the host) */
    const float *shift, *scale;   /* [64 (2 C + 1)] */
    float *x0;                    /* [B][ldx] */
    int ldx, context, n_utt;
};
__global__ void dnn_gather_splice_kernel(DnnGatherArgs a); /* a workgroup per minibatch row: grid B */

/* Items 3 and 4: e = y - t[idx[m]], r[m] = the fmaf chain of e^2 over j ascending from +0, delta = e d(y) */
struct DnnDeltaOutArgs {
    const float *y;       /* [B][ldy] */
    const float *targets; /* [rows][N] */
    const long long *idx; /* [B] */
    float *delta;         /* [B][ldd], or null: the loss alone */
    float *r;             /* [B] */
    int B, N, ldy, ldd, act;
};
__global__ void dnn_delta_out_kernel(DnnDeltaOutArgs a); /* a wave per minibatch row: grid ceil (B / 4), 256 threads */

/* Item 3's sum: p[l] = sum over i ascending of (double) r[64 i + l], *loss = 0.5 * sum over l ascending of p[l] */
__global__ void dnn_loss_kernel(const float *r, int B, double *loss); /* one wave */

/* both GEMMs: a 64 x 64 output tile; the reduction in steps of 32 (dgrad, over j) and 64 (wgrad, over m) */
constexpr int kDnnTrainTile = 64, kDnnTrainTileR = 32, kDnnTrainTileRw = 64;

/* Item 7: E[m][k] = sum over j ascending of delta[m][j] w[j][k] from +0, out[m][k] = E d(a_prev[m][k]) */
struct DnnDgradArgs {
    const float *delta;  /* [M][ldd], ldd a multiple of 4; columns N .. ldd - 1 hold anything */
    const float *w;      /* [N rounded up to kDnnTileN][Kp], zeros beyond N and K */
    const float *a_prev; /* [M][lda] */
    float *out;          /* [M][ldo] */
    int M, N, K, Kp, ldd, lda, ldo, act; /* act: the activation that produced a_prev */
};
__global__ void dnn_dgrad_kernel(DnnDgradArgs a); /* grid (M tiles, K tiles), 256 threads */

/* Items 5 and 6: G[j][k] = sum over m ascending of delta[m][j] a_prev[m][k] from +0; the kernel takes a_prev[m][K] as 1, so
 * that column K of the product is g[j] = the sum over m ascending of delta[m][j]: fmaf (delta, 1, acc) is the float add */
struct DnnWgradArgs {
    const float *delta;  /* [M][ldd] */
    const float *a_prev; /* [M][lda]; both pitches multiples of 4, columns beyond N and K hold anything */
    float *G;            /* [N][K] */
    float *g;            /* [N] */
    int M, N, K, ldd, lda;
};
__global__ void dnn_wgrad_kernel(DnnWgradArgs a); /* grid (N tiles, tiles of K + 1 columns), 256 threads */

/* Item 8 over the real entries of one layer: v = mu v + g (a multiply, an add), w = w - eta v (a multiply, a subtract) */
struct DnnSgdArgs {
    float *w;       /* [..][Kp]: entry (j, k) at j Kp + k; the padding is never written */
    float *b;       /* [N] */
    const float *G; /* [N][K] */
    const float *g; /* [N] */
    float *vw;      /* [N][K] */
    float *vb;      /* [N] */
    int N, K, Kp;
    float eta, mu;
};
__global__ void dnn_sgd_kernel(DnnSgdArgs a); /* grid-stride over N K + N entries */

} // namespace sea
