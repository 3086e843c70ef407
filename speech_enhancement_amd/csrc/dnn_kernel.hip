/*
 * dnn_kernel.hip -- the DNN mask estimator between subband_kernel and resynth_fused_kernel, gfx950:
 *
 *   cochleagram64_kernel   the Wang-lab cochleagram of the 64 int16 subband streams: the energy of 20 ms frames every 10 ms as
 *                          an exact integer, one conversion to float, sea_lnf
 *   dnn_splice_kernel      the network's input row: +-C frames of context clamped to the utterance, + shift, * scale
 *   dnn_layer_kernel       y = act (x W^T + b) on v_mfma_f32_32x32x2_f32
 *
 * Everything is pinned on the bits by the plain-C model tests/dnn_model_driver.c, which includes the same dnn_math.h: the
 * f32-input MFMA is a k-ordered fmaf chain with one rounding per product, so a layer is the model's loop
 * `acc = fmaf (x[k], W[j][k], acc)` from acc = b[j] so long as the K tiles enter one accumulator in ascending k (no split-K)
 * and the bias is the first MFMA's C operand.
 */
#include "dnn_kernels.h"
#include "dnn_math.h"

namespace sea {

/* ---- cochleagram ---------------------------------------------------------------------------------------------------------
 * A wave takes tiles of 63 frames: lane l sums the squares of half-frame 63 t + l (160 samples = twenty 16-byte loads, the
 * half-frame starts 320 B apart are 16-byte aligned because pitch is a multiple of 8 samples), frame f is half-frame f plus
 * half-frame f + 1, fetched from the next lane.  Half-frames 0 .. F cover samples below 160 (F + 1) <= L only: the padding
 * of a channel row is never part of a sum. */
__global__ __launch_bounds__(256) void cochleagram64_kernel(CochleagramArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x >> 6, c = blockIdx.x & 63;
    const long long L = a.lengths[u];
    if (L < 320) return;
    const long long F = (L - 320) / 160 + 1, pitch = (L + 7) & ~7LL;
    const int16_t *row = a.sub + a.offsets[u] * 64 + c * pitch;
    float *out = a.feats + a.row_offsets[u] * 64 + c;
    const long long ntile = (F + 62) / 63;
    for (long long tile = wave; tile < ntile; tile += 4) {
        const long long h = tile * 63 + lane; /* this lane's half-frame */
        unsigned long long sum = 0;
        if (h <= F) {
            const int16_t *src = row + h * 160;
            const long long avail = pitch - h * 160; /* samples of this channel row from the half-frame's start on */
#pragma unroll 5
            for (int j = 0; j < 20; ++j) {
                const uint4 v = (8LL * j + 8 <= avail) ? *reinterpret_cast<const uint4 *>(src + 8 * j) : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int s0 = (short)(d[q] & 0xffffu), s1 = (short)(d[q] >> 16);
                    sum += (uint32_t)(s0 * s0) + (uint32_t)(s1 * s1); /* two squares: at most 2^31 */
                }
            }
        }
        const uint32_t lo = __shfl_down((uint32_t)sum, 1), hi = __shfl_down((uint32_t)(sum >> 32), 1);
        const unsigned long long next = ((unsigned long long)hi << 32) | lo;
        if (lane < 63 && h < F) out[h * 64] = sea_lnf((float)(long long)(sum + next + 1ULL));
    }
}

/* ---- splice + shift + scale ---------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void dnn_splice_kernel(DnnSpliceArgs a)
{
    const long long row = blockIdx.x;
    int lo = 0, hi = a.n_utt; /* the utterance u with row_offsets[u] <= row < row_offsets[u + 1] */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.row_offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    const long long r0 = a.row_offsets[lo], F = a.row_offsets[lo + 1] - r0, f = row - r0;
    const int K0 = 64 * (2 * a.context + 1);
    float *x = a.x0 + row * a.ldx;
    for (int k = threadIdx.x; k < K0; k += 256) {
        long long g = f + (k >> 6) - a.context;
        g = g < 0 ? 0 : (g > F - 1 ? F - 1 : g);
        x[k] = __fmul_rn(__fadd_rn(a.feats[(r0 + g) * 64 + (k & 63)], a.shift[k]), a.scale[k]);
    }
}

/* ---- one layer ---------------------------------------------------------------------------------------------------------------
 * A 128 x 128 output tile per workgroup, four waves as 2 x 2, each wave 2 x 2 tiles of 32 x 32 (four accumulators of 16
 * registers), K in steps of 32 through LDS.  v_mfma_f32_32x32x2_f32 takes one float per lane for A and for B: lane l holds
 * A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], and returns D[i = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][j = l & 31]
 * in register r.  Here A is x (i the row m) and B[k][j] = w[n = j][k], both staged as [row][k] with a pitch of 36 floats
 * (16-byte rows for the float4 stores).  The next K tile is fetched into registers while this one is multiplied. */
namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kLd = kDnnTileK + 4;
} // namespace

__global__ __launch_bounds__(256) void dnn_layer_kernel(DnnLayerArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[kDnnTileM][kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kDnnTileN][kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * kDnnTileM;
    const int n0 = blockIdx.y * kDnnTileN;
    const int li = lane & 31, lk = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) { /* the bias is the chain's first C operand: column j = lane & 31 in every register */
        const int n = n0 + wn * 64 + tn * 32 + li;
        const float bias = n < a.N ? a.b[n] : 0.0f;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = bias;
    }

    /* this thread's four float4 of each operand tile: piece p -> row p >> 3, columns 4 (p & 7) .. + 3 */
    float4 ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * i, r = p >> 3, k = k0 + 4 * (p & 7);
            const long long m = m0 + r;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < a.M && k < a.K) { /* k + 3 < ldx: ldx is a multiple of 4 and at least K */
                v = *reinterpret_cast<const float4 *>(a.x + m * a.ldx + k);
                if (k + 1 >= a.K) v.y = 0.0f; /* K padding is zeros, whatever the buffer holds there */
                if (k + 2 >= a.K) v.z = 0.0f;
                if (k + 3 >= a.K) v.w = 0.0f;
            }
            ra[i] = v;
            rb[i] = *reinterpret_cast<const float4 *>(a.w + (long long)(n0 + r) * a.Kp + k); /* padded with zeros at creation */
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < a.Kp; k0 += kDnnTileK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * i, r = p >> 3, c4 = 4 * (p & 7);
            *reinterpret_cast<float4 *>(&As[r][c4]) = ra[i];
            *reinterpret_cast<float4 *>(&Bs[r][c4]) = rb[i];
        }
        __syncthreads();
        if (k0 + kDnnTileK < a.Kp) fetch(k0 + kDnnTileK);
#pragma unroll
        for (int kk = 0; kk < kDnnTileK / 2; ++kk) { /* ascending k: 2 kk (lanes 0..31) then 2 kk + 1 (lanes 32..63) */
            const float a0 = As[wm * 64 + li][2 * kk + lk], a1 = As[wm * 64 + 32 + li][2 * kk + lk];
            const float b0 = Bs[wn * 64 + li][2 * kk + lk], b1 = Bs[wn * 64 + 32 + li][2 * kk + lk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + wn * 64 + tn * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < a.M && n < a.N) a.y[m * a.ldy + n] = sea_dnn_act(acc[tm][tn][r], a.act);
            }
        }
}

} // namespace sea
