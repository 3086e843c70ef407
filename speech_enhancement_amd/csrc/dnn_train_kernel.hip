/*
 * dnn_train_kernel.hip -- one SGD step of the DNN mask estimator, gfx950, after the unchanged forward
 * dnn_layer_kernel:
 *
 *   dnn_gather_splice_kernel   the minibatch's input rows through an index list (dnn_splice_kernel's arithmetic)
 *   dnn_delta_out_kernel       e = y - t, the row's chain of e^2, the output delta; dnn_loss_kernel sums the rows in double
 *   dnn_dgrad_kernel           E = delta W on v_mfma_f32_32x32x2_f32 (reduction over j), times d (a) in the epilogue
 *   dnn_wgrad_kernel           G = delta^T a on the same instruction (reduction over the minibatch row m); the bias gradient g
 *                              rides it as a column of ones at k = K
 *   dnn_sgd_kernel             momentum and step over the real weights and biases
 *
 * Pinned on the bits by tests/dnn_train_model_driver.c: every reduction is one fmaf chain from +0 in ascending order of its
 * index, so all reduction tiles of an output enter one accumulator in order, the first C operand is zero, and there is no
 * split reduction and no atomic.  Every other operation is an individually rounded float operation.
 */
#include "dnn_math.h"
#include "dnn_train_kernels.h"

namespace sea {

__global__ __launch_bounds__(256) void dnn_gather_splice_kernel(DnnGatherArgs a)
{
    const long long row = a.idx[blockIdx.x];
    int lo = 0, hi = a.n_utt; /* the utterance u with row_offsets[u] <= row < row_offsets[u + 1] */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.row_offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    const long long r0 = a.row_offsets[lo], F = a.row_offsets[lo + 1] - r0, f = row - r0;
    const int K0 = 64 * (2 * a.context + 1);
    float *x = a.x0 + (long long)blockIdx.x * a.ldx;
    for (int k = threadIdx.x; k < K0; k += 256) {
        long long g = f + (k >> 6) - a.context;
        g = g < 0 ? 0 : (g > F - 1 ? F - 1 : g);
        x[k] = __fmul_rn(__fadd_rn(a.feats[(r0 + g) * 64 + (k & 63)], a.shift[k]), a.scale[k]);
    }
}

/* delta = e d (a) by the activation that produced a: the sigmoid's a (1 - a) is a subtract then a multiply, then one more
 * multiply; the rectifier passes e where a > 0; the identity passes e */
__device__ static inline float dnn_delta_of(float e, float a, int act)
{
    if (act == 1) return __fmul_rn(e, __fmul_rn(a, __fsub_rn(1.0f, a)));
    if (act == 2) return a > 0.0f ? e : 0.0f;
    return e;
}

/* A wave per row.  Lane l holds e[j0 + l]; the chain over j is serial, so every lane runs it on the values fetched from the
 * lanes in turn (all lanes hold the same acc). */
__global__ __launch_bounds__(256) void dnn_delta_out_kernel(DnnDeltaOutArgs a)
{
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.B) return; /* uniform over the wave */
    const float *y = a.y + (long long)m * a.ldy;
    const float *t = a.targets + a.idx[m] * a.N;
    float acc = 0.0f;
    for (int j0 = 0; j0 < a.N; j0 += 64) {
        const int j = j0 + lane;
        float e = 0.0f;
        if (j < a.N) {
            const float yy = y[j];
            e = __fsub_rn(yy, t[j]);
            if (a.delta) a.delta[(long long)m * a.ldd + j] = dnn_delta_of(e, yy, a.act);
        }
        const int n = a.N - j0 < 64 ? a.N - j0 : 64;
        for (int q = 0; q < n; ++q) {
            const float eq = __shfl(e, q);
            acc = __fmaf_rn(eq, eq, acc);
        }
    }
    if (lane == 0) a.r[m] = acc;
}

__global__ __launch_bounds__(64) void dnn_loss_kernel(const float *r, int B, double *loss)
{
    const int lane = threadIdx.x;
    double p = 0.0;
    for (int i = lane; i < B; i += 64) p += (double)r[i];
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += __shfl(p, l);
    if (lane == 0) *loss = 0.5 * s;
}

/* ---- the two GEMMs -------------------------------------------------------------------------------------------------------------
 * A 64 x 64 output tile per workgroup, four waves as 2 x 2, each wave one 32 x 32 accumulator (16 registers), the reduction
 * in steps of 32 (dgrad) or 64 (wgrad, whose reduction is the long one: B rows) through LDS, the next step's operands fetched
 * into registers while this one is multiplied.  With the lane map of dnn_kernel.hip (A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]):
 *
 *   a tile staged as it lies with the reduction index as its ROW (W [j][k] in dgrad, delta [m][j] and a [m][k] in wgrad) is read
 *   T[2 kk + (l >> 5)][col + (l & 31)].  ds_read_b32 serves lanes 0..31 and 32..63 in separate cycles, on 32 banks: the two
 *   reduction rows of one instruction can never collide, and a row's 32 consecutive floats take 32 banks.  The pitch is the
 *   tile's 64 floats, which keeps the float4 stores aligned and conflict-free.
 *   dgrad's delta tile has the reduction index as its COLUMN, as the forward's x: lanes 0..31 read 32 rows of one column, so
 *   the pitch is 33 floats (odd: 32 rows, 32 banks) and the stores are single floats.
 */
namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kT = kDnnTrainTile, kR = kDnnTrainTileR, kRw = kDnnTrainTileRw, kLdCol = kR + 1;

/* Four floats of row `row` from column c on, zeros from column `real` on and for a row or column outside the buffer (ld and c
 * are multiples of 4, so c < ld means c + 3 < ld), in two parts.  raw4 only loads -- an invalid piece reads the buffer's first
 * four floats -- so that a step's loads are all in flight while the previous step is multiplied; mask4 puts the zeros in when
 * the piece goes to LDS, one step later.  Neither branches. */
__device__ inline bool piece_ok(long long row, long long rows, int c, int real, int ld) { return row < rows && c < ld && c < real; }
__device__ inline float4 raw4(const float *base, long long row, long long rows, int c, int real, int ld)
{
    return *reinterpret_cast<const float4 *>(base + (piece_ok(row, rows, c, real, ld) ? row * ld + c : 0));
}
__device__ inline float4 mask4(float4 v, long long row, long long rows, int c, int real, int ld)
{
    const bool ok = piece_ok(row, rows, c, real, ld);
    return make_float4(ok ? v.x : 0.0f, ok && c + 1 < real ? v.y : 0.0f, ok && c + 2 < real ? v.z : 0.0f, ok && c + 3 < real ? v.w : 0.0f);
}
} // namespace

__global__ __launch_bounds__(256) void dnn_dgrad_kernel(DnnDgradArgs a)
{
    __shared__ float Ds[kT][kLdCol];                                /* delta [m][j] */
    __shared__ __attribute__((aligned(16))) float Ws[kR][kT];       /* W [j][k] as it lies */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
    const int m0 = blockIdx.x * kT, k0 = blockIdx.y * kT;
    const int Nr = (a.N + kR - 1) / kR * kR; /* rows N .. Nr - 1 of w exist and are zeros */

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

    float4 rd[2], rw[2]; /* piece p of delta: row p >> 3, columns 4 (p & 7) .. + 3; of W: row p >> 4, columns 4 (p & 15) .. + 3 */
    auto fetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i, k = k0 + 4 * (p & 15);
            rd[i] = raw4(a.delta, m0 + (p >> 3), a.M, j0 + 4 * (p & 7), a.N, a.ldd);
            rw[i] = *reinterpret_cast<const float4 *>(a.w + (k < a.Kp ? (long long)(j0 + (p >> 4)) * a.Kp + k : 0));
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < Nr; j0 += kR) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = tid + 256 * i;
            const float4 v = mask4(rd[i], m0 + (p >> 3), a.M, j0 + 4 * (p & 7), a.N, a.ldd);
            float *d = &Ds[p >> 3][4 * (p & 7)];
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            *reinterpret_cast<float4 *>(&Ws[p >> 4][4 * (p & 15)]) = k0 + 4 * (p & 15) < a.Kp ? rw[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        __syncthreads();
        if (j0 + kR < Nr) fetch(j0 + kR);
        float av[kR / 2], bv[kR / 2]; /* the step's operands first, so that the chain of MFMAs waits for LDS once */
#pragma unroll
        for (int kk = 0; kk < kR / 2; ++kk) av[kk] = Ds[wm * 32 + li][2 * kk + lk], bv[kk] = Ws[2 * kk + lk][wn * 32 + li];
        __builtin_amdgcn_sched_barrier(0); /* or the scheduler sinks every read back in front of its MFMA */
#pragma unroll
        for (int kk = 0; kk < kR / 2; ++kk) /* ascending j: 2 kk (lanes 0..31) then 2 kk + 1 (lanes 32..63) */
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
        __syncthreads();
    }

    const int k = k0 + wn * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (m < a.M && k < a.K) a.out[(long long)m * a.ldo + k] = dnn_delta_of(acc[r], a.a_prev[(long long)m * a.lda + k], a.act);
    }
}

__global__ __launch_bounds__(256) void dnn_wgrad_kernel(DnnWgradArgs a)
{
    __shared__ __attribute__((aligned(16))) float Ds[kRw][kT]; /* delta [m][j] as it lies */
    __shared__ __attribute__((aligned(16))) float As[kRw][kT]; /* a [m][k] as it lies */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
    const int j0 = blockIdx.x * kT, k0 = blockIdx.y * kT;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

    /* rows m >= M are zeros in BOTH operands: 0 * (whatever the buffer holds there) may be NaN */
    float4 rd[kRw / 16], ra[kRw / 16]; /* piece p of either tile: row p >> 4, columns 4 (p & 15) .. + 3 */
    auto fetch = [&](int m0) {
#pragma unroll
        for (int i = 0; i < kRw / 16; ++i) {
            const int p = tid + 256 * i, c4 = 4 * (p & 15);
            rd[i] = raw4(a.delta, m0 + (p >> 4), a.M, j0 + c4, a.N, a.ldd);
            ra[i] = raw4(a.a_prev, m0 + (p >> 4), a.M, k0 + c4, a.K, a.lda);
        }
    };
    fetch(0);
    for (int m0 = 0; m0 < a.M; m0 += kRw) {
#pragma unroll
        for (int i = 0; i < kRw / 16; ++i) {
            const int p = tid + 256 * i, c4 = 4 * (p & 15);
            float4 v = mask4(ra[i], m0 + (p >> 4), a.M, k0 + c4, a.K, a.lda);
            /* the column of ones at k = K: fmaf (delta, 1, acc) is acc + delta, the bias gradient's chain */
            const int d = m0 + (p >> 4) < a.M ? a.K - (k0 + c4) : -1;
            v.x = d == 0 ? 1.0f : v.x, v.y = d == 1 ? 1.0f : v.y, v.z = d == 2 ? 1.0f : v.z, v.w = d == 3 ? 1.0f : v.w;
            *reinterpret_cast<float4 *>(&Ds[p >> 4][c4]) = mask4(rd[i], m0 + (p >> 4), a.M, j0 + c4, a.N, a.ldd);
            *reinterpret_cast<float4 *>(&As[p >> 4][c4]) = v;
        }
        __syncthreads();
        if (m0 + kRw < a.M) fetch(m0 + kRw);
#pragma unroll
        for (int h = 0; h < kRw / 2; h += 16) { /* sixteen MFMAs' operands first, so that the chain waits for LDS once per half */
            float av[16], bv[16];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) av[kk] = Ds[2 * (h + kk) + lk][wm * 32 + li], bv[kk] = As[2 * (h + kk) + lk][wn * 32 + li];
            __builtin_amdgcn_sched_barrier(0); /* or the scheduler sinks every read back in front of its MFMA */
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) /* ascending m */
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
        }
        __syncthreads();
    }

    const int k = k0 + wn * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = j0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (j < a.N && k < a.K) a.G[(long long)j * a.K + k] = acc[r];
        if (j < a.N && k == a.K) a.g[j] = acc[r];
    }
}

__global__ __launch_bounds__(256) void dnn_sgd_kernel(DnnSgdArgs a)
{
    const long long nw = (long long)a.N * a.K, total = nw + a.N;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float *w, *v;
        float g;
        if (i < nw) {
            const long long j = i / a.K, k = i - j * a.K;
            w = a.w + j * a.Kp + k, v = a.vw + i, g = a.G[i];
        } else {
            w = a.b + (i - nw), v = a.vb + (i - nw), g = a.g[i - nw];
        }
        const float vn = __fadd_rn(__fmul_rn(a.mu, *v), g);
        *v = vn;
        *w = __fsub_rn(*w, __fmul_rn(a.eta, vn));
    }
}

} // namespace sea
