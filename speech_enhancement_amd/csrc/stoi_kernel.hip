/*
 * stoi_kernel.hip -- the short-time objective intelligibility measure of clean against enhanced int16 audio, gfx950 (DESIGN.md
 * section 5.24):
 *
 *   stoi_resample_kernel   16 k or 8 k -> 10 k: one output sample per thread, an in-order fmaf chain over at most 33 taps
 *   stoi_energy_kernel     the windowed energy of every 256-sample frame of the reference, and the utterance's largest
 *   stoi_compact_kernel    a workgroup per utterance: the frames within 40 dB of the largest, in order, and their count M
 *   stoi_band_kernel       the 15 third-octave magnitudes of every kept frame of both signals: the overlap-added, windowed
 *                          frames [rows][256] times the transform's basis [256][424] on v_mfma_f32_32x32x2_f32
 *   stoi_segment_kernel    one thread per (30-frame segment, band): normalise, clip, correlate
 *   stoi_finish_kernel     a wave per utterance: the sum of the terms as one in-order double chain per lane
 *
 * Every value is pinned on the bits by the plain-C model tests/stoi_model_driver.c, which includes the same stoi_tables.inc.
 * The only unordered reduction is a maximum of non-negative floats (an integer atomicMax on their bits); there is no
 * floating-point atomic.  The number of kept frames lives on the device: the later kernels are launched for every frame and
 * the rows past M leave at once.
 */
#include "dnn_math.h"
#include "stoi_kernels.h"
#include "stoi_tables.inc"

namespace sea {

namespace {

__device__ const float kW[256] = {SEA_STOI_W_VALUES};
__device__ const float kCs[512] = {SEA_STOI_CS_VALUES};
__device__ const float kH16[161] = {SEA_STOI_H16_VALUES};
__device__ const float kH8[101] = {SEA_STOI_H8_VALUES};
__device__ const int kLo[16] = {SEA_STOI_BAND_LO};

/* the utterance that owns item `item` of a prefix table with cum[0] = 0 <= item < cum[n]: the largest u with cum[u] <= item */
__device__ int owner_of(const long long *cum, int n, long long item)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= item) lo = mid;
        else hi = mid;
    }
    return lo;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kLd = kStoiTileK + 4;     /* pitch of the staged operand tiles: 16-byte rows */
constexpr int kPd = 32 * kStoiBinTiles + 1; /* pitch of the power tile */

} // namespace

/* ---- the basis: row 64 t + 32 s + b is the cosine (s = 0) or sine (s = 1) column of bin 7 + 32 t + b, zeros past bin 218 --- */
__global__ __launch_bounds__(256) void stoi_basis_kernel(float *basis)
{
    const int row = blockIdx.x, n = threadIdx.x;
    const int k = kStoiBin0 + 32 * (row >> 6) + (row & 31), s = (row >> 5) & 1;
    basis[row * 256 + n] = k < kStoiBin0 + kStoiBins ? kCs[(n * k + 128 * s) & 511] : 0.0f;
}

/* ---- step a ---------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void stoi_resample_kernel(StoiArgs a)
{
    const long long item = blockIdx.x;
    const int u = owner_of(a.x_tiles, a.n_utt, item);
    const int p = 5, q = a.rate == 16000 ? 8 : 4, half = a.rate == 16000 ? 80 : 50;
    const float *h = a.rate == 16000 ? kH16 : kH8;
    const long long L = a.lengths[u], L10 = (5 * L + q - 1) / q;
    const long long i = (item - a.x_tiles[u]) * kStoiItems + threadIdx.x;
    if (i >= L10) return;
    const int16_t *x = (blockIdx.y ? a.est : a.ref) + a.offsets[u];
    const long long c = i * q;
    long long k = c > half ? (c - half + p - 1) / p : 0; /* the first k with c - k p <= half */
    long long k1 = (c + half) / p;                       /* the last k with c - k p >= -half */
    if (k1 > L - 1) k1 = L - 1;
    float acc = 0.0f;
    for (; k <= k1; ++k) acc = sea_fmaf(h[half + (int)(c - k * p)], (float)x[k], acc);
    a.x10[(blockIdx.y ? a.x_offsets[a.n_utt] : 0) + a.x_offsets[u] + i] = acc;
}

/* ---- step b: the energies ---------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void stoi_energy_kernel(StoiArgs a)
{
    const long long item = blockIdx.x;
    const int u = owner_of(a.e_tiles, a.n_utt, item);
    const long long F = a.frame_cum[u + 1] - a.frame_cum[u];
    const long long f = (item - a.e_tiles[u]) * kStoiItems + threadIdx.x;
    if (f >= F) return;
    const float *x = a.x10 + a.x_offsets[u] + 128 * f;
    float e = 0.0f;
    for (int n = 0; n < 256; ++n) {
        const float v = __fmul_rn(kW[n], x[n]);
        e = __fadd_rn(e, __fmul_rn(v, v));
    }
    a.energy[a.frame_cum[u] + f] = e;
    atomicMax(a.emax + u, sea_dnn_bits(e)); /* e >= +0: the order of the bits is the order of the values */
}

/* ---- step b: the kept frames ------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void stoi_compact_kernel(StoiArgs a)
{
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
    const long long f0 = a.frame_cum[u], F = a.frame_cum[u + 1] - f0;
    const float emax = sea_dnn_float(a.emax[u]);
    int base = 0;
    for (long long g = 0; g < F; g += 256) {
        const long long f = g + tid;
        const bool on = f < F && __fmul_rn(a.energy[f0 + f], 10000.0f) > emax;
        const unsigned long long b = __ballot(on);
        if (lane == 0) wave_count[wave] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ULL << lane) - 1ULL)), all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_count[w];
            all += wave_count[w];
        }
        if (on) a.keep[f0 + base + before] = (int)f;
        base += all;
        __syncthreads();
    }
    if (tid == 0) a.kept[u] = base;
}

/* ---- steps c and d -----------------------------------------------------------------------------------------------------------
 * A workgroup takes rows m0 .. m0 + 63 of the M kept frames of one signal and every bin.  The operand layout and the stepping
 * are dnn_layer_kernel's: lane l gives v_mfma_f32_32x32x2_f32 A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] and
 * finds D[i = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][j = l & 31] in register r; K enters one accumulator in ascending order, 16 at
 * a time through LDS, so each accumulator is the chain of step d from acc = 0.  Wave w owns bin tiles w and w + 4 (wave 3 has
 * one) for both 32-row halves, the cosine and the sine tile of a bin in the same lane and register: eight accumulators.
 * The A tile is formed while staging: element (m, n) is w[n] z[128 m + n], z the overlap-add of step c gathered through keep[].
 * Then p[k] goes to LDS (over the staging tiles), and a thread per (row, band) adds its bins in order. */
__global__ __launch_bounds__(256, 2) void stoi_band_kernel(StoiArgs a)
{
    __shared__ __attribute__((aligned(16))) float smem[kStoiTileRows * kPd]; /* staging: As [64][20] + Bs [448][20]; then P [64][225] */
    __shared__ int kp[kStoiTileRows + 2];                                     /* keep[m0 - 1 .. m0 + 64], -1 where there is none */
    static_assert(kStoiTileRows * kPd >= (kStoiTileRows + kStoiBasisRows) * kLd, "the power tile covers the staging tiles");
    float(*As)[kLd] = reinterpret_cast<float(*)[kLd]>(smem);
    float(*Bs)[kLd] = reinterpret_cast<float(*)[kLd]>(smem + kStoiTileRows * kLd);
    float(*P)[kPd] = reinterpret_cast<float(*)[kPd]>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lk = lane >> 5;
    const long long item = blockIdx.x;
    const int u = owner_of(a.band_tiles, a.n_utt, item);
    const int M = a.kept[u];
    const int m0 = (int)(item - a.band_tiles[u]) * kStoiTileRows;
    if (m0 >= M) return; /* the whole workgroup: before any barrier */
    const long long f0 = a.frame_cum[u], total = a.frame_cum[a.n_utt];
    const float *x = a.x10 + (blockIdx.y ? a.x_offsets[a.n_utt] : 0) + a.x_offsets[u];
    if (tid < kStoiTileRows + 2) {
        const int m = m0 - 1 + tid;
        kp[tid] = m >= 0 && m < M ? a.keep[f0 + m] : -1;
    }
    __syncthreads();

    f32x16 acc[2][2][2]; /* [bin tile w + 4 t][row half][cosine, sine] */
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][tm][s][r] = 0.0f;

    const int ar = tid >> 2, ac = 4 * (tid & 3); /* this thread's float4 of the A tile: row ar, columns ac .. ac + 3 */
    const bool row_on = m0 + ar < M;
    for (int k0 = 0; k0 < 256; k0 += kStoiTileK) {
        /* A: frame m = m0 + ar covers blocks m (n < 128) and m + 1; block j is w[nn + 128] x10[128 keep[j - 1] + nn + 128] +
         * w[nn] x10[128 keep[j] + nn], a missing neighbour contributing nothing */
        {
            const int n = k0 + ac, nn = n & 127, blk = ar + (n >> 7); /* kp[blk] is keep[j - 1], kp[blk + 1] keep[j] */
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (row_on) {
                const int prev = kp[blk], cur = kp[blk + 1];
                float4 xp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xc = xp;
                if (prev >= 0) xp = *reinterpret_cast<const float4 *>(x + 128LL * prev + nn + 128);
                if (cur >= 0) xc = *reinterpret_cast<const float4 *>(x + 128LL * cur + nn);
                const float fp[4] = {xp.x, xp.y, xp.z, xp.w}, fc[4] = {xc.x, xc.y, xc.z, xc.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float tp = __fmul_rn(kW[nn + e + 128], fp[e]), tc = __fmul_rn(kW[nn + e], fc[e]);
                    const float z = prev < 0 ? tc : cur < 0 ? tp : __fadd_rn(tp, tc);
                    v[e] = __fmul_rn(kW[n + e], z);
                }
            }
            *reinterpret_cast<float4 *>(&As[ar][ac]) = make_float4(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int i = 0; i < kStoiBasisRows / 64; ++i) {
            const int p = tid + 256 * i, r = p >> 2, c4 = 4 * (p & 3);
            *reinterpret_cast<float4 *>(&Bs[r][c4]) = *reinterpret_cast<const float4 *>(a.basis + r * 256 + k0 + c4);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kStoiTileK / 2; ++kk) { /* ascending k: 2 kk (lanes 0..31) then 2 kk + 1 (lanes 32..63) */
            const float a0 = As[li][2 * kk + lk], a1 = As[32 + li][2 * kk + lk];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int tb = wave + 4 * t;
                if (tb < kStoiBinTiles) {
                    const float bc = Bs[64 * tb + li][2 * kk + lk], bs = Bs[64 * tb + 32 + li][2 * kk + lk];
                    acc[t][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bc, acc[t][0][0], 0, 0, 0);
                    acc[t][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bs, acc[t][0][1], 0, 0, 0);
                    acc[t][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bc, acc[t][1][0], 0, 0, 0);
                    acc[t][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bs, acc[t][1][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    /* p[k] = im im + re re, over the staging tiles (every wave is past the last barrier of the loop) */
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int tb = wave + 4 * t;
        if (tb < kStoiBinTiles) {
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float re = acc[t][tm][0][r], im = acc[t][tm][1][r];
                    P[32 * tm + (r & 3) + 8 * (r >> 2) + 4 * lk][32 * tb + li] = __fadd_rn(__fmul_rn(im, im), __fmul_rn(re, re));
                }
        }
    }
    __syncthreads();
    float *out = a.bands + ((blockIdx.y ? total : 0) + f0) * kStoiBands;
    for (int idx = tid; idx < kStoiTileRows * kStoiBands; idx += 256) {
        const int row = idx / kStoiBands, j = idx - row * kStoiBands;
        if (m0 + row >= M) break; /* idx ascends with row */
        float s = 0.0f;
        for (int k = kLo[j]; k < kLo[j + 1]; ++k) s = __fadd_rn(s, P[row][k - kStoiBin0]);
        out[(long long)(m0 + row) * kStoiBands + j] = sqrtf(s);
    }
}

/* ---- step e ---------------------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void stoi_segment_kernel(StoiArgs a)
{
    const long long item = blockIdx.x;
    const int u = owner_of(a.seg_tiles, a.n_utt, item);
    const long long M = a.kept[u], S = M > kStoiSegment - 1 ? M - (kStoiSegment - 1) : 0;
    const long long t = (item - a.seg_tiles[u]) * kStoiItems + threadIdx.x;
    if (t >= kStoiBands * S) return;
    const long long s = t / kStoiBands;
    const int j = (int)(t - s * kStoiBands);
    const float *X = a.bands + (a.frame_cum[u] + s) * kStoiBands + j;
    const float *Y = X + a.frame_cum[a.n_utt] * kStoiBands;
    float xs[kStoiSegment], ys[kStoiSegment];
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int f = 0; f < kStoiSegment; ++f) {
        xs[f] = X[f * kStoiBands], ys[f] = Y[f * kStoiBands];
        sx = __fadd_rn(sx, __fmul_rn(xs[f], xs[f]));
        sy = __fadd_rn(sy, __fmul_rn(ys[f], ys[f]));
    }
    float d = 0.0f;
    if (sy != 0.0f) {
        const float al = sqrtf(__fdiv_rn(sx, sy));
        float mx = 0.0f, my = 0.0f;
#pragma unroll
        for (int f = 0; f < kStoiSegment; ++f) {
            const float tt = __fmul_rn(al, ys[f]), c = __fmul_rn(SEA_STOI_CLIP, xs[f]);
            ys[f] = tt < c ? tt : c;
            mx = __fadd_rn(mx, xs[f]);
            my = __fadd_rn(my, ys[f]);
        }
        mx = __fdiv_rn(mx, 30.0f);
        my = __fdiv_rn(my, 30.0f);
        float num = 0.0f, vx = 0.0f, vy = 0.0f;
#pragma unroll
        for (int f = 0; f < kStoiSegment; ++f) {
            const float dx = __fsub_rn(xs[f], mx), dy = __fsub_rn(ys[f], my);
            num = __fadd_rn(num, __fmul_rn(dx, dy));
            vx = __fadd_rn(vx, __fmul_rn(dx, dx));
            vy = __fadd_rn(vy, __fmul_rn(dy, dy));
        }
        const float den = __fmul_rn(sqrtf(vx), sqrtf(vy));
        d = den > 0.0f ? __fdiv_rn(num, den) : 0.0f;
    }
    a.d[a.seg_cum[u] * kStoiBands + t] = d;
}

/* ---- step f: one wave per utterance ---------------------------------------------------------------------------------------
 * stoi_sum in the shape of one wave, as score_finish_kernel's seg_sum: p[l] over the terms 64 i + l in ascending i, then the
 * lanes in ascending l */
__global__ __launch_bounds__(64) void stoi_finish_kernel(StoiArgs a)
{
    const int lane = threadIdx.x, u = blockIdx.x;
    const long long M = a.kept[u], terms = M > kStoiSegment - 1 ? kStoiBands * (M - (kStoiSegment - 1)) : 0;
    const float *d = a.d + a.seg_cum[u] * kStoiBands;
    double p = 0.0;
    for (long long i = lane; i < terms; i += 64) p += (double)d[i];
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += __shfl(p, l);
    if (lane == 0) a.stoi_sum[u] = s;
}

} // namespace sea
