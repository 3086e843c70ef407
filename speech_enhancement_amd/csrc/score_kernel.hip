/*
 * score_kernel.hip -- objective scores of enhanced audio against clean audio and of an estimated mask against the ideal one,
 * gfx950:
 *
 *   score_frames_kernel <HOP>   Srr, See, Sre of every half-frame as exact integers; per 20 ms frame the segmental-SNR term
 *                               d = clamp ((ln (srr + 1) - ln (n + 1)) 10 / ln 10, -10, 35), n = srr - 2 sre + see
 *   score_finish_kernel         a wave per utterance: the utterance's three integers (wave partials + the tail past the last
 *                               half-frame), seg_sum as one in-order double chain per lane, seg_frames
 *   mask_score_kernel           the 2 x 2 table of (estimated unit on, ideal unit on) from wave ballots
 *
 * Every value is pinned on the bits by the plain-C model tests/score_model_driver.c, which includes the same dnn_math.h.
 * Integers are summed in any order; the only floating-point sums are the per-lane chains of score_finish_kernel and the
 * 64-term chain over the lanes, both in a fixed order.  No floating-point atomic.
 */
#include "dnn_math.h"
#include "score_kernels.h"

namespace sea {

namespace {

constexpr uint32_t kSkipped = 0x7fc00000u; /* frame_db of a frame whose reference is silent */

/* the utterance that owns item `item` of a prefix table with cum[0] = 0 <= item < cum[n]: the largest u with cum[u] <= item
 * (an utterance without an item repeats its neighbour's entry and is passed over) */
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

__device__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

} // namespace

/* ---- frames ------------------------------------------------------------------------------------------------------------------
 * As cochleagram64_kernel: lane l of wave tile t sums half-frame h = 63 t + l (HOP samples = HOP / 8 16-byte loads of each
 * signal; utterance bases are multiples of 8 samples and HOP is one, so every load is aligned), frame f is half-frame f plus
 * half-frame f + 1, fetched from the next lane.  Only whole half-frames h < H = L / HOP are read: HOP (h + 1) <= L, so no load
 * passes the utterance's end and the staging padding is never part of a sum. */
template <int HOP>
__global__ __launch_bounds__(256) void score_frames_kernel(ScoreArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = blockIdx.x;
    const int u = owner_of(a.tile_cum, a.n_utt, item);
    const long long H = a.lengths[u] / HOP, F = H > 1 ? H - 1 : 0;
    const long long h = ((item - a.tile_cum[u]) * kScoreWaves + wave) * kScoreWaveHalves + lane;
    long long srr = 0, see = 0, sre = 0;
    if (h < H) {
        const uint4 *pr = reinterpret_cast<const uint4 *>(a.ref + a.offsets[u] + h * HOP);
        const uint4 *pe = reinterpret_cast<const uint4 *>(a.est + a.offsets[u] + h * HOP);
#pragma unroll 5
        for (int j = 0; j < HOP / 8; ++j) {
            const uint4 vr = pr[j], ve = pe[j];
            const uint32_t dr[4] = {vr.x, vr.y, vr.z, vr.w}, de[4] = {ve.x, ve.y, ve.z, ve.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r0 = (short)(dr[q] & 0xffffu), r1 = (short)(dr[q] >> 16);
                const int e0 = (short)(de[q] & 0xffffu), e1 = (short)(de[q] >> 16);
                srr += (uint32_t)(r0 * r0) + (uint32_t)(r1 * r1); /* two squares: at most 2^31 */
                see += (uint32_t)(e0 * e0) + (uint32_t)(e1 * e1);
                sre += (long long)(r0 * e0) + (long long)(r1 * e1); /* each within +-2^30; their sum may be 2^31 */
            }
        }
    }
    const long long frr = srr + __shfl_down(srr, 1), fee = see + __shfl_down(see, 1), fre = sre + __shfl_down(sre, 1);
    if (lane < kScoreWaveHalves && h < F) {
        float d = sea_dnn_float(kSkipped);
        if (frr != 0) {
            const long long n = frr - 2 * fre + fee; /* the sum of (r - e)^2: exact, >= 0, below 2^41 */
            d = __fmul_rn(__fsub_rn(sea_lnf((float)(frr + 1)), sea_lnf((float)(n + 1))), 0x1.15f2cep+2f);
            d = d < -10.0f ? -10.0f : d > 35.0f ? 35.0f : d;
        }
        a.frame_db[a.frame_offsets[u] + h] = d;
    }
    /* this wave's share of the utterance's sums: the half-frames it owns (lane 63's belongs to the next wave) */
    const bool own = lane < kScoreWaveHalves;
    const long long wrr = wave_sum(own ? srr : 0), wee = wave_sum(own ? see : 0), wre = wave_sum(own ? sre : 0);
    if (lane == 0) {
        long long *p = a.partials + (item * kScoreWaves + wave) * 3;
        p[0] = wrr, p[1] = wee, p[2] = wre;
    }
}

template __global__ void score_frames_kernel<80>(ScoreArgs);
template __global__ void score_frames_kernel<160>(ScoreArgs);

/* ---- one wave per utterance ---------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(64) void score_finish_kernel(ScoreArgs a)
{
    const int lane = threadIdx.x, u = blockIdx.x;
    const long long L = a.lengths[u], H = L / a.hop, F = H > 1 ? H - 1 : 0;
    long long srr = 0, see = 0, sre = 0;
    for (long long t = a.tile_cum[u] * kScoreWaves + lane; t < a.tile_cum[u + 1] * kScoreWaves; t += 64) {
        const long long *p = a.partials + t * 3;
        srr += p[0], see += p[1], sre += p[2];
    }
    const int16_t *ref = a.ref + a.offsets[u], *est = a.est + a.offsets[u];
    for (long long i = H * a.hop + lane; i < L; i += 64) { /* the tail: fewer than hop samples */
        const int r = ref[i], e = est[i];
        srr += r * r, see += e * e, sre += r * e;
    }
    srr = wave_sum(srr), see = wave_sum(see), sre = wave_sum(sre);
    /* seg_sum in the shape of one wave, as dnn_loss_kernel: p[l] over the frames 64 i + l in ascending i, then the lanes in
     * ascending l; a skipped frame adds nothing */
    const float *d = a.frame_db + a.frame_offsets[u];
    double p = 0.0;
    int used = 0;
    for (long long f = lane; f < F; f += 64) {
        const float v = d[f];
        if (sea_dnn_bits(v) != kSkipped) p += (double)v, ++used;
    }
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += __shfl(p, l);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) used += __shfl_xor(used, m);
    if (lane == 0) {
        a.sums[3LL * u] = srr, a.sums[3LL * u + 1] = see, a.sums[3LL * u + 2] = sre;
        a.seg_sum[u] = s;
        a.seg_frames[u] = used;
    }
}

/* ---- masks ---------------------------------------------------------------------------------------------------------------------
 * A workgroup per tile of 64 rows (4096 units of each mask): four float4 of either mask per thread, a unit on iff value >
 * threshold (a NaN is off), the four classes counted per wave from ballots, one integer atomic per class and wave. */
__global__ __launch_bounds__(256) void mask_score_kernel(MaskScoreArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const long long item = blockIdx.x;
    const int u = owner_of(a.tile_cum, a.n_utt, item);
    const long long r0 = a.row_offsets[u], tile = item - a.tile_cum[u];
    const long long left = (a.row_offsets[u + 1] - r0 - tile * kMaskTileRows) * 64; /* units from the tile's start to the end */
    const long long base = (r0 + tile * kMaskTileRows) * 64;
    unsigned c11 = 0, c10 = 0, c01 = 0, c00 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = i * 1024 + tid * 4; /* rows are 64 units: a float4 is inside the utterance or past it as a whole */
        const bool valid = e < left;
        float4 ve = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vi = ve;
        if (valid) {
            ve = *reinterpret_cast<const float4 *>(a.est + base + e);
            vi = *reinterpret_cast<const float4 *>(a.ideal + base + e);
        }
        const float xe[4] = {ve.x, ve.y, ve.z, ve.w}, xi[4] = {vi.x, vi.y, vi.z, vi.w};
        const unsigned long long bv = __ballot(valid);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long be = __ballot(valid && xe[q] > a.t_est), bi = __ballot(valid && xi[q] > a.t_ideal);
            c11 += __popcll(be & bi);
            c10 += __popcll(be & ~bi);
            c01 += __popcll(~be & bi);
            c00 += __popcll(bv & ~be & ~bi);
        }
    }
    if (lane == 0) {
        unsigned long long *c = a.counts + 4LL * u;
        if (c11) atomicAdd(c + 0, (unsigned long long)c11);
        if (c10) atomicAdd(c + 1, (unsigned long long)c10);
        if (c01) atomicAdd(c + 2, (unsigned long long)c01);
        if (c00) atomicAdd(c + 3, (unsigned long long)c00);
    }
}

} // namespace sea
