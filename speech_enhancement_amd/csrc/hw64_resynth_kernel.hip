/*
 * hw64_resynth_kernel.hip -- resynthesis() of the Hu-Wang estimator at 16 kHz on its 64-channel gammatone bank, gfx950
 * (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1498-1549 compiled against resyth_64sub_IBM/cpp/HuWang.h:
 * NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320).  A first form with the shape of hw25_resynth_kernel.hip, not tuned.
 *
 * Per channel the reference divides gOut by midEarCoeff, filters it backwards in time with the analysis filter, divides
 * again, weights the result with the overlap-add window of the frames whose unit is set, and adds the 64 channels in order.
 * Here one wave takes one utterance, in tiles of 64 samples from the last tile to the first:
 *
 *   lanes 0..63 = channel   divide -> gammaToneFilter step -> divide for the tile's samples, latest first, gOut read in groups
 *                           of 8 samples as two 16-byte loads with the next group requested ahead; `reverse` goes to an LDS
 *                           tile [64][64] with a row stride of 65 words (no bank conflict on either side)
 *   lanes 0..63 = sample    sum over the channels 0..63 in order from +0.0f of weight * reverse, every channel multiplied and
 *                           added whatever its weight; coalesced float store and, on request, the x86-64 (short) conversion
 *
 * WINDOW is exactly two hops, so a set frame f adds its rising half on [160 (f - 1), 160 f) (not for f = 0) and its falling
 * half on [160 f, 160 f + 160), and nothing else: the weight of a channel at sample 160 k + o depends on o and on whether the
 * frames k and k + 1 exist and are set, one of the 640 floats of sea_hw64_ola_tables (sea_tables.c), held in LDS.  The largest
 * index a frame writes is 160 (F - 1) + 159 < L: the reference stays inside its arrays, there is nothing to drop, and the tail
 * [160 F, L) has weight 0.  A tile touches at most two values of k, so three mask rows: every lane loads its channel's unit of
 * each before the recurrence, and a ballot per row leaves the row as 64 bits -- all 64 lanes are channels, nothing is narrowed.
 * Every product and sum is rounded on its own (-ffp-contract=off); the divisions are the compiler's correctly rounded ones.
 * gOut is only read; no intermediate goes to global memory.
 */
#include "hw25_device.h"
#include "sea_device.h"
#include "sea_kernels.h"

namespace sea {

namespace {

constexpr int kCh = SEA_HW64_NCHAN, kHop = SEA_HW64_HOP;
constexpr int kTile = kResynthTile, kGroup = kResynthGroup, kStride = kResynthStride; /* hw25_device.h, with resynth_group */
static_assert(kCh == kTile, "a lane is a channel in the first half and a sample in the second");
static_assert(kTile <= kHop, "a tile must not reach a third hop");

} // namespace

__global__ __launch_bounds__(64) void hw64_resynth_kernel(Hw64ResynthArgs a)
{
    __shared__ float rev[kCh * kStride];
    __shared__ float wtab[SEA_HW64_OLA_WEIGHTS];
    const int lane = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u];
    if (L <= 0) return;
    const long long pitch = (L + 7) & ~7LL, nfr = L / kHop, row0 = a.row_offsets[u];
    const sea_hw64_tables &t = *a.tables;
    for (int i = lane; i < SEA_HW64_OLA_WEIGHTS; i += kTile) wtab[i] = t.olaW[i];
    const int c = lane;
    const float f1 = t.f1[c], f2 = t.f2[c], gain = t.gain[c], ear = t.midEar[c];
    const float *src = a.gout + off * kCh + c * pitch;
    const float *mask = a.mask + row0 * kCh + c;
    const float thr = a.threshold;
    float *row = rev + c * kStride;
    Gt25 s = {};
    /* gout holds `pitch` floats per channel: the reads of the last group stay inside the channel's padded stretch */
    float4 n0, n1;
    {
        const long long tg = (L - 1) & ~(long long)(kGroup - 1);
        n0 = *reinterpret_cast<const float4 *>(src + tg);
        n1 = *reinterpret_cast<const float4 *>(src + tg + 4);
    }
    for (long long tile = (L - 1) / kTile; tile >= 0; --tile) {
        const long long t0 = tile * kTile;
        const long long k0 = t0 / kHop; /* the frame of the tile's first sample; its last one lies in k0 or k0 + 1 */
        /* the units of the frames k0 .. k0 + 2; a frame that does not exist is not set */
        float mv[3];
        bool have[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const long long f = k0 + r;
            have[r] = f < nfr;
            mv[r] = have[r] ? mask[f * kCh] : 0.0f;
        }
#pragma unroll 1
        for (int gi = kTile / kGroup - 1; gi >= 0; --gi) {
            const long long tg = t0 + gi * kGroup;
            if (tg >= L) continue;
            const float x[kGroup] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
            if (tg >= kGroup) {
                n0 = *reinterpret_cast<const float4 *>(src + tg - kGroup);
                n1 = *reinterpret_cast<const float4 *>(src + tg - kGroup + 4);
            }
            if (tg + kGroup <= L) resynth_group<false>(s, x, tg, L, f1, f2, gain, ear, row);
            else resynth_group<true>(s, x, tg, L, f1, f2, gain, ear, row);
        }
        unsigned long long set[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) set[r] = __ballot(have[r] && mv[r] > thr); /* NaN and -0.0 > 0 are false */
        __syncthreads();
        const long long tt = t0 + lane;
        if (tt < L) {
            const long long k = tt / kHop;
            const int o = (int)(tt - k * kHop);
            const bool next = k != k0;
            const unsigned long long b0 = next ? set[1] : set[0], b1 = next ? set[2] : set[1]; /* frame k, frame k + 1 */
            const float *w = wtab + o * 4;
            float sum = 0.0f;
#pragma unroll
            for (int ch = 0; ch < kCh; ++ch) {
                const unsigned bits = (unsigned)((b0 >> ch) & 1ull) | ((unsigned)((b1 >> ch) & 1ull) << 1);
                sum += w[bits] * rev[ch * kStride + lane];
            }
            if (a.out_f32) a.out_f32[off + tt] = sum;
            if (a.out_i16) a.out_i16[off + tt] = resynth_to_short(sum);
        }
        __syncthreads();
    }
}

} // namespace sea
