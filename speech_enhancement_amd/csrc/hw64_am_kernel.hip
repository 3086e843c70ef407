/*
 * hw64_am_kernel.hip -- the Hu-Wang estimator's AM labels and final grouping at 16 kHz on the 64-channel bank, gfx950:
 * createIBM():89-106 of function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp at the constants of resyth_64sub_IBM/cpp/
 * HuWang.h (NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320, SAMPLING_FREQUENCY 16000), that is computeAM:1146-1317 (amPatt, hilbert,
 * computeAMRate, sinModel, with kaiserPara / kaiserBandPass / bessi0 / fft:1553-1677), finalSeg:1321-1494 (reSegmentation,
 * develope) and the binarisation.  The mapping is hw25_am_kernel.hip's.  Those functions hold no literal channel count or
 * rate, so what the constants change is restated, not templated: the pattern, rate and final-grouping kernels, and the FFT's
 * head; the FFT's global stages and the normalisation share their bodies with the 25-band unit (hw25_device.h).  A first form,
 * not tuned.  DESIGN.md section 5.18.
 *
 *   hw64_am_prepare_kernel    per utterance: N of the FFT, whether the stage runs at all, the status flags; the outputs of an
 *                             utterance that skips the stage are zeroed here
 *   hw64_am_patt_kernel       amPatt: per block of five frames (800 samples) the Kaiser band-pass for the block's mean pitch,
 *                             up to 1119 taps computed in the workgroup (lane = tap), then the FIR over max (gOut, 0)
 *   hw64_am_fft_head_kernel   fft's bit reversal and its stages 1..12 on 4096 points in LDS
 *   hw64_am_fft_stage_kernel  one of the stages 13..18 over global memory
 *   hw64_am_norm_kernel       the pattern over its envelope, computeAM:1177-1178
 *   hw64_am_rate_kernel       computeAMRate + sinModel, lane = (frame, channel), the 320-sample loops inside the lane: the
 *                             window of frame f is [160 (f - 1), 160 (f + 1)), exactly two hops
 *   hw64_finalseg_kernel      finalSeg and the binarisation, one wave per utterance; a channel is a lane of the WHOLE wave:
 *                             64-bit ballots, nothing masked to the channel count
 *
 * Types as in hw25_am_kernel.hip: every expression keeps the type the reference's C++ gives it (-ffp-contract=off); sinModel's
 * cosf / sinf / atanf are the double functions rounded to float, so ratio is compared with a tolerance, everything before it
 * bit for bit.
 */
#include "../../include/sea_mi355x.h"
#include "hw25_device.h"
#include "sea_device.h"
#include "sea_kernels.h"

namespace sea {

namespace {

constexpr int kCh = SEA_HW64_NCHAN, kHop = SEA_HW64_HOP, kWin = SEA_HW64_WINDOW;
constexpr int kBlock = 5 * kHop; /* amPatt's blocks of five frames */
constexpr int kMaxTaps = SEA_HW64_AM_MAXTAPS;
constexpr int kLdsLog2 = SEA_HW25_AM_LDS_LOG2;
constexpr int kFs = 16000;                                 /* SAMPLING_FREQUENCY */
constexpr double kPi = 3.1415926535897932384626433832795; /* HuWang.h:7 */
static_assert(kCh == 64, "a channel is a lane of the whole wave");
static_assert(kWin == 2 * kHop, "computeAMRate's window is two hops");

using ChanSet = unsigned long long; /* channel c is bit c */

} // namespace

__global__ __launch_bounds__(64) void hw64_am_prepare_kernel(Hw25AmArgs a)
{
    const int lane = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u], row0 = a.row_offsets[u];
    const long long pitch = (L + 7) & ~7LL;
    const int nfr = L > 0 ? (int)(L / kHop) : 0;
    int flags = 0;
    bool voiced = false, bad = false;
    if (L > SEA_HW25_MAXLEN) {
        flags |= SEA_HW25_AM_TOO_LONG;
    } else {
        for (int f = lane; f < nfr; f += 64) {
            const int p = a.pitch[row0 + f];
            voiced = voiced || p > 0;
            bad = bad || p >= SEA_HW64_DELAYS;
        }
        voiced = __any(voiced);
        bad = __any(bad);
        if (bad) flags |= SEA_HW25_AM_BAD_PITCH;
    }
    /* amPatt's first block is centred on frame 2: fewer than three frames leave the pattern at zero */
    const bool run = flags == 0 && voiced && nfr >= 3;
    if (lane == 0) {
        a.info[u] = run ? fft_log2(L) : -1;
        if (a.status_or)
            a.status[u] |= flags;
        else
            a.status[u] = flags;
    }
    if (run) return;
    const long long cells = (long long)nfr * kCh;
    for (long long i = lane; i < cells; i += 64) {
        a.amcrn[row0 * kCh + i] = 0.0f;
        if (a.ratio) a.ratio[row0 * kCh + i] = 0.0f;
        if (a.seng) a.seng[row0 * kCh + i] = 0.0f;
    }
    if (L > 0)
        for (int c = 0; c < kCh; ++c)
            for (long long n = lane; n < L; n += 64) {
                a.ampatt[off * kCh + c * pitch + n] = 0.0f;
                a.am[off * kCh + c * pitch + n] = 0.0f;
            }
}

/* grid (n_utt, PATT_GRID, 64): workgroup (u, g, c) takes the blocks g, g + PATT_GRID, ... of channel c.  A block is the 800
 * samples of five frames centred on frame 5 b + 2; one without that frame, or without a voiced frame, is zeros.  12 160 bytes
 * of LDS: 1120 taps and the 800 + 1120 samples they reach. */
__global__ __launch_bounds__(256) void hw64_am_patt_kernel(Hw25AmArgs a)
{
    __shared__ float taps[kMaxTaps];
    __shared__ float win[kBlock + kMaxTaps];
    const int tid = threadIdx.x, c = blockIdx.z;
    const AmUtt t = am_utterance<kHop>(a);
    if (t.N < 0) return;
    const long long L = t.L;
    const float *in = a.gout + t.off * kCh + c * t.pitch;
    float *out = a.ampatt + t.off * kCh + c * t.pitch;
    const int nblocks = (int)((L + kBlock - 1) / kBlock);
    const float b0 = bessi0_small(a.tables->am_beta);
    for (int b = blockIdx.y; b < nblocks; b += gridDim.y) {
        const int frame = 5 * b + 2;
        const long long n0 = (long long)b * kBlock;
        /* amPatt:1199-1211: the float mean of the block's positive pitches */
        float mp = 0.0f;
        int count = 0;
        if (frame < t.nfr)
            for (int f = frame - 2; f <= frame + 2; ++f)
                if (f < t.nfr) {
                    const int p = a.pitch[t.row0 + f];
                    if (p > 0) {
                        mp += (float)p;
                        count++;
                    }
                }
        if (count == 0) {
            for (int i = tid; i < kBlock; i += 256)
                if (n0 + i < L) out[n0 + i] = 0.0f;
            continue;
        }
        mp /= (float)count;
        /* kaiserPara (0.01, 0.4 / mp, ..):1553-1569 with a and beta from the tables */
        const float transBw = (float)(0.4 / (double)mp);
        const float len = (float)(((double)a.tables->am_a - 7.95) / 14.36 / (double)transBw);
        int fLength = (int)len;
        if ((double)(len - (float)fLength) < 0.5)
            fLength++;
        else
            fLength += 2;
        if (fLength % 2 != 0) fLength++;
        if (fLength + 1 > kMaxTaps) fLength = kMaxTaps - 2; /* unreachable with pitches up to 200: keeps LDS in bounds */
        const int half = fLength / 2;
        /* kaiserBandPass (filter, fLength, beta, 2.1 / mp, 0.7 / mp):1571-1601 */
        const float wc = (float)(2.1 / (double)mp), wn = (float)(0.7 / (double)mp);
        __syncthreads(); /* the last block's readers are done */
        for (int tim = tid; tim <= fLength; tim += 256) {
            const float k = (float)(2 * tim) / (float)fLength - 1.0f;
            float f = bessi0_small(a.tables->am_beta * sqrtf(1.0f - k * k)) / b0;
            const int step = tim - half;
            if (step != 0)
                f = (float)((double)f * (sin((double)wn * kPi * (double)step) / kPi / (double)step));
            else
                f *= wn;
            taps[tim] = (float)((double)f * (2.0 * cos((double)((float)step * wc) * kPi)));
        }
        /* win[j] holds max (gOut, 0) at sample n0 - half + j, zero outside [0, L): a skipped term and an added zero give the
         * same sum (it starts at +0) */
        for (int j = tid; j < kBlock + fLength; j += 256) {
            const long long tim = n0 - half + j;
            float v = 0.0f;
            if (tim >= 0 && tim < L) {
                v = in[tim];
                v = v > 0.0f ? v : 0.0f;
            }
            win[j] = v;
        }
        __syncthreads();
        for (int i = tid; i < kBlock; i += 256) {
            if (n0 + i >= L) break;
            float sum = 0.0f;
#pragma unroll 4
            for (int m = 0; m <= fLength; ++m) sum += win[i + fLength - m] * taps[m]; /* tim = n + fLength / 2 - m */
            out[n0 + i] = sum;
        }
    }
}

/* grid (n_utt, FFT_GRID, chunk): workgroup (u, g, z) takes the 4096-point pieces g, g + FFT_GRID, ... of channel chan0 + z.
 * Piece k of the bit-reversed array is loaded from the reversed indices, and the stages 1 .. min (N, 12) never leave it.
 * hw25_am_fft_head_kernel's text with this bank's channel count in `pat` and in the channel bound: shared as a body, that
 * kernel's instructions came out in another order. */
__global__ __launch_bounds__(256) void hw64_am_fft_head_kernel(Hw25AmArgs a)
{
    __shared__ float2 x[1 << kLdsLog2];
    const int tid = threadIdx.x, z = blockIdx.z, c = a.chan0 + z;
    const AmUtt t = am_utterance<kHop>(a);
    if (t.N < 0 || c >= kCh) return;
    const int N = t.N, K = N < kLdsLog2 ? N : kLdsLog2;
    const long long sigL = 1LL << N, L = t.L;
    const int points = 1 << K, pieces = (int)(sigL >> K);
    const long long base = t.off * a.chunk * 2 + (long long)z * 2 * t.pitch;
    const float *pat = a.ampatt + t.off * kCh + c * t.pitch;
    const float2 *src = a.fa + base;
    float2 *dst = (a.inverse ? a.fb : a.fa) + base;
    const float sign = a.inverse ? -1.0f : 1.0f; /* the inverse's twiddles are the conjugates */
    for (int piece = blockIdx.y; piece < pieces; piece += gridDim.y) {
        __syncthreads();
        for (int i = tid; i < points; i += 256) {
            const unsigned gi = (unsigned)piece * (unsigned)points + (unsigned)i;
            const long long s = (long long)(__brev(gi) >> (32 - N));
            float2 v = make_float2(0.0f, 0.0f);
            if (!a.inverse) {
                if (s < L) v.x = pat[s]; /* computeAM:1170-1174 */
            } else if (s <= sigL / 2) {  /* hilbert:1244-1254: bins 0 and sigL / 2 as they are, the ones between doubled */
                v = src[s];
                if (s != 0 && s != sigL / 2) {
                    v.x *= 2.0f;
                    v.y *= 2.0f;
                }
            }
            x[i] = v;
        }
        __syncthreads();
        for (int n = 1; n <= K; ++n) {
            const int period = 1 << (n - 1);
            const float2 *tw = a.tw + (period - 1);
            for (int b = tid; b < points / 2; b += 256) {
                const int j = b & (period - 1);
                const int i = ((b >> (n - 1)) << n) + j;
                const float uR = tw[j].x, uI = sign * tw[j].y;
                const float2 lo = x[i], hi = x[i + period];
                const float tmpR = hi.x * uR - hi.y * uI; /* fft:1663-1669 */
                const float tmpI = hi.x * uI + hi.y * uR;
                x[i + period] = make_float2(lo.x - tmpR, lo.y - tmpI);
                x[i] = make_float2(lo.x + tmpR, lo.y + tmpI);
            }
            __syncthreads();
        }
        for (int i = tid; i < points; i += 256) dst[(long long)piece * points + i] = x[i];
    }
}

/* stage a.stage (13 .. 18) in place over global memory; this body and the next are the two banks' (hw25_device.h) */
__global__ __launch_bounds__(256) void hw64_am_fft_stage_kernel(Hw25AmArgs a) { am_fft_stage<kCh, kHop>(a); }

/* computeAM:1177-1178 */
__global__ __launch_bounds__(256) void hw64_am_norm_kernel(Hw25AmArgs a) { am_norm<kCh, kHop>(a); }

/* grid (n_utt, RATE_GRID): computeAMRate:1259-1287 and sinModel:1289-1317, lane = (frame, channel).  cosf, sinf and atanf
 * are the double functions rounded to float. */
__global__ __launch_bounds__(64) void hw64_am_rate_kernel(Hw25AmArgs a)
{
    const AmUtt t = am_utterance<kHop>(a);
    if (t.N < 0) return;
    const int cells = t.nfr * kCh;
    for (int i = blockIdx.y * 64 + threadIdx.x; i < cells; i += gridDim.y * 64) {
        const int frame = i / kCh, c = i % kCh;
        const long long shift = (long long)(frame - 1) * kHop;
        const float *sig = a.am + t.off * kCh + c * t.pitch + shift;
        float sEng = 0.0f;
        if (frame < t.nfr - 1 && frame > 0)
            for (int tim = 0; tim < kWin; ++tim) sEng += sig[tim] * sig[tim];
        const int p = a.pitch[t.row0 + frame];
        float ratio = 0.0f, label = 0.0f;
        if (p > 0 && sEng > 0.0f) {
            float freq = (float)kFs / (float)p;
            freq = (float)((double)freq * (2 * kPi / kFs));
            float pa = 0.0f, pb = 0.0f;
            for (int tim = 0; tim < kWin; ++tim) {
                const double arg = (double)(freq * (float)tim);
                pa += (float)cos(arg) * sig[tim];
                pb += (float)sin(arg) * sig[tim];
            }
            const float phase = (pa == 0.0f) ? (float)(kPi / 2) : (float)(double)(float)atan((double)(-pb / pa));
            float error1 = 0.0f, error2 = 0.0f;
            for (int tim = 0; tim < kWin; ++tim) {
                const float s = 1.0f * (float)cos((double)(freq * (float)tim + phase));
                error1 += (sig[tim] - s) * (sig[tim] - s);
                error2 += (sig[tim] + s) * (sig[tim] + s);
            }
            const float error = error1 < error2 ? error1 : error2;
            ratio = error / sEng;
            label = ((double)ratio > 0.20) ? 0.0f : 1.0f; /* THETAE */
        }
        a.amcrn[t.row0 * kCh + i] = label;
        if (a.ratio) a.ratio[t.row0 * kCh + i] = ratio;
        if (a.seng) a.seng[t.row0 * kCh + i] = sEng;
    }
}

/* ---- finalSeg ------------------------------------------------------------------------------------------------------------- */
namespace {

struct FinalScr {
    int *lab, *key, *lo, *hi, *m, *g; /* [F][64] each */
};

/* reSegmentation:1390-1440 on m: the components that hold a unit whose two time neighbours are marked (the reference's
 * segments) and span at least MIN_SEG_LENGTH frames stay, everything else is cleared.  Returns the number of segments.
 * F * 64 is a multiple of the wave: every lane holds a unit in every pass. */
__device__ __forceinline__ int re_segmentation(const FinalScr &s, int F, int lane)
{
    const int ncell = F * kCh;
    int *m = s.m;
    for (int i = lane; i < ncell; i += 64) {
        s.lab[i] = m[i] ? i : kHw25None;
        s.key[i] = kHw25None;
        s.lo[i] = F;
        s.hi[i] = 0;
    }
    lanes_fence();
    hw64_label_components(s.lab, F, lane);
    lanes_fence();
    for (int i = lane; i < ncell; i += 64) {
        const int f = i / kCh;
        if (!m[i]) continue;
        const int root = s.lab[i];
        atomicMin(&s.lo[root], f);
        atomicMax(&s.hi[root], f);
        if (f >= 1 && f <= F - 2 && m[i - kCh] && m[i + kCh]) atomicMin(&s.key[root], i);
    }
    lanes_fence();
    int count = 0;
    for (int i = lane; i < ncell; i += 64) count += __popcll(__ballot(s.lab[i] == i && s.key[i] != kHw25None));
    for (int i = lane; i < ncell; i += 64) {
        int keep = 0;
        if (m[i]) {
            const int root = s.lab[i];
            keep = (s.key[root] != kHw25None && s.hi[root] - s.lo[root] + 1 >= 5) ? 1 : 0;
        }
        m[i] = keep;
    }
    lanes_fence();
    return count;
}

/* develope:1442-1494: the reference sweeps in place until nothing changes; the fixpoint is the closure of {g == v} over
 * 4-neighbours with m set, whatever the sweep order.  Lane = channel: a frame takes v from the frame before it in sweep
 * direction, then v spreads along the frame's marked channels, over all 64 lanes. */
__device__ __forceinline__ void develope(const FinalScr &s, int F, int v, int lane)
{
    bool again = true;
    while (again) {
        bool changed = false;
        for (int dir = 0; dir < 2; ++dir) {
            ChanSet carry = 0;
            for (int k = 0; k < F; ++k) {
                const int f = dir ? F - 1 - k : k;
                const bool isv = s.g[f * kCh + lane] == v;
                const ChanSet V0 = __ballot(isv), M = __ballot(s.m[f * kCh + lane] != 0);
                ChanSet V = V0 | (carry & M), prev;
                do {
                    prev = V;
                    V |= ((V << 1) | (V >> 1)) & M;
                } while (V != prev);
                if (((V >> lane) & 1ull) && !isv) {
                    s.g[f * kCh + lane] = v;
                    changed = true;
                }
                carry = V;
            }
        }
        again = __any(changed);
    }
    lanes_fence();
}

} // namespace

__global__ __launch_bounds__(64) void hw64_finalseg_kernel(Hw25FinalArgs a)
{
    const int lane = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long L = a.lengths[u], row0 = a.row_offsets[u];
    const int F = L > 0 ? (int)(L / kHop) : 0, ncell = F * kCh;
    int *block = a.rowscr + row0 * SEA_HW64_FINAL_SCRATCH_WORDS;
    const FinalScr s = {block, block + ncell, block + 2 * ncell, block + 3 * ncell, block + 4 * ncell, block + 5 * ncell};
    const float *grp = a.grp + row0 * kCh, *am = a.amcrn + row0 * kCh, *cross = a.cross_ev + row0 * kCh, *pr = a.pratio + row0 * kCh;
    float *stages = a.stages ? a.stages + row0 * (SEA_HW25_FINAL_STAGES * kCh) : nullptr;
    auto put_stage = [&](int k) {
        if (stages)
            for (int i = lane; i < ncell; i += 64) stages[(long long)k * ncell + i] = (float)s.g[i];
    };
    bool too_many = false;
    /* in the whole estimator: an utterance whose AM stage was refused (too long, a pitch out of range) gets a zero mask */
    const bool refused = a.status_or && (a.status[u] & (SEA_HW25_AM_TOO_LONG | SEA_HW25_AM_BAD_PITCH)) != 0;
    if (F >= 3 && !refused) {
        /* finalSeg:1330-1338: segments for unresolved harmonics */
        for (int i = lane; i < ncell; i += 64) {
            s.g[i] = (int)grp[i];
            s.m[i] = (grp[i] == 0.0f && am[i] != 0.0f && (double)cross[i] > 0.985) ? 1 : 0;
        }
        lanes_fence();
        too_many = re_segmentation(s, F, lane) > SEA_HW25_MAX_SEGMENTS;
        for (int i = lane; i < ncell; i += 64) s.g[i] += s.m[i] * 2;
        lanes_fence();
        put_stage(0);
        /* :1341-1352 */
        for (int i = lane; i < ncell; i += 64) s.m[i] = (s.g[i] == 1 && (double)pr[i] > 0.85) ? 1 : 0;
        lanes_fence();
        too_many = re_segmentation(s, F, lane) > SEA_HW25_MAX_SEGMENTS || too_many;
        for (int i = lane; i < ncell; i += 64)
            if (s.g[i] == 1 && (double)pr[i] > 0.85) s.g[i] = s.m[i] == 1 ? 1 : -2;
        lanes_fence();
        put_stage(1);
        /* :1355-1366 */
        for (int i = lane; i < ncell; i += 64) s.m[i] = (s.g[i] == 1 && (double)pr[i] <= 0.85) ? 1 : 0;
        lanes_fence();
        too_many = re_segmentation(s, F, lane) > SEA_HW25_MAX_SEGMENTS || too_many;
        for (int i = lane; i < ncell; i += 64)
            if (s.g[i] == 1 && (double)pr[i] <= 0.85) s.g[i] = s.m[i] == 1 ? -1 : -2;
        lanes_fence();
        put_stage(2);
        /* :1368-1379 */
        for (int i = lane; i < ncell; i += 64) s.m[i] = s.g[i] == -2 ? 1 : 0;
        lanes_fence();
        develope(s, F, -1, lane);
        for (int i = lane; i < ncell; i += 64)
            if (s.g[i] == -2 || s.g[i] == 2) s.g[i] = 1;
        lanes_fence();
        put_stage(3);
        /* :1381-1385 */
        for (int i = lane; i < ncell; i += 64) s.m[i] = (am[i] == 1.0f && s.g[i] == 0) ? 1 : 0;
        lanes_fence();
        develope(s, F, 1, lane);
        put_stage(4);
    }
    if (F < 3 || refused || too_many) {
        /* no segment can exist, or more than the reference's list holds: every output of the utterance is zero */
        for (int i = lane; i < ncell; i += 64) {
            a.mask[row0 * kCh + i] = 0.0f;
            if (a.grp_final) a.grp_final[row0 * kCh + i] = 0.0f;
        }
        if (stages)
            for (int i = lane; i < SEA_HW25_FINAL_STAGES * ncell; i += 64) stages[i] = 0.0f;
    } else {
        for (int i = lane; i < ncell; i += 64) {
            a.mask[row0 * kCh + i] = s.g[i] > 0 ? 1.0f : 0.0f; /* createIBM:103 */
            if (a.grp_final) a.grp_final[row0 * kCh + i] = (float)s.g[i];
        }
    }
    if (lane == 0) {
        const int flags = too_many ? SEA_HW25_FINAL_TOO_MANY_SEGMENTS : 0;
        if (a.status_or)
            a.status[u] |= flags;
        else
            a.status[u] = flags;
    }
}

} // namespace sea
