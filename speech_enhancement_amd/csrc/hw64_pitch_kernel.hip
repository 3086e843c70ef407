/*
 * hw64_pitch_kernel.hip -- the Hu-Wang estimator's initial grouping and pitch tracking at 16 kHz on the 64-channel bank, gfx950:
 * createIBM():79-87 of function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp at the constants of resyth_64sub_IBM/cpp/
 * HuWang.h (NUMBER_CHANNEL 64, MAX_DELAY 201, MIN_DELAY 32, OFFSET 160), that is initGroup:639-702 (with segmentation / search /
 * relationship:466-637) and pitchDtm:795-824.  The mapping is hw25_pitch_kernel.hip's; what the channel count changes is
 * restated, not templated: a channel is a lane of the WHOLE wave, so ballots are 64-bit and nothing is masked to the channel
 * lanes, the segmented minimum runs over 64 lanes, sumAuto deals its 169 delays in three passes.  A first form, not tuned.
 * DESIGN.md section 5.17.
 *
 *   hw64_pitch_max_kernel      per (frame, channel) the maximum of acf[c][32..200].  One wave per frame, lane = delay.
 *   hw64_pitch_segment_kernel  segmentation + initGroup, one wave per utterance, lane = channel in the label propagation
 *   hw64_pitch_frame_kernel    findPitch and / or timeCrn, one wave per frame: lane = delay in sumAuto, lane = channel after
 *   hw64_pitch_regroup_kernel  reGroup (theta), one wave per utterance, lane = frame in relationship2
 *   hw64_pitch_track_kernel    checkPitch, leftDevelope, rightDevelope, linearEstimate: serial over frames, one wave per
 *                              utterance, lane = delay inside sumAuto, lane = channel in the unit tests
 *
 * FORTY CHANNELS.  leftDevelope and rightDevelope say `if (chan<40)` where they compute chan_mark and `for(chan=0; chan<40;
 * chan++)` where they count number2 (HuWang.cpp:969, 1009, 1047, 1087).  On this bank these are real channels: 40..63 never
 * enter chan_mark, hence never chan_mark2, number or the sumAuto inside a Develope, and are not counted in number2.  kDevelope
 * is that bound; it is applied at those four places (two in develope(), which is both functions) and nowhere else.  There are
 * no ghost channels here, so nothing reads the cross array.
 *
 * Every expression keeps the type the reference's C++ gives it, as in hw25_pitch_kernel.hip: pRatio > THETAP in initGroup and
 * acf / mvalue > THETAP are float values against the double 0.95; reGroup's theta is a float; pitchCrn's bounds and the
 * Developes' k1 / k2 are double expressions stored in float variables, clamped at 32 and 200; x / 0 is IEEE.  Sums run over the
 * marked channels in the order 0..63, maxima are first strict maxima.  No kernel modifies acf, pratio_in or mark_in.
 *
 * Scratch: utterance u's block of SEA_HW64_SCRATCH_WORDS words per row at a.rowscr + row_offsets[u] * SEA_HW64_SCRATCH_WORDS
 * (lab, key: [F][64] ints; mraw: [F][64] floats; buf: [F] ints), and a.segse: [n_utt][2][400] ints.  Memory that one lane
 * writes and another lane of the same wave reads later is separated by a fence; inside a serial loop the carried values stay
 * in registers.
 */
#include "../../include/sea_mi355x.h"
#include "hw25_device.h"
#include "sea_device.h"
#include "sea_kernels.h"

namespace sea {

namespace {

constexpr int kCh = SEA_HW64_NCHAN, kDel = SEA_HW64_DELAYS, kHop = SEA_HW64_HOP, kMinDel = SEA_HW64_MINDELAY;
constexpr int kRow = kCh * kDel;
constexpr int kMaxSeg = SEA_HW25_MAX_SEGMENTS;
constexpr double kThetaP = 0.95;
constexpr unsigned long long kDevelope = (1ull << 40) - 1ull; /* the Developes' `chan<40` */
static_assert(kCh == 64, "a channel is a lane of the whole wave");

using ChanSet = unsigned long long; /* channel c is bit c */

__device__ __forceinline__ int popc64(ChanSet m) { return __popcll(m); }

/* sumAuto:862-885 on one frame's acf [64][201]: the channels of `mask` in order per delay (lane = delay), the first strict
 * maximum over [lo, hi) from mvalue = 0; every lane returns it.  mask is the same in every lane. */
__device__ __forceinline__ int sum_auto(const float *acf, ChanSet mask, int lo, int hi, int lane)
{
    float bv = 0.0f;
    int bd = 0;
    for (int d0 = lo; d0 < hi; d0 += 64) {
        const int d = d0 + lane;
        if (d < hi) {
            float sum = 0.0f;
            for (ChanSet m = mask; m; m &= m - 1ull) sum += acf[(__ffsll((long long)m) - 1) * kDel + d];
            if (sum > bv) {
                bv = sum;
                bd = d;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int od = __shfl_xor(bd, off);
        if (ov > bv || (ov == bv && od < bd)) {
            bv = ov;
            bd = od;
        }
    }
    return bd;
}

/* the channels with Grp > 0 and (acf[c][delay] / mvalue) > THETAP: the float quotient against the double constant */
__device__ __forceinline__ ChanSet ratio_mask(const float *acf, const float *mraw, const float *grp, int delay, int lane)
{
    const float q = acf[lane * kDel + delay] / mvalue_of(mraw[lane]);
    return __ballot(grp[lane] > 0.0f && (double)q > kThetaP);
}

/* count[0] / count[1] of segment `id` in one frame: its units with pRatio above / not above the threshold */
template <bool kDouble>
__device__ __forceinline__ void seg_votes(const int *lab, const float *pr, int id, float theta, int &n1, int &n2)
{
    n1 = 0;
    n2 = 0;
    for (int c = 0; c < kCh; ++c)
        if (lab[c] == id) {
            const bool hi = kDouble ? ((double)pr[c] > kThetaP) : (pr[c] > theta);
            n1 += hi ? 1 : 0;
            n2 += hi ? 0 : 1;
        }
}

struct Utt {
    int u, nfr;
    long long row0;
    int *lab, *key, *buf; /* the utterance's scratch block: lab | key | mraw [F][64], buf [F] */
    float *mraw;
};
__device__ __forceinline__ Utt utterance(const Hw64PitchArgs &a)
{
    Utt t;
    t.u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long L = a.lengths[t.u];
    t.nfr = L > 0 ? (int)(L / kHop) : 0;
    t.row0 = a.row_offsets[t.u];
    int *block = a.rowscr + t.row0 * SEA_HW64_SCRATCH_WORDS;
    const long long plane = (long long)t.nfr * kCh;
    t.lab = block;
    t.key = block + plane;
    t.mraw = reinterpret_cast<float *>(block + 2 * plane);
    t.buf = block + 3 * plane;
    return t;
}

/* utterance u's stage block: [5][F] ints (Pitch), then [2][F][64] floats (Grp) */
__device__ __forceinline__ int *stage_pitch(const Hw64PitchArgs &a, const Utt &t, int k)
{
    return a.stages + t.row0 * SEA_HW64_STAGE_WORDS + (long long)k * t.nfr;
}
__device__ __forceinline__ float *stage_grp(const Hw64PitchArgs &a, const Utt &t, int k)
{
    return reinterpret_cast<float *>(a.stages + t.row0 * SEA_HW64_STAGE_WORDS + 5LL * t.nfr) + (long long)k * t.nfr * kCh;
}

/* segment count 0 or a set TOO_MANY bit: the segment kernel wrote zeros, the later kernels leave the utterance alone */
__device__ __forceinline__ bool inactive(int status) { return (status & 0xffff) == 0 || (status & SEA_HW25_TOO_MANY_SEGMENTS); }

} // namespace

__global__ __launch_bounds__(64) void hw64_pitch_max_kernel(Hw64PitchArgs a)
{
    const int lane = threadIdx.x;
    const Utt t = utterance(a);
    for (int frame = blockIdx.y; frame < t.nfr; frame += gridDim.y) {
        const long long row = t.row0 + frame;
        const float *acf = a.acf + row * kRow;
        float keep = 0.0f;
        for (int c = 0; c < kCh; ++c) {
            const float *p = acf + c * kDel + kMinDel + lane;
            float m = -INFINITY;
            const float v0 = p[0], v1 = p[64]; /* delays 32..95, 96..159 */
            if (v0 > m) m = v0;
            if (v1 > m) m = v1;
            if (kMinDel + 128 + lane < kDel) { /* delays 160..200 */
                const float v2 = p[128];
                if (v2 > m) m = v2;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float o = __shfl_xor(m, off);
                if (o > m) m = o;
            }
            if (lane == c) keep = m;
        }
        t.mraw[frame * kCh + lane] = keep;
    }
}

__global__ __launch_bounds__(64) void hw64_pitch_segment_kernel(Hw64PitchArgs a)
{
    __shared__ int sS[kMaxSeg], sE[kMaxSeg], sRel[kMaxSeg];
    const int lane = threadIdx.x;
    const Utt t = utterance(a);
    const int F = t.nfr, ncell = F * kCh;
    int *lab = t.lab, *key = t.key;
    const float *mark = a.mark_in + t.row0 * kCh, *pr = a.pratio_in + t.row0 * kCh;
    int nseg = 0, flags = 0;

    if (F >= 3) {
        for (int i = lane; i < ncell; i += 64) {
            lab[i] = mark[i] != 0.0f ? i : kHw25None;
            key[i] = kHw25None;
        }
        lanes_fence();
        /* ---- components: every marked unit ends with the smallest unit index of its component ---- */
        hw64_label_components(lab, F, lane);
        lanes_fence();
        /* ---- per component its first seed in scan order ---- */
        for (int i = lane; i < ncell; i += 64) {
            const int f = i / kCh;
            if (f >= 1 && f <= F - 2 && mark[i] != 0.0f && mark[i - kCh] != 0.0f && mark[i + kCh] != 0.0f) atomicMin(&key[lab[i]], i);
        }
        lanes_fence();
        /* ---- the segment list: components in the order of their first seeds; key[root] becomes -(index + 1) ---- */
        int count = 0;
        for (int base = 0; base < ncell; base += 64) {
            const int i = base + lane, f = i / kCh; /* ncell is a multiple of 64: i < ncell */
            bool first = false;
            int root = 0;
            if (f >= 1 && f <= F - 2 && mark[i] != 0.0f && mark[i - kCh] != 0.0f && mark[i + kCh] != 0.0f) {
                root = lab[i];
                first = key[root] == i;
            }
            const ChanSet bal = __ballot(first);
            const int idx = count + popc64(bal & ((1ull << lane) - 1ull));
            if (first && idx < kMaxSeg) {
                key[root] = -(idx + 1);
                sS[idx] = F;
                sE[idx] = 0;
            }
            count += popc64(bal);
        }
        lanes_fence();
        __syncthreads();
        if (count > kMaxSeg) {
            flags |= SEA_HW25_TOO_MANY_SEGMENTS;
            nseg = count > 0xffff ? 0xffff : count;
        } else {
            nseg = count;
        }
    }

    float *grp = a.grp + t.row0 * kCh;
    if (nseg == 0 || flags) {
        /* no segment, or more than the reference's list holds: every output of the utterance is zero */
        for (int i = lane; i < ncell; i += 64) {
            grp[i] = 0.0f;
            a.pratio[t.row0 * kCh + i] = 0.0f;
        }
        for (int f = lane; f < F; f += 64) a.pitch[t.row0 + f] = 0;
        if (a.stages)
            for (int i = lane; i < F * SEA_HW64_STAGE_WORDS; i += 64) a.stages[t.row0 * SEA_HW64_STAGE_WORDS + i] = 0;
        if (lane == 0) a.status[t.u] = nseg | flags;
        return;
    }

    /* ---- every unit's segment index (-1: in no segment), sFrame / eFrame ---- */
    for (int i = lane; i < ncell; i += 64) {
        int id = -1;
        if (mark[i] != 0.0f) {
            const int s = key[lab[i]];
            if (s < 0) id = -(s + 1);
        }
        lab[i] = id;
        if (id >= 0) {
            atomicMin(&sS[id], i / kCh);
            atomicMax(&sE[id], i / kCh);
        }
    }
    lanes_fence();
    __syncthreads();
    /* ---- relationship:499-558 ---- */
    int longest = 0, length = 0;
    for (int i = 0; i < nseg; ++i)
        if (sE[i] - sS[i] > length) {
            length = sE[i] - sS[i];
            longest = i;
        }
    const int sL = sS[longest], eL = sE[longest];
    int cnt = 0;
    for (int f0 = sL; f0 <= eL; f0 += 64) {
        const int f = f0 + lane;
        int n1 = 0, n2 = 0;
        if (f <= eL) seg_votes<true>(lab + f * kCh, pr + f * kCh, longest, 0.0f, n1, n2);
        cnt += popc64(__ballot(f <= eL && n1 > n2)) - popc64(__ballot(f <= eL && !(n1 > n2)));
    }
    const int relL = cnt <= 0 ? -1 : 1;
    for (int i = 0; i < nseg; ++i) {
        const int s = sL < sS[i] ? sS[i] : sL, e = eL > sE[i] ? sE[i] : eL;
        int number1 = 0, number2 = 0;
        for (int f0 = s; f0 <= e; f0 += 64) {
            const int f = f0 + lane;
            int n1 = 0, n2 = 0, n3 = 0, n4 = 0;
            if (f <= e) {
                seg_votes<true>(lab + f * kCh, pr + f * kCh, longest, 0.0f, n1, n2);
                seg_votes<true>(lab + f * kCh, pr + f * kCh, i, 0.0f, n3, n4);
            }
            const bool agree = (n1 > n2 && n3 > n4) || (n1 < n2 && n3 < n4);
            number1 += popc64(__ballot(f <= e && agree));
            number2 += popc64(__ballot(f <= e && !agree));
        }
        if (lane == 0) sRel[i] = number1 > number2 * 2 ? relL : -relL;
    }
    __syncthreads();
    /* ---- Grp: only the frames of the longest segment are labelled ---- */
    for (int i = lane; i < ncell; i += 64) {
        const int id = lab[i], f = i / kCh;
        const float g = (id >= 0 && f >= sL && f <= eL) ? (float)sRel[id] : 0.0f;
        grp[i] = g;
        if (a.stages) stage_grp(a, t, 0)[i] = g;
    }
    for (int i = lane; i < nseg; i += 64) {
        a.segse[(long long)t.u * 2 * kMaxSeg + i] = sS[i];
        a.segse[(long long)t.u * 2 * kMaxSeg + kMaxSeg + i] = sE[i];
    }
    if (lane == 0) a.status[t.u] = nseg;
}

__global__ __launch_bounds__(64) void hw64_pitch_frame_kernel(Hw64PitchArgs a)
{
    const int lane = threadIdx.x;
    const Utt t = utterance(a);
    if (inactive(a.status[t.u])) return;
    const bool find = a.mode & SEA_HW25_FRAME_FIND, crn = a.mode & SEA_HW25_FRAME_TIMECRN;
    for (int frame = blockIdx.y; frame < t.nfr; frame += gridDim.y) {
        const long long row = t.row0 + frame;
        const float *acf = a.acf + row * kRow, *mraw = t.mraw + frame * kCh;
        int P;
        if (find) {
            /* findPitch:836-858; with Pitch = 0 the reference divides acf[chan][0], and zeroes a zero */
            const float *grp = a.grp + row * kCh;
            const ChanSet gm = __ballot(grp[lane] > 0.0f);
            P = sum_auto(acf, gm, kMinDel, kDel, lane);
            const int n1 = popc64(gm), n2 = popc64(ratio_mask(acf, mraw, grp, P, lane));
            /* lFrame / rFrame (:838-839) come from sumAuto's result BEFORE the vote zeroes it: kept for the track kernel */
            if (lane == 0) t.buf[frame] = P;
            if (n2 * 2 <= n1) P = 0;
            if (lane == 0) {
                a.pitch[row] = P;
                if (a.stages) stage_pitch(a, t, a.stage)[frame] = P;
            }
        } else {
            P = a.pitch[row];
        }
        if (crn) {
            /* timeCrn:771-790: mp starts at acf[chan][Pitch] */
            float out = 0.0f;
            if (P > 0) {
                const float at = acf[lane * kDel + P], mx = mraw[lane];
                const float mp = mx > at ? mx : at;
                out = at / mp;
            }
            a.pratio[row * kCh + lane] = out;
        }
    }
}

__global__ __launch_bounds__(64) void hw64_pitch_regroup_kernel(Hw64PitchArgs a)
{
    __shared__ int sRel[kMaxSeg];
    const int lane = threadIdx.x;
    const Utt t = utterance(a);
    const int status = a.status[t.u];
    if (inactive(status)) return;
    const int nseg = status & 0xffff, ncell = t.nfr * kCh;
    const int *lab = t.lab;
    const float *pr = a.pratio + t.row0 * kCh;
    const int *sS = a.segse + (long long)t.u * 2 * kMaxSeg, *sE = sS + kMaxSeg;
    /* relationship2:560-582 */
    for (int i = 0; i < nseg; ++i) {
        const int s = sS[i], e = sE[i];
        int number1 = 0, number2 = 0;
        for (int f0 = s; f0 <= e; f0 += 64) {
            const int f = f0 + lane;
            int n1 = 0, n2 = 0;
            if (f <= e) seg_votes<false>(lab + f * kCh, pr + f * kCh, i, a.theta, n1, n2);
            number1 += popc64(__ballot(f <= e && n1 >= n2));
            number2 += popc64(__ballot(f <= e && !(n1 >= n2)));
        }
        if (lane == 0) sRel[i] = number1 >= number2 ? 1 : -1;
    }
    __syncthreads();
    float *grp = a.grp + t.row0 * kCh;
    for (int i = lane; i < ncell; i += 64) {
        const int id = lab[i];
        const float g = id >= 0 ? (float)sRel[id] : 0.0f;
        grp[i] = g;
        if (a.stages && a.stage >= 0) stage_grp(a, t, a.stage)[i] = g;
    }
}

namespace {

/* leftDevelope:954-1030 (step -1) / rightDevelope:1032-1108 (step +1) from `frame` to `last`.  chan_mark lives in a register
 * pair as a channel set; it starts at zeros, and reading it before it was computed is reported.  The pitch and buffer of the
 * frame just handled are carried to the next step in registers. */
__device__ __forceinline__ bool develope(const Hw64PitchArgs &a, const Utt &t, int frame, int last, int step, int lane)
{
    const bool left = step < 0;
    if (left ? frame < last : frame > last) return false;
    int *pitch = a.pitch + t.row0, *buf = t.buf;
    const float *grp0 = a.grp + t.row0 * kCh, *acf0 = a.acf + t.row0 * kRow, *mraw0 = t.mraw;
    ChanSet chan_mark = 0;
    bool computed = false, unset = false;
    int pn = pitch[frame - step], bn = buf[frame - step];
    for (; left ? frame >= last : frame <= last; frame += step) {
        const int nb = frame - step;
        if (pn) {
            /* :966-979 / :1044-1057: chan_mark[chan] = 0 for every channel, the test only `if (chan<40)` */
            chan_mark = ratio_mask(acf0 + (long long)nb * kRow, mraw0 + nb * kCh, grp0 + nb * kCh, pn, lane) & kDevelope;
            computed = true;
        }
        int pf = pitch[frame], bf = buf[frame];
        if (pitch_crn(bf, bn)) {
            pf = bf;
        } else {
            unset = unset || !computed;
            const float g = grp0[frame * kCh + lane];
            const ChanSet own = __ballot(left ? g > 0.0f : g != 0.0f); /* :986 / :1064: all 64 channels */
            const ChanSet mark2 = own & chan_mark;
            const int number = popc64(mark2);
            if (number) {
                float k1 = (float)(0.65 * (double)(float)(bn + 1) - 1);
                if (k1 < (float)kMinDel) k1 = (float)kMinDel;
                float k2 = (float)(1.55 * (double)(float)(bn + 1) - 1);
                if (k2 > (float)(kDel - 1)) k2 = (float)(kDel - 1);
                const float *acf = acf0 + (long long)frame * kRow;
                pf = sum_auto(acf, mark2, (int)k1, (int)k2, lane);
                bool keep = false;
                if (pitch_crn(pf, bn)) {
                    /* :1009 / :1087: `for(chan=0; chan<40; chan++)` */
                    const int number2 = popc64(ratio_mask(acf, mraw0 + frame * kCh, grp0 + frame * kCh, pf, lane) & kDevelope);
                    keep = number2 * 2 > number;
                }
                if (keep) {
                    bf = pf;
                } else {
                    pf = 0;
                    bf = bn;
                }
            } else {
                bf = bn;
            }
        }
        if (lane == 0) {
            pitch[frame] = pf;
            buf[frame] = bf;
        }
        pn = pf;
        bn = bf;
    }
    return unset;
}

} // namespace

__global__ __launch_bounds__(64) void hw64_pitch_track_kernel(Hw64PitchArgs a)
{
    const int lane = threadIdx.x;
    const Utt t = utterance(a);
    if (inactive(a.status[t.u])) return;
    const int F = t.nfr;
    int *pitch = a.pitch + t.row0, *buf = t.buf;
    /* findPitch's lFrame / rFrame: the first and the last frame where sumAuto found a delay, whether or not the vote then
     * zeroed Pitch (buf holds sumAuto's result of the last findPitch); F and 0 when there is none */
    int lF = F, rF = 0;
    for (int f = lane; f < F; f += 64) {
        const int p = pitch[f], found = buf[f];
        buf[f] = p;
        pitch[f] = 0;
        if (found > 0) {
            lF = f < lF ? f : lF;
            rF = f > rF ? f : rF;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int l = __shfl_xor(lF, off), r = __shfl_xor(rF, off);
        lF = l < lF ? l : lF;
        rF = r > rF ? r : rF;
    }
    lanes_fence();
    /* ---- checkPitch:901-952, sStreak = 0 and eStreak = 1 to start with as the reference has them ---- */
    int sStreak = 0, eStreak = 1, sFrame = lF, eFrame = lF;
    auto close_streak = [&]() {
        if (eFrame - sFrame > eStreak - sStreak) {
            sStreak = sFrame;
            eStreak = eFrame;
        }
        if (eFrame - sFrame + 1 > 2)
            for (int f = sFrame + lane; f <= eFrame; f += 64) pitch[f] = buf[f];
    };
    if (lF < rF) {
        int prev = buf[lF];
        for (int f0 = lF + 1; f0 <= rF; f0 += 64) {
            const int mine = f0 + lane <= rF ? buf[f0 + lane] : 0;
            const int n = rF - f0 + 1 < 64 ? rF - f0 + 1 : 64;
            for (int j = 0; j < n; ++j) {
                const int cur = __shfl(mine, j);
                if (pitch_crn(prev, cur)) {
                    eFrame = f0 + j;
                } else {
                    close_streak();
                    sFrame = eFrame = f0 + j;
                }
                prev = cur;
            }
        }
    }
    close_streak();
    lanes_fence();
    if (a.stages)
        for (int f = lane; f < F; f += 64) stage_pitch(a, t, 2)[f] = pitch[f];
    /* ---- leftDevelope, rightDevelope ---- */
    bool unset = develope(a, t, sStreak - 1, lF, -1, lane);
    lanes_fence();
    if (a.stages)
        for (int f = lane; f < F; f += 64) stage_pitch(a, t, 3)[f] = pitch[f];
    unset = develope(a, t, eStreak + 1, rF, +1, lane) || unset;
    lanes_fence();
    if (a.stages)
        for (int f = lane; f < F; f += 64) stage_pitch(a, t, 4)[f] = pitch[f];
    /* ---- linearEstimate:1110-1142: `else if (sd)` as it stands, so frame 0 never starts an interpolation.  The frames it
     * fills lie behind the frame being read ---- */
    int judge = 0, sd = 0, psd = 0;
    for (int f0 = 0; f0 <= rF; f0 += 64) {
        const int mine = f0 + lane <= rF ? pitch[f0 + lane] : 0;
        const int n = rF - f0 + 1 < 64 ? rF - f0 + 1 : 64;
        for (int j = 0; j < n; ++j) {
            const int p = __shfl(mine, j), frame = f0 + j;
            if (p) {
                if (judge) {
                    const float k = (float)(p - psd) / (float)(frame - sd);
                    for (int tf = sd + 1 + lane; tf < frame; tf += 64) {
                        const float pd = (float)psd + k * (float)(tf - sd);
                        int q = (int)pd;
                        if ((pd - (float)q) >= 0.5f) q++;
                        pitch[tf] = q;
                    }
                    judge = 0;
                }
                sd = frame;
                psd = p;
            } else if (sd) {
                judge = 1;
            }
        }
    }
    if (unset && lane == 0) a.status[t.u] |= SEA_HW25_CHANMARK_UNSET;
}

} // namespace sea
