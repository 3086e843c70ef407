/*
 * ns6_beat_plan.h -- which beats of a six-wave NoiseSup role need no frame bookkeeping (ns_pipe6_kernel.hip).
 *
 * Every role of the six-wave form runs niter = nfr + kDepth beats (nfr + depth_of(variant): the variant with kIdctS is deeper); at beat i it handles a few frames i - d, and what it does with
 * each hangs on one flag, "frame i - d exists and has tick >= k":
 *
 *      flag(i; d, k)  =  i - d < nfr  &&  i - d - (k - 1) >= onset          (tick_ge of the kernel; onset = first non-zero frame)
 *
 * which is true exactly for  onset + d + k - 1 <= i < nfr + d.  The flags of a role are therefore ALL true on one interval of beats,
 * from the largest lower end to the smallest upper end: the role's steady range.  Inside it the kernel runs a copy of the role's beat
 * in which every flag is the literal `true`; before and after it the general copy, which evaluates them.  This header holds the table
 * of (d, k) per role and the two ends of the range; the kernel's flags are checked against the table at compile time (beat_flag
 * there), tests/test_ns6_beat_plan_cpu.py sweeps the ends on the host.
 *
 * Plain C++: no HIP types, includable from a host program.
 */
#ifndef SEA_NS6_BEAT_PLAN_H
#define SEA_NS6_BEAT_PLAN_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SEA_NS6_HD __host__ __device__
#else
#define SEA_NS6_HD
#endif

namespace sea {
namespace ns6plan {

constexpr int kNoOnset = 0x7fffffff; /* the gate never opened (or: not yet seen) */
constexpr int kDepth = 9;            /* a role runs nfr + kDepth beats; S stores frame i - kDepth */

enum Role { FA = 0, FB = 1, B0 = 2, N1 = 3, G1 = 4, S = 5, kRoles = 6 };

/* the compile-time variants of the body: a flag of the table belongs to all of them (kAlways) or to those with one of these */
constexpr unsigned kAlways = 0u, kFd = 1u, kLight = 2u, kDifg1 = 4u;
/* kRedeal (round 8, the dense kernel): feed-forward work dealt to the waves that wait -- N1 takes the VAD log-energy of frame i-2 off S,
 * FA runs the stage-0 17-tap filter of frame i-3 (off B0) in the beat in which it windows that frame's stage-1 input */
constexpr unsigned kRedeal = 8u;
/* the three kernels; kVariantDense is the dense body without the re-deal, which no kernel takes since round 8 */
constexpr unsigned kVariantPlain = kLight | kDifg1, kVariantDense = 0u, kVariantFd = kFd | kLight | kDifg1;
constexpr unsigned kVariantDenseRedeal = kRedeal;
/* kBin64 (round 10, the dense kernel): the stage-1 Wiener gain of bin 64 rides in B0's stage-0 filter pass -- lane 1 of the component
 * that carries bin 64 takes stage-1 frame i-6 (N1 left its mean PSD and noise at i-5), G1 computes bins 0..63 only.  The dense kernel is
 * kVariantDenseBin64; kVariantDenseRedeal is the body it grew from, which no kernel takes any more */
constexpr unsigned kBin64 = 16u;
constexpr unsigned kVariantDenseBin64 = kRedeal | kBin64;
/* kIdctS (round 11, the dense kernel): the two in-order IDCT sums (DoMelIDCT, nine rows of 25 terms per stage) ride in idle lanes of the
 * helper wave's stream.  B0 and G1 leave the 9 x 25 rounded products, S adds them up one beat later, and the 17-tap filters follow one
 * beat after that: FA filters stage-0 frame i-4 (was i-3), so every stage-1 job moves by one beat, and G1 filters frame i-11 in the
 * beat in which it takes the gains of frame i-9.  The variant has a table of its own (kPlanIdct) and a depth of its own (depth_of);
 * the dense kernel is kVariantDenseIdct, kVariantDenseBin64 is the body it grew from, which no kernel takes any more */
constexpr unsigned kIdctS = 32u;
constexpr unsigned kVariantDenseIdct = kRedeal | kBin64 | kIdctS;
constexpr int kDepthIdct = 12;       /* a role of that variant runs nfr + 12 beats; S stores frame i - 12 */
/* kFirPair (round 14, the dense kernel): both 17-tap filters run as ONE pass on the two lane halves of G1 -- stage-0 frame i-4 (off FA)
 * and stage-1 frame i-12, whose taps S leaves at the same beat i-1.  The filtered stage-0 frame crosses a frame barrier before FA windows
 * it (FA: stage 1 of frame i-5, was i-4), so every stage-1 job moves by one more beat.  The variant has a table of its own
 * (kPlanFirPair) and a depth of its own; the dense kernel is kVariantDenseFirPair, kVariantDenseIdct is the body it grew from, which no
 * kernel takes any more */
constexpr unsigned kFirPair = 64u;
constexpr unsigned kVariantDenseFirPair = kRedeal | kBin64 | kIdctS | kFirPair;
constexpr int kDepthFirPair = 13;    /* a role of that variant runs nfr + 13 beats; S stores frame i - 13 */

struct Flag {
    int d;         /* the flag is about frame i - d ... */
    int k;         /* ... having tick >= k */
    unsigned when; /* kAlways, or the variant bit that adds it */
};
constexpr int kMaxFlags = 5;
struct RolePlan {
    int n;
    Flag f[kMaxFlags];
    int ahead;  /* frames BEYOND frame i that a steady beat touches: FA prefetches frame i + 1, so i + 1 < nfr must hold */
    int settle; /* beats the general copy must have run with all flags true before the steady copy may take over: S notes the
                 * index of its first output frame (firstOut) at the first beat whose `produced` is true, the steady copy does not */
};

constexpr RolePlan kPlan[kRoles] = {
    /* FA: frame i itself enters stage 0 from tick 3; stage 1 of frame i-3 from tick 5; LIGHT: the VAD log-energy of frame i-2;
     * kRedeal: the stage-0 filter of frame i-3, from tick 3 (ticks 3 and 4 leave output that the first stage-1 window needs) */
    {4, {{0, 3, kAlways}, {3, 5, kAlways}, {2, 1, kLight}, {3, 3, kRedeal}, {0, 0, 0}}, 1, 0},
    /* FB: one beat behind FA on both transforms */
    {2, {{1, 3, kAlways}, {4, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* B0: stage-0 back half of frame i-2; kBin64: stage-1 bin 64 of frame i-6 */
    {2, {{2, 3, kAlways}, {6, 5, kBin64}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* N1: noise tracking of frame i-5, gain-factor scalars of frame i-7; kRedeal: the VAD log-energy of frame i-2 */
    {3, {{5, 5, kAlways}, {7, 5, kAlways}, {2, 1, kRedeal}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* G1: gains of frame i-8 */
    {1, {{8, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* S: VAD sum of frame i-1, denSigSE1 sum of i-3, noise sum of i-6, output of i-9; FD: the speech flags of frame i-9 */
    {5, {{1, 1, kAlways}, {3, 3, kAlways}, {6, 5, kAlways}, {kDepth, 5, kAlways}, {kDepth, 5, kFd}}, 0, 1},
};

/* the table of the variants with kIdctS: every flag belongs to the one kernel that takes it */
constexpr RolePlan kPlanIdct[kRoles] = {
    /* FA: frame i itself enters stage 0 from tick 3; the stage-0 filter of frame i-4 from tick 3, from the sums S left at i-1; stage 1
     * of frame i-4 from tick 5 */
    {3, {{0, 3, kAlways}, {4, 5, kAlways}, {4, 3, kAlways}, {0, 0, 0}, {0, 0, 0}}, 1, 0},
    /* FB: one beat behind FA on both transforms */
    {2, {{1, 3, kAlways}, {5, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* B0: stage-0 back half of frame i-2 (up to the IDCT products); stage-1 bin 64 of frame i-7 */
    {2, {{2, 3, kAlways}, {7, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* N1: the VAD log-energy of frame i-2, noise tracking of frame i-6, gain-factor scalars of frame i-8 */
    {3, {{2, 1, kAlways}, {6, 5, kAlways}, {8, 5, kAlways}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* G1: gains, mel and IDCT products of frame i-9; Hanning weight and 17-tap filter of frame i-11, from the sums S left at i-1 */
    {2, {{9, 5, kAlways}, {11, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* S: VAD sum of frame i-1, denSigSE1 sum and stage-0 IDCT sums of i-3, noise sum of i-7, stage-1 IDCT sums of i-10, output of i-12 */
    {5, {{1, 1, kAlways}, {3, 3, kAlways}, {7, 5, kAlways}, {10, 5, kAlways}, {kDepthIdct, 5, kAlways}}, 0, 1},
};
/* the table of the variants with kFirPair, likewise.  Derivation, from the stage-0 chain (FA i, FB i-1, B0 i-2, S i-3, whose offsets do
 * not move): S leaves the stage-0 taps of frame f at f+3, G1 filters at f+4 (from tick 3: ticks 3 and 4 leave output that the first
 * stage-1 window reads), FA windows the stage-1 input at f+5, FB f+6, N1 tracks at f+7, S sums the noise and B0 takes bin 64 at f+8, N1's
 * gain-factor scalars at f+9, G1's gains and products at f+10, S's stage-1 sums at f+11, G1 filters at f+12, S stores at f+13 */
constexpr RolePlan kPlanFirPair[kRoles] = {
    /* FA: frame i itself enters stage 0 from tick 3; stage 1 of frame i-5 from tick 5 */
    {2, {{0, 3, kAlways}, {5, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 1, 0},
    /* FB: one beat behind FA on both transforms */
    {2, {{1, 3, kAlways}, {6, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* B0: stage-0 back half of frame i-2 (up to the IDCT products); stage-1 bin 64 of frame i-8 */
    {2, {{2, 3, kAlways}, {8, 5, kAlways}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* N1: the VAD log-energy of frame i-2, noise tracking of frame i-7, gain-factor scalars of frame i-9 */
    {3, {{2, 1, kAlways}, {7, 5, kAlways}, {9, 5, kAlways}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* G1: the merged filter pass over stage-0 frame i-4 and stage-1 frame i-12; gains, mel and IDCT products of frame i-10 */
    {3, {{4, 3, kAlways}, {10, 5, kAlways}, {12, 5, kAlways}, {0, 0, 0}, {0, 0, 0}}, 0, 0},
    /* S: VAD sum of frame i-1, denSigSE1 sum and stage-0 IDCT sums of i-3, noise sum of i-8, stage-1 IDCT sums of i-11, output of i-13 */
    {5, {{1, 1, kAlways}, {3, 3, kAlways}, {8, 5, kAlways}, {11, 5, kAlways}, {kDepthFirPair, 5, kAlways}}, 0, 1},
};
SEA_NS6_HD constexpr const RolePlan &plan_of(unsigned variant, int role)
{
    return (variant & kFirPair) ? kPlanFirPair[role] : ((variant & kIdctS) ? kPlanIdct[role] : kPlan[role]);
}
/* beats a role runs past the last frame; S stores frame i - depth_of */
SEA_NS6_HD constexpr int depth_of(unsigned variant) { return (variant & kFirPair) ? kDepthFirPair : ((variant & kIdctS) ? kDepthIdct : kDepth); }

SEA_NS6_HD constexpr bool flag_applies(const Flag &f, unsigned variant) { return f.when == kAlways || (f.when & variant) != 0u; }

/* (d, k) is a flag of the role in that variant: what the kernel asserts of every flag it evaluates */
SEA_NS6_HD constexpr bool has_flag(unsigned variant, int role, int d, int k)
{
    const RolePlan &p = plan_of(variant, role);
    for (int j = 0; j < p.n; ++j)
        if (p.f[j].d == d && p.f[j].k == k && flag_applies(p.f[j], variant)) return true;
    return false;
}

/* beats after the onset from which all flags hold: max over the flags of d + k - 1, plus the settle beats */
SEA_NS6_HD constexpr int steady_lead(unsigned variant, int role)
{
    const RolePlan &p = plan_of(variant, role);
    int lead = 0;
    for (int j = 0; j < p.n; ++j) {
        const Flag &f = p.f[j];
        if (flag_applies(f, variant) && f.d + f.k - 1 > lead) lead = f.d + f.k - 1;
    }
    return lead + p.settle;
}
/* beats past nfr at which the first flag falls: min over the flags of d, less the frames a steady beat touches ahead (may be < 0) */
SEA_NS6_HD constexpr int steady_tail(unsigned variant, int role)
{
    const RolePlan &p = plan_of(variant, role);
    int tail = depth_of(variant);
    for (int j = 0; j < p.n; ++j) {
        const Flag &f = p.f[j];
        if (flag_applies(f, variant) && f.d < tail) tail = f.d;
    }
    return tail - p.ahead;
}

/* first beat at which every flag of the role is true; kNoOnset while there is no onset (no beat is >= it: frame counts stay below) */
SEA_NS6_HD constexpr int steady_begin(unsigned variant, int role, int onset)
{
    return onset == kNoOnset ? kNoOnset : onset + steady_lead(variant, role);
}
/* first beat from steady_begin on at which one of them is false again (never above nfr + depth_of(variant) - 1; the range is empty when this
 * is not above steady_begin) */
SEA_NS6_HD constexpr int steady_end(unsigned variant, int role, int nfr)
{
    const int e = nfr + steady_tail(variant, role);
    return e > 0 ? e : 0;
}

} // namespace ns6plan
} // namespace sea

#undef SEA_NS6_HD
#endif
