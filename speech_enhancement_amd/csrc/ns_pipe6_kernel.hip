/*
 * ns_pipe6_kernel.hip -- etsi_denoise over a packed batch, SIX pipelined wavefronts per utterance.
 *
 * Same arithmetic as ns_pipe_kernel.hip (four waves), cut finer.  With up to four utterances per CU the
 * run time of a launch is the longest utterance's chain of frames, i.e. (number of frames) x (frame
 * period of one workgroup), and the frame period is the longest role.  The role timers of the
 * four-wave kernel (tools/ns_timing.py) read F 4670, B0 3590, B1 4690, S 4310 clk; here the dual
 * transform is cut at its middle level and the second-stage back half into noise tracking | gains:
 *
 *   wave FA  iteration i: load int16 frame i, zero-frame gate, push; window + register-resident start
 *            + levels n2 = 8, 16, 32 of BOTH transforms (stage 0 of frame i, stage 1 of frame i-3)
 *   wave FB  i+1 / i+4:   levels n2 = 64, 128, 256 and the two 65-bin PSDs
 *   wave B0  frame i-2:   stage-0 FilterCalc, VAD, mel, IDCT, FIR -> stage-1 buffer
 *   wave N1  frame i-5:   stage-1 PSD mean, noise tracking -> P, noise
 *            frame i-7:   gain-factor scalars from S's noise sum and the denSigSE1 sums -> alfa
 *   wave G1  frame i-8:   stage-1 Wiener gains, mel, gain factorisation, IDCT, FIR
 *   wave S   the lane-grouped scalar chains: VAD log-energy of the frame pushed at i-1, in-order sum of
 *            denSigSE1 of frame i-3, in-order sum of the noise spectrum of frame i-6, DC-offset recurrence
 *            + cast + store of frame i-9 (kDepth)
 * (the dense kernel's schedule since round 11 is three beats deeper, since round 14 four: the Round 11 and Round 14 paragraphs below)
 *
 * Round 6: the in-order sum of the 65 second-stage noise magnitudes (64 v_readlane + v_add in N1, ~129 vector instructions
 * for one scalar) rides the helper wave's serial stream in lanes 48..63, which only repeated the DC chain: no instruction
 * more there.  N1's frame is thereby cut in two jobs two beats apart, and G1 and S's output follow two beats later than
 * before; the lifetimes and ring depths are derived beside kP1Ring below.  configs[1]: 1.84 -> 1.76 ms = 465 M frames/s
 * (profiles/ns6_noise_sum_in_helper.txt).
 *
 * Round 7: every role's beat exists in a general copy, which derives the frame's flags, and a steady copy without them for the beats on
 * which all are true (run_beats below, ns6_beat_plan.h); the dense and the _fd kernel take it, the plain kernel lost with it and stays on
 * the general copy (template parameter STEADY_LOOP).  configs[1]: 1.76 -> 1.71 ms = 479 M frames/s, 489 -> 356 scalar instructions per
 * frame (profiles/ns6_steady_loop.txt).
 *
 * Round 8, the dense kernel only (REDEAL of ns_pipe6_body): two pieces of feed-forward work leave the two longest roles for waves that
 * waited at the barrier, the instruction stream and the results unchanged --
 *   wave N1  also: the VAD log-energy of the frame pushed at i-2, from the sum S left in frameEn one beat before -> frameEnLog (read by B0)
 *   wave B0  stops at the nine IDCT sums of frame i-2 -> tap[]
 *   wave FA  also: Hanning weight and the 17-tap filter of frame i-3 over the stage-0 buffer -> stage-1 buffer, before it windows that frame
 *   wave S   leaves 64 + the frame's sum of squares, not its logarithm
 * and that kernel has a wave -> role map of its own (kRedealPerm).  The plain and the _fd kernel run what is described above.
 * configs[1]: 1.71 -> 1.66 ms (profiles/ns6_redeal.txt).
 *
 * Round 9, all three kernels, scheduling only: what S, G1 and B0 waited for in turn is fetched as batches of LDS reads --
 *   wave S   the prep of its chains (squares of the frame, differences of G1's output) from ONE batch in lanes 0..39, where four
 *            round trips over 64 + 16 lanes were
 *   wave B0  the 25 IDCT basis values ahead of the lane reads of the mel gains, then the unchanged in-order sum (ns_core.h,
 *            ns_idct_basis_request); G1 of the plain and the _fd kernel likewise
 *   wave G1  of the dense kernel: the same in two batches, 13 + 12 (one of 25 spills a register there); the mean PSD with its first reads
 * S 2935 -> 2700, G1 2920 -> 2720, B0 2640 -> 2365 clk per frame.  256 utterances 1.541 -> 1.412 ms, 768 1.609 -> 1.544, the _fd
 * kernel on 512 2.669 -> 2.433 (B0 sets those kernels' period); configs[1] 1.66 -> 1.64 ms, the same 0.020 ms in three alternations,
 * which is over three times the spread in one of them only (profiles/ns6_lds_batches.txt).
 *
 * Round 10, the dense kernel only (BIN64 of ns_pipe6_body): the Wiener-gain chain ran on the pair (bin lane, bin 64) in B0 and in G1, and
 * the second component is one useful value in 64 identical lanes --
 *   wave B0  also: stage-1 bin 64 of frame i-6 in lane 1 of that second component (PSD, mean PSD and updated noise from FB's and N1's
 *            records, the recursive den in a register of its own) -> w1hi (read by G1 two beats later)
 *   wave G1  bins 0..63 through the single-component chain, W[64] from w1hi
 *   wave N1  also: its fast-division decision of the frame -> rn[].P[65]; G1 and B0 read it instead of testing the PSD again
 * and the wave -> role map was swept again (kRedealPerm).  G1 2720 -> 2120 clk per frame, B0 2365 -> 2575, the beat 3065 -> 2975;
 * the step moved with the new map, not before it: the figures are in profiles/ns6_bin64_in_b0.txt.
 *
 * Round 11, the dense kernel only (IDCTS of ns_pipe6_body): DoMelIDCT's nine in-order sums of 25 terms cost B0 and G1, for nine useful
 * lanes each, 25 lane reads, 25 basis reads, 25 multiplications and a chain of 25 dependent additions per frame.  Now --
 *   wave B0  frame i-2 as before, up to the 9 x 25 rounded products of the mel gains and the basis (lane = (row, quad): four
 *            multiplications and one 128-bit store) -> prod[0]
 *   wave G1  frame i-9: gains, mel, gain factorisation, the same products -> prod[1]; frame i-11: the 17-tap filter from S's taps
 *   wave S   also: the nine rows of stage-0 frame i-3 in lanes 1..9 and of stage-1 frame i-10 in lanes 17..25 of its serial stream
 *            (they only repeated the VAD and the den chain), `acc = fma(1, acc, x)` from +0, which is the reference's
 *            h += W * idct term by term; then the Hanning weight, one multiplication -> tap[]; noise sum of i-7, output of i-12
 *   wave FA  the stage-0 filter of frame i-4 from S's taps, and with it every stage-1 job one beat later: FB i-5, N1 i-6 / i-8, B0's
 *            guest i-7
 * The pipeline is twelve beats deep instead of nine (ns6plan::depth_of), the stream keeps its length (110 instructions between the
 * 80 FMAs of the listing, 113 before: the three bases are set before it), and the map was swept again (kRedealPerm).  configs[1]:
 * 1.61 -> 1.47 ms = 555 M frames/s (profiles/ns6_idct_in_helper.txt).
 *
 * Round 12, all three kernels (PAIRED of ns_pipe6_body, run_beats): the steady beats run two by two, an even beat and the odd one
 * after it, so the frame parity is a constant of each copy.  Every record that is double-buffered by parity gets its address as an
 * instruction offset, and FB (FA but for its register-resident start) keeps the transform's operand addresses unpacked in registers: the
 * eight `base + packed half-word` additions in front of every level's LDS reads are gone.  Same operations, same order.  Dense kernel:
 * 1169 -> 1088 vector and 349 -> 314 scalar instructions per frame, configs[1] 1.49 -> 1.41 ms (1.456 -> 1.377 over 200 steps) =
 * 594 M frames/s; the plain kernel takes the steady copies with it.  What that issue set out to do -- FA and FB on the latency form of
 * the transform (the four-wave F wave's since round 3) and N1's two logarithms in one lane-split pass -- was built, measured and
 * dropped: FB's role 2490 -> 2350 clk but the step 1.479 -> 1.501 ms, FA 1.479 -> 1.496, both 1.479 -> 1.520, the logarithm pair
 * 1.479 -> 1.486 with N1 2440 -> 2585 clk, none better under its own best wave -> role map; the step follows the instruction count, not
 * the longest role: all four launch rows end together (profiles/ns6_transform_chain.txt).
 *
 * Round 13, all three kernels: address and operand set-up off the steady beats of the two transform waves, no operation, beat, barrier, ring
 * slot or LDS instruction added --
 *   wave FA  the steady copies take the onset and their pair counter through v_readfirstlane at the switch into the range (FA writes its
 *            onset under the gate's ballot and the compiler took it, and everything derived from it, for lane-dependent): ticks, ring
 *            slots and window bases are scalar, the next frame's address is an SGPR pair counted on by one frame per beat and its load
 *            sits under the store's lane branch
 *   FA, FB   the twiddled butterfly's four output additions read the halves of their operand pairs through op_sel / neg_lo / neg_hi
 *            (sea_device.h, fft2_bf_out) instead of operands built with a packed negation, an exclusive-or and three moves
 *   wave FB  the PSD's neighbour fetches need no zero in their destination (bound_ctrl) and repair the two wrap lanes with v_writelane
 *            (ns_core.h, psd_from_last_level)
 *   all      the test "is this a beat on which the priority is set" is one scalar compare and branch (prio_by_remaining; not the _fd kernel)
 * Dense kernel: FA 251.5 -> 217.5, FB 150.5 -> 130.5 vector instructions per beat on the listing; counted, 1088 -> 1036 vector, 314 -> 322
 * scalar and 205 -> 204 LDS instructions per frame; configs[1] 1.365-1.370 -> 1.332-1.336 ms over 200 steps, 2.5 % and over five times the
 * spread in two alternations of the final code (profiles/ns6_offstream.txt).
 *
 * Round 14, the dense kernel only (FIRP of ns_pipe6_body): the time-domain filter ApplyWF ran twice per frame in two waves, each time 80
 * outputs as 40 lanes x 2, 68 multiplications and additions on 40 of 64 lanes with its own taps and samples; both become ready at the same
 * beat, S leaves both stages' taps at i-1.  Now --
 *   wave G1  also: ONE pass on its two lane halves (ns_core.h, ns_fir_pair3), lane 32 h + j computing outputs 3j .. 3j + 2 of stage h from
 *            per-lane taps: stage-0 frame i-4 -> the stage-1 buffer, stage-1 frame i-12 -> ro[]; 102 multiplications and additions for both
 *            where 136 were, one set of reads, no mirrored taps; then the gains of frame i-10
 *   wave FA  filters no more; it windows stage-1 frame i-5, which G1 left one beat before, behind a frame barrier
 *   all      every stage-1 job one more beat later: FB i-6, N1 i-7 / i-9, B0's guest i-8, S's noise sum i-8, stage-1 sums i-11, output i-13
 * The pipeline is thirteen beats deep (ns6plan::depth_of), S's ring of den sums sixteen (kDenRing16), and the map was swept again
 * (kRedealPerm).  Every output is the same in-order 17-term sum of the same rounded products.  Listing, steady beats: FA 81 vector and 8
 * LDS instructions fewer per frame, G1 34 and 5 more; configs[1] over 200 steps 1.344 -> 1.295 ms with the parent's map (8 x the larger spread), 1.334 ->
 * 1.267 ms = 646 M frames/s with the swept one (-5.0 %, 7 x; profiles/ns6_fir_merged.txt).
 *
 * Round 15, the dense kernel only (LOGP of ns_pipe6_body): N1's VAD logarithm was a full wave64 instruction stream, most of it double
 * precision, for one wave-uniform value per beat.  Its argument is feed-forward (S's sum of squares) and its result is read two beats
 * later, so there is a spare beat: in a steady pair of beats (2h, 2h+1) --
 *   wave N1  nothing for the VAD in the even beat; in the odd beat the sums of both beats in its even and odd lanes through ONE pass
 *            (ns_core.h, ns_log_lanes_request / ns_log_lanes_take: per lane the operations of ns_vad_energy_expr<false>, the guard of
 *            all lanes under one ballot), the table rows by per-lane loads requested at the top of the beat and taken behind the
 *            noise tracking -> both slots of frameEnLog, one barrier ahead of B0's read of the first
 * The general copy keeps one logarithm per beat; no flag, ring, beat or barrier changed.  N1's steady pair on the listing: 928 -> 888
 * vector (349 -> 316 of them f64), 331 -> 278 scalar instructions; configs[1] over 200 steps 1.278 -> 1.243 ms = 658 M frames/s (-2.7 %,
 * 7 x the larger spread; profiles/ns6_log_pairs.txt, which also says what of that issue was not built: the averSNR pair and the
 * fourteen-beat schedule it needs).
 *
 * All records between neighbouring stages are double-buffered by frame parity (written at one
 * iteration, read at the next), those that are read in place over several beats sit in rings (kP1Ring, kRnRing); the two
 * transform work areas alternate between FA and FB.  The records carry data only: which frames are valid, their ticks
 * and whether they produce output follow from ONE number per utterance, the index of its first non-zero frame, which
 * FA publishes once (kNoOnset / onset_poll below).
 *
 * Round 4: this is the form for up to FOUR utterances per CU, configs[1] included (capi.hip::ns_pick_form).  Up to three per CU
 * ns_denoise_pipe6_kernel (bound of 80 VGPRs, the lighter helper wave: LIGHT / DIFG1 of ns_pipe6_body); for the fourth ns_denoise_pipe6_dense_kernel, the same
 * body compiled for seven waves per SIMD -- with six, the dispatcher never found room for the fourth six-wave workgroup of a CU, which is
 * what rounds 1-3 measured as "the six-wave form loses at four per CU" (see the comment at the kernels below).  With more than one
 * utterance per CU the waves set their issue priority by the frames their utterance has left (prio_by_remaining, the rule of
 * ns_pipe_kernel.hip), and the wave -> role map (kDefaultPerm) puts B0 and S on the two oldest waves: among equal priorities a SIMD
 * issues its oldest wave first.  configs[1]: 1.91-1.95 ms = 420-427 M frames/s (four-wave form 2.08-2.13);
 * profiles/r04_ns_six_wave_dense.txt.  With the bookkeeping taken off the per-frame stream: 1.85 ms = 442 M frames/s
 * (profiles/r05_ns6_bookkeeping.txt).
 */
#include "ns_core.h"
#include "ns6_beat_plan.h"

namespace sea {

namespace p6 { /* everything of the six-wave form */

/* timing-only diagnostic (-DSEA_NS6_TIMING): shader clocks workgroup 0's six roles spend working / waiting at the frame barrier
 * -> g_ns6_timing[role * 2 + {0, 1}], [12] = frames; read through sea_debug_ns6_timing (tools/ns6_roles.py) */
#ifdef SEA_NS6_TIMING
__device__ unsigned long long g_ns6_timing[16];
struct RoleTimer6 {
    unsigned long long work = 0, wait = 0, t0 = 0, t1 = 0;
    __device__ __forceinline__ void begin() { t0 = clock64(); }
    __device__ __forceinline__ void mid() { t1 = clock64(); work += t1 - t0; }
    __device__ __forceinline__ void end() { wait += clock64() - t1; }
};
#define NS6_T_DECL RoleTimer6 rt_
#define NS6_T_BEGIN rt_.begin()
#define NS6_T_MID rt_.mid()
#define NS6_T_END rt_.end()
#define NS6_T_FLUSH(r, n) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) { g_ns6_timing[2 * (r)] = rt_.work; g_ns6_timing[2 * (r) + 1] = rt_.wait; g_ns6_timing[12] = (unsigned long long)(n); } } while (0)
#else
#define NS6_T_DECL
#define NS6_T_BEGIN
#define NS6_T_MID
#define NS6_T_END
#define NS6_T_FLUSH(r, n)
#endif

constexpr int kSlots = 8;   /* stage-0 buffer, and the per-tick rings frameEn, frameEnLog, denSum, fdFlags */
constexpr int kSlots1 = 16; /* stage-1 buffer (derivation at kP1Ring) */
constexpr int kSlotLen = SEA_HOP;
constexpr int kCirc = kSlots * kSlotLen;
constexpr int kCirc1 = kSlots1 * kSlotLen;
constexpr int kMirror = 3 * kSlotLen;
constexpr int kWaves = 6;
constexpr int kDepth = ns6plan::kDepth; /* 9: S stores frame i - kDepth (IDCTS: ns6plan::depth_of, 12) */
constexpr int kSChunks = 10; /* helper_chains: the helper wave's 20 quads are requested in ten chunks (2 x 8 VGPRs in flight) */
/* issue priority by remaining frames: evaluated every kPrioStep frames, kPrioLevels levels dithered into the four hardware ones
 * (the rule and its measurements: ns_pipe_kernel.hip) */
constexpr int kPrioStep = 16;
constexpr int kPrioLevels = 32;
/* wave -> role (octal digits, wave 0 rightmost; roles 0 FA, 1 FB, 2 B0, 3 N1, 4 G1, 5 S): B0 and S on the two oldest waves.
 * NsBatchArgs::perm6 != 0 replaces it (sea_debug_ns6_perm, which accepts permutations of 0..5 only). */
constexpr int kDefaultPerm = 0014352;
/* The re-dealt dense kernel: a map of its own, re-swept whenever the roles' lengths move (tools/ns6_perm_sweep.py, all 720 maps).
 * Round 8: 0053412 (B0, FB, G1, N1, S, FA on waves 0..5).  Round 10, with G1 the shortest role instead of the longest: FA, N1, B0, G1, S,
 * FB on waves 0..5 -- the best ten maps of that sweep all keep G1 on wave 3 and B0 or N1 on wave 2; 0053412 is 76th there, 2.8 %
 * behind (profiles/ns6_bin64_in_b0.txt).  Round 11, with the IDCT sums in S: S, B0, N1, FA, G1, FB on waves 0..5 -- six of the best
 * ten maps of that sweep keep N1 on wave 2 and G1 on wave 4, seven have S on wave 0 or 1; 0154230 is 122nd there, 3.9 % behind
 * (profiles/ns6_idct_in_helper.txt).  Round 14, with both filters in G1 and FA the lighter for it: S, B0, N1, G1, FA, FB on waves 0..5
 * -- G1 and FA change places; eight of the best ten maps of that sweep keep G1 on wave 3, seven N1 on wave 2, all ten S on wave 0 or 1; 0140325 is 18th there,
 * 1.2 % behind (profiles/ns6_fir_merged.txt) */
constexpr int kRedealPerm = 0104325;

/* Frame bookkeeping (valid / tick / produced of every frame) is a pure function of the frame index: the zero-frame gate
 * (ParmInterface.c:244-251) has one degree of freedom per utterance, the index `onset` of the first non-zero frame.  From it on every
 * frame f < nfr is valid with tick(f) = f - onset + 1, stage 0 runs from tick 3 (NoiseSup.c:1152) and stage 1 / the output from tick 5
 * (NoiseSup.c:1178).  So the records between the roles carry data only; FA publishes the onset ONCE (Pipe6Lds::onset) and every role
 * derives the flags of the frame it handles with scalar arithmetic on (f, onset, nfr).
 *
 * A reader keeps the onset in an SGPR.  While that is still kNoOnset it reads the LDS word once per beat (onset_poll); from the beat
 * it sees a value on it never reads it again.  Why "not yet" may be taken for "invalid": a role at iteration i only handles frames
 * f < i.  FA decides frame g at its own iteration g and writes the word there, before the barrier that ends iteration g; a reader at
 * iteration i has passed the barriers of iterations 0 .. i-1, so it sees FA's write of every iteration g <= i-1.  Reading kNoOnset at
 * beat i therefore means onset >= i > f: the frame is before the onset, i.e. invalid -- exactly what f >= onset gives with
 * kNoOnset = INT_MAX.  (FA's write of iteration i itself may or may not be seen; both readings give the same flags for f < i.) */
constexpr int kNoOnset = ns6plan::kNoOnset; /* 0x7fffffff */
constexpr long long kMaxFrames = 0x7fffffffLL - 16; /* frame indices, iteration counts and ticks stay below kNoOnset */
__device__ __forceinline__ void onset_poll(int &onset, const int *word)
{
    if (onset == kNoOnset)
        onset = __builtin_amdgcn_readfirstlane(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
/* tick of frame f (meaningful for f >= onset; unsigned so that kNoOnset wraps instead of overflowing -- callers only mask such a value) */
__device__ __forceinline__ int tick_of(int f, int onset) { return (int)((unsigned)f - (unsigned)onset + 1u); }
/* frame f exists and has tick >= k (k >= 1; f may be negative: onset >= 0) */
__device__ __forceinline__ bool tick_ge(int f, int k, int onset, int nfr) { return f < nfr && f - (k - 1) >= onset; }

/* Round 7: one general and one steady copy of every role's beat.  Once the onset is known and the pipeline is full, every flag a role
 * derives from (f, onset, nfr) is true until the utterance runs out (ns6_beat_plan.h: all of them hold exactly on the beats
 * steady_begin <= i < steady_end).  A role's beat is ONE body, a lambda taking the compile-time STEADY; with STEADY every flag is the
 * literal `true` (beat_flag), the onset is not polled, and what only the fill and the drain need (FA's gate, S's firstOut and its
 * zero-filled output frames) folds away.  Ticks, ring slots and the arithmetic are the same expressions in both copies.
 *
 * run_beats is the loop of every role.  Invariants:
 *   Barriers.  Each call of beat(.., i), general or steady, executes exactly one block_sync(), and i goes up by one after each call
 *     and by nothing else: the inner loop runs beat<true>(i) for i .. e-1 and leaves i = e, the statement after it runs
 *     beat<false>(i) and ++i only while i < niter.  i starts at 0 and the outer loop ends at i == niter, so every wave executes exactly
 *     niter barriers whatever its role, its variant and its switch points are; roles switch at different beats, which no barrier sees.
 *   The switch is decided in the general loop only, once per beat: `onset` is the role's own register copy, which only the general
 *     copy updates (onset_poll, FA's gate), so "not yet" may still be read for "invalid" exactly as before (comment at kNoOnset), and
 *     steady_begin(kNoOnset) = kNoOnset is above every beat.
 *   After the steady loop i = min(steady_end, niter) and control is back in the same general copy for the drain; the test is then true
 *     again on every drain beat and the inner loop runs zero times (e <= i).
 *   Frames after the onset: the flags hold for EVERY frame onset <= f < nfr, zero or not (the gate has one degree of freedom), so the
 *     steady copy never looks at the samples' being zero.
 *   FA: steady_end(FA) = nfr - 1 (RolePlan::ahead), so a steady beat's prefetch of frame i + 1 stays inside the utterance -- for the
 *     last utterance of the batch that is the end of the packed buffer.
 *   S: steady_begin(S) = onset + 14 (RolePlan::settle): the first produced frame is onset + 4 at beat onset + 13, in the general
 *     copy, which sets firstOut; the steady copy never touches it.
 *   PAIRED (round 12): the steady beats run two by two, an even beat and the odd one after it, written as beat(2h), beat(2h + 1).  The
 *     frame parity -- by which the records between the roles and the two transform work areas are double-buffered -- is then a
 *     constant of each of the two copies: every `(i - k) & 1` folds, record addresses become instruction offsets, and the compiler
 *     keeps the transform's operand addresses unpacked in registers instead of forming base + packed half-word before every LDS
 *     access.  The general copy is valid on every beat, so a steady range that begins on an odd beat gives its first beat to the
 *     general copy (the test `(i & 1) == 0` fails once, the statement behind it runs beat<false>(i) and ++i, and the range is entered
 *     on the next pass), and one that ends behind an even beat its last (h stops at e >> 1, i = 2h = e - 1 < e).  Each call still
 *     executes one barrier and i goes up by one per call, so the barrier count above holds; the steady copies only ever see
 *     steady_begin <= i < steady_end, as before. */
template <bool B>
struct BoolC {
    static constexpr bool value = B;
};
/* the flag "frame i - D exists and has tick >= K" of role ROLE; it must be in the role's beat plan, from which the steady range follows */
template <unsigned VARIANT, int ROLE, int D, int K, bool STEADY>
__device__ __forceinline__ bool beat_flag(int i, int onset, int nfr)
{
    static_assert(ns6plan::has_flag(VARIANT, ROLE, D, K), "a flag the beat plan of ns6_beat_plan.h does not know");
    return STEADY || tick_ge(i - D, K, onset, nfr);
}
struct NoEnter {
    __device__ __forceinline__ int operator()(int h) const { return h; }
};
template <bool STEADY_LOOP, unsigned VARIANT, int ROLE, bool PAIRED = false, class Beat, class Enter = NoEnter>
__device__ __forceinline__ void run_beats(int niter, int nfr, const int &onset, Beat &&beat, Enter &&enter = Enter{})
{
    int i = 0;
    while (i < niter) {
        if (STEADY_LOOP && i >= ns6plan::steady_begin(VARIANT, ROLE, onset)) {
            const int e0 = ns6plan::steady_end(VARIANT, ROLE, nfr), e = e0 < niter ? e0 : niter;
            if constexpr (PAIRED) {
                if ((i & 1) == 0) { /* an odd beat in front goes through the general copy below, and so does one left over behind */
                    /* enter: the role's hook at the switch into a steady range; it gets the pair counter's first value and returns
                     * the one to count from (FA: the same number, stated to be wave-uniform) */
                    int h = enter(i >> 1);
                    for (const int he = e >> 1; h < he; ++h) {
                        beat(BoolC<true>{}, 2 * h);
                        beat(BoolC<true>{}, 2 * h + 1);
                    }
                    i = 2 * h;
                }
            } else
                for (; i < e; ++i) beat(BoolC<true>{}, i);
        }
        if (i < niter) {
            beat(BoolC<false>{}, i);
            ++i;
        }
    }
}

/* The second-stage schedule and its ring depths.  Everything written at iteration w is visible from iteration w+1 on (the frame
 * barrier); a slot may be written again at the iteration of its last read at the earliest when writer and reader touch different
 * slots there, i.e. a ring of depth D written at f+w and last read at f+r needs f+D+w > f+r: D > r - w.
 *   frame f is        transformed (stage 1) by FA at f+3, FB at f+4       (unchanged)
 *                     noise-tracked by N1 at f+5      -> rn[f].P, rn[f].noise
 *                     noise-summed by S at f+6        -> nzSum[f]          (the 65 addends are rn[f].noise)
 *                     gain-factored by N1 at f+7      -> alfa[f]           (nzSum[f], denSum of ticks t-2 .. t)
 *                     filtered by G1 at f+8           -> ro[f]             (p1[f], rn[f], alfa[f], stage-1 buffer)
 *                     DC-filtered and stored by S at f+9 = f+kDepth
 *   p1 (stage-1 PSD)  written by FB at f+4, read by N1 at f+5 and by G1 at f+8: D > 4, five would do; eight makes the slot a mask
 *   rn (P, noise)     written at f+5, read by S at f+6 and by G1 at f+8: D > 3, kRnRing = 4
 *   nzSum, alfa, ro   written at one iteration, read at the next: D > 1, by frame parity
 *   denSum[tick & 7]  tick t (frame f) written by S at f+3; N1 reads ticks t-2 .. t for the frames f .. f+2, the last at f+9: D > 6
 *   fdFlags[tick & 7] written by B0 at f+2, read by S at f+9: D > 7 -- eight still hold, by one
 *   frameEn, frameEnLog, rd, p0: between FA, B0 and S's first two chains, whose frame offsets did not move
 *   stage-1 buffer    B0 writes the slot of tick t+6 (frame f+6, at iteration f+8) while G1 reads the window of tick t, slots
 *                     t-3 .. t, and FA that of tick t+5 (frame f+5 at f+8), slots t+2 .. t+5: ten live slots, eight collide
 *                     (t+6 = t-2 mod 8), so kSlots1 = 16, with the same three mirrored slots behind the last one
 *   REDEAL            FA itself writes the stage-1 slot, one iteration later: at iteration f+8 the slot of tick t+5 (frame f+5), which
 *                     its own window of that beat reads right after (same wave, wave_sync between), while G1 reads slots t-3 .. t:
 *                     nine live slots, eight still collide (t+5 = t-3 mod 8), sixteen do not; the slot's previous content, tick t-11,
 *                     was last read by G1 at iteration f.  The filter reads the stage-0 slots of ticks t+2 .. t+4 (buf[72..167] of the
 *                     window of tick t+5) while FA's own push of that beat writes the slot of tick t+8 = t (mod 8) and S reads that of
 *                     tick t+7: no other wave writes the stage-0 buffer, and FA's write is to none of the three.  kDepth stays 9.
 *   tap               B0 writes the nine IDCT sums of frame f at f+2, FA reads them at f+3: D > 1, by frame parity
 *   frameEnLog        REDEAL: N1 writes the slot (tick + 2) & 7 of the frame pushed at i-2 at iteration i, B0 reads it two iterations
 *                     later -- LIGHT's timing, where FA writes it
 *   BIN64 (round 10)  B0 takes stage-1 bin 64 of frame f at f+6: it reads p1[f] (written at f+4, last read by G1 at f+8) and rn[f]
 *                     (written at f+5, last read at f+8) inside their lifetimes, so neither ring grows.  It leaves the gain in
 *                     w1hi[f], written at f+6, read by G1 at f+8: D > 2, three would do; four makes the slot a mask (kW1Ring).
 *                     N1's domain flag of frame f sits in rn[f].P[kNsFastWord] and lives as rn does.
 *   IDCTS (round 11)  every stage-1 job one beat later, the filter two beats behind the gains:
 *                     frame f is transformed (stage 1) by FA at f+4, FB at f+5; noise-tracked at f+6 (B0's guest: f+7); noise-summed at
 *                     f+7; gain-factored at f+8; G1 takes its gains and leaves the products at f+9; S adds them up at f+10; G1 filters
 *                     at f+11 -> ro[f]; S stores at f+12 = f+DEPTH.  Stage 0: B0's products at f+2, S's sums at f+3, FA's filter at f+4.
 *   p1                written at f+5, read by N1 at f+6, B0 at f+7, G1 at f+9: D > 4, as before
 *   rn                written at f+6, read by S and B0 at f+7, by G1 at f+9: D > 3, as before
 *   w1hi              written at f+7, read at f+9: D > 2, as before
 *   nzSum, alfa, ro   f+7 -> f+8, f+8 -> f+9, f+11 -> f+12: by frame parity, as before
 *   prod, tap         written at one iteration, read at the next (B0 f+2 -> S f+3 -> FA f+4; G1 f+9 -> S f+10 -> G1 f+11): by frame
 *                     parity; at one beat S reads stage 0's record of parity (i-3) & 1 and stage 1's of the other, (i-10) & 1
 *   denSum[tick & 7]  tick t written by S at f+3; N1 reads ticks t-2 .. t for the frames f .. f+2, the last at f+2+8: D > 7 -- eight
 *                     still hold, by one
 *   fdFlags           not this variant's (no FD)
 *   stage-1 buffer    FA writes the slot of frame i-4 at iteration i (tick t+7, where t is the tick of frame i-11), and its own
 *                     window of that beat reads slots t+4 .. t+7; G1's filter of frame i-11 reads slots t-3 .. t: eleven live slots,
 *                     sixteen do not collide (t+7 = t-9 mod 16); the slot's previous content, tick t-9, was last read by G1 at
 *                     iteration i-6.  The three mirrored slots are written with their slots and live as they do.
 *   stage-0 buffer    FA's filter of frame i-4 reads the slots of frames i-7 .. i-5 (buf[72..167] of that frame's window) while its push
 *                     of that beat writes the slot of frame i = i-8 (mod 8), and its own window reads i-3 .. i: no collision, by one
 *   LDS               31 856 B per workgroup; five fit a CU's 160 KB, which is what the compiler's occupancy of 7 counts
 *   FIRP (round 14)   both filters in G1, FA's stage-1 window behind a frame barrier, every stage-1 job one more beat later:
 *                     stage 0: B0's products at f+2, S's sums at f+3, G1's filter (low half) at f+4 -> the stage-1 buffer.  Frame f is
 *                     transformed (stage 1) by FA at f+5, FB at f+6; noise-tracked at f+7 (B0's guest: f+8); noise-summed at f+8;
 *                     gain-factored at f+9; G1 takes its gains and leaves the products at f+10; S adds them up at f+11; G1 filters
 *                     (high half) at f+12 -> ro[f]; S stores at f+13 = f+DEPTH.
 *   p1                written at f+6, read by N1 at f+7, B0 at f+8, G1 at f+10: D > 4, as before
 *   rn                written at f+7, read by S and B0 at f+8, by G1 at f+10: D > 3, as before
 *   w1hi              written at f+8, read at f+10: D > 2, as before
 *   nzSum, alfa, ro   f+8 -> f+9, f+9 -> f+10, f+12 -> f+13: by frame parity, as before
 *   prod, tap         B0 f+2 -> S f+3 -> G1 f+4; G1 f+10 -> S f+11 -> G1 f+12: by frame parity; at one beat S reads stage 0's record of
 *                     parity (i-3) & 1 and stage 1's of the SAME parity, (i-11) & 1 -- all four product records sit in the same bank
 *                     slots (asserted below), so which two meet does not matter -- and G1's two halves read the tap records of one
 *                     parity, (i-4) & 1 = (i-12) & 1
 *   denSum            tick t written by S at f+3; N1 reads ticks t-2 .. t for the frames f .. f+2, the last at f+2+9: D > 8.  Eight
 *                     no longer hold (at iteration f+11 S writes tick t+8 while N1 reads tick t): the variant has a ring of its own,
 *                     Pipe6Idct::denSum16, sixteen deep (kDenRing16); Pipe6Lds::denSum stays for the other kernels
 *   stage-1 buffer    G1 writes the slot of frame i-4 at iteration i (tick T) and its three mirrored words' slot with it; FA's window
 *                     of frame i-5 reads slots T-4 .. T-1 (written at iterations i-4 .. i-1, each behind a barrier), G1's high half
 *                     reads buf[72..168] of the window of frame i-12, slots T-11 .. T-9: twelve live slots T-11 .. T, sixteen do not
 *                     collide (the slot's previous content, tick T-16 = frame i-20, was last read by G1 at iteration i-7, as the last slot
 *                     of frame i-19's filter).  A mirrored slot is written only with its slot and read only as that slot's tick: it lives as the slot does.
 *   stage-0 buffer    its reader is now G1, concurrently with FA's push of that beat (until now both were FA): G1's low half reads
 *                     buf[72..168] of the window of frame i-4, i.e. the slots of frames i-7 (8 words), i-6 and i-5 (9 words; the
 *                     ninth, buf[168], only feeds lane 26's unused third output), FA writes the slot of frame i = i-8 (mod 8) and,
 *                     for slots 0..2, its mirrored copy: a different tick mod 8 from all three, so neither the slot nor its mirror is
 *                     one G1 reads -- by one, as before; S reads the slot of frame i-1.  The slots G1 reads were written at iterations
 *                     i-7 .. i-5.
 *   LDS               31 920 B per workgroup (+ 64 for denSum16): five still fit a CU's 160 KB
 *   LOGP (round 15)   frameEn, frameEnLog in a steady pair (2h, 2h+1): the slot of tick(2h) is written by S at 2h-1, read by N1 at 2h+1
 *                     (was 2h) and rewritten by S at 2h+7; its logarithm is written by N1 at 2h+1 (was 2h), read by B0 at 2h+2 and
 *                     rewritten at the earliest at 2h+8.  The slot of tick(2h+1) keeps its beats (S 2h, N1 2h+1, B0 2h+3).  At beat
 *                     2h+1 S writes the slot of tick(2h+2), which is neither.  Rings of eight hold both with room; no schedule moved.
 * nbFrame of the gain-factor job: N1's counter has by then counted the two frames tracked since; the job takes the frame's own
 * count, tick - 4 (the first second-stage frame has tick 5).
 * LDS: 24 960 B per workgroup (24 624 + the two tap records + the ring of W1[64]); four workgroups per CU take 99.8 KB of the 160. */
constexpr int kP1Ring = 8;
constexpr int kRnRing = 4;
constexpr int kW1Ring = 4;
constexpr int kDenRing16 = 16;
struct __attribute__((aligned(16))) RecPsd { /* FB -> B0 (stage 0) / N1, G1 (stage 1) */
    float psd[68];
};
struct __attribute__((aligned(16))) RecDen { /* B0 -> S */
    float den[68];
};
struct __attribute__((aligned(16))) RecN { /* N1 -> S (noise[0..67], [65..67] stay zero), G1 */
    float P[68], noise[68];
};
struct __attribute__((aligned(16))) RecOut { /* G1 -> S */
    float out[80]; /* second-stage filter output before the DC-offset filter */
};

struct __attribute__((aligned(16))) RecTap { /* B0 -> FA: ns_idct_head's record, of which [28..36] are written and read */
    float rec[kIdctRecFloats];
};

struct __attribute__((aligned(16))) Pipe6Lds {
    float circ0[kCirc + kMirror];   /* stage-0 buffer: kSlots slots and three mirrored ones */
    float circ1[kCirc1 + kMirror];  /* stage-1 buffer: kSlots1 slots and three mirrored ones */
    float work[2][512];             /* transform work areas: FA fills [i & 1], FB finishes [(i-1) & 1] */
    BackLds back[2];                /* scratch of B0 and G1 */
    float ssq[80], sdif[80], sout[80], szero[4]; /* scratch of S */
    float frameEn[kSlots], denSum[kSlots];
    int onset;                      /* index of the first non-zero frame, kNoOnset until FA has met it */
    float frameEnLog[kSlots];       /* LIGHT, REDEAL: frameEn = 64 + sum of squares (S), frameEnLog = its log-energy (FA / N1, one beat later) */
    int fdFlags[kSlots];
    float idctT[SEA_NMEL * 16];
    RecPsd p0[2], p1[kP1Ring];
    RecDen rd[2];
    RecN rn[kRnRing];
    RecOut ro[2];
    float nzSum[2], alfa[2];        /* S -> N1: in-order sum of rn[f].noise; N1 -> G1: alfaGF of frame f; both by frame parity */
    RecTap tap[2];                  /* B0 -> FA (dense form): the stage-0 filter's taps before their window, by frame parity */
    float w1hi[kW1Ring];            /* B0 -> G1 (dense form, BIN64): the stage-1 gain of bin 64 */
};
/* The helper wave reads its four sources with one ds_read_b128 per quad; lanes of different chains share a lane group
 * ({ssq, den} in two of the four groups, {dif, noise} in the other two; past term 68 the sums read szero), so two sources that sit a
 * multiple of 256 B apart would cost an LDS cycle more per quad (both are 16-byte aligned: equal slot or disjoint banks).  That is the
 * bank rule of ds_read_b128 applied to this layout, NOT a measurement: no layout that breaks one of these conditions was run.  What was
 * measured is this layout's SQ_LDS_BANK_CONFLICT as a whole (profiles/ns6_noise_sum_in_helper.txt). */
constexpr bool lds_slots_differ(size_t a, size_t b) { return (a % 256) != (b % 256); }
#define NS6_OFF(m) offsetof(Pipe6Lds, m)
static_assert(lds_slots_differ(NS6_OFF(ssq), NS6_OFF(rd[0].den)) && lds_slots_differ(NS6_OFF(ssq), NS6_OFF(rd[1].den)), "ssq | den");
static_assert(lds_slots_differ(NS6_OFF(sdif), NS6_OFF(rn[0].noise)) && lds_slots_differ(NS6_OFF(sdif), NS6_OFF(rn[1].noise)) &&
              lds_slots_differ(NS6_OFF(sdif), NS6_OFF(rn[2].noise)) && lds_slots_differ(NS6_OFF(sdif), NS6_OFF(rn[3].noise)), "sdif | noise");
/* DIFG1: dif = ro[fo & 1].out with fo = i - 9, noise = rn[(i - 6) & 3]: opposite parities */
static_assert(lds_slots_differ(NS6_OFF(ro[0].out), NS6_OFF(rn[1].noise)) && lds_slots_differ(NS6_OFF(ro[0].out), NS6_OFF(rn[3].noise)) &&
              lds_slots_differ(NS6_OFF(ro[1].out), NS6_OFF(rn[0].noise)) && lds_slots_differ(NS6_OFF(ro[1].out), NS6_OFF(rn[2].noise)), "ro | noise");
static_assert(lds_slots_differ(NS6_OFF(ssq[68]), NS6_OFF(szero)) && lds_slots_differ(NS6_OFF(ssq[72]), NS6_OFF(szero)) &&
              lds_slots_differ(NS6_OFF(ssq[76]), NS6_OFF(szero)), "ssq tail | szero");
static_assert(lds_slots_differ(NS6_OFF(sdif[68]), NS6_OFF(szero)) && lds_slots_differ(NS6_OFF(sdif[72]), NS6_OFF(szero)) &&
              lds_slots_differ(NS6_OFF(sdif[76]), NS6_OFF(szero)), "sdif tail | szero");
static_assert(lds_slots_differ(NS6_OFF(ro[0].out[68]), NS6_OFF(szero)) && lds_slots_differ(NS6_OFF(ro[0].out[72]), NS6_OFF(szero)) &&
              lds_slots_differ(NS6_OFF(ro[0].out[76]), NS6_OFF(szero)) && lds_slots_differ(NS6_OFF(ro[1].out[68]), NS6_OFF(szero)) &&
              lds_slots_differ(NS6_OFF(ro[1].out[72]), NS6_OFF(szero)) && lds_slots_differ(NS6_OFF(ro[1].out[76]), NS6_OFF(szero)), "ro tail | szero");
#undef NS6_OFF
static_assert(sizeof(Pipe6Lds) == 24960 && 4 * sizeof(Pipe6Lds) <= 160 * 1024 && sizeof(Pipe6Lds) < 40 * 1024,
              "the figure in the comment at kP1Ring; four workgroups fit a CU");

/* IDCTS (round 11, the dense kernel): what the IDCT sums in the helper wave need, behind the record every six-wave kernel has -- whose
 * layout, and with it the other two kernels' listings and LDS size, stays as it was (tap[] is the one member the dense kernel no longer
 * touches).  prod: the products B0 ([0]) and G1 ([1]) leave, by frame parity, read by S one beat later; tap: S's nine sums per stage
 * times their Hanning weights, by frame parity, read by FA / G1 one beat later; zeros: what S's row lanes
 * read behind their 28 terms, and its den and noise lanes behind their 68.
 * Bank rule of S's ds_read_b128 (as above: a 16-lane group serves 256 B per clock, so two DIFFERENT addresses of a group must differ
 * mod 256 B; equal addresses are one access).  The groups are {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (and two more in lanes
 * 32-63, which carry no row): each holds the VAD lanes' ssq + n, the den lanes' den + n, three rows of one stage and six of the other.
 * Every product record is a multiple of 256 B long, so all four put their row t into the same slot, and S's two records of a beat
 * have opposite frame parities.  ssq sits in slot 12 of 16, den in slots 0 and 1 by parity: with rows 28 floats = 7 slots apart no
 * offset of the records keeps both groups free of a collision (nor with 9, 13: searched over all offsets), with 11 slots = 44 floats
 * (kIdctStride) three offsets do, with 15 two; 44 is the shorter record.  From n = 28 on the row lanes read zeros + n - 28 (one address), from n = 68 on the
 * den and noise lanes zeros + n - 68: both must miss ssq + n, the first den + n as well, the second sdif + n.  All of it asserted
 * below; as above it is the rule applied, what was measured is SQ_LDS_BANK_CONFLICT as a whole (profiles/ns6_idct_in_helper.txt). */
struct __attribute__((aligned(16))) Pipe6Idct {
    float tap[2][2][kIdsTapFloats];    /* [stage][frame parity]: the nine windowed taps, kIdsTapStride apart */
    float pad0[4];                     /* puts zeros, */
    float zeros[kIdsZeros];
    float pad[4];                      /* and the rows' slots, where ssq, sdif and den are not */
    float prod[2][2][kIdctProdFloats]; /* [stage][frame parity] */
    float denSum16[kDenRing16];        /* FIRP: S's denSigSE1 sums by tick & 15, in place of Pipe6Lds::denSum (derivation at kP1Ring) */
};
/* basisQ takes the place of idctT, which this variant does not read: four workgroups need 4 x 40 KB at the most, but the compiler's
 * occupancy figure counts whole workgroups against the CU's 160 KB, and seven waves per SIMD are five of these, 32 KB each */
constexpr int kIdctBasisAt = 3; /* floats into idctT: the first 16-byte boundary */
struct __attribute__((aligned(16))) Pipe6LdsIdct {
    Pipe6Lds base;
    Pipe6Idct x;
};
constexpr size_t lds_slot(size_t off) { return (off / 16) % 16; }
/* the slots of one 16-lane group at n < 28: ssq, den, rows r0 .. r1-1 of one record and the other rows of the other, all different */
constexpr bool lds_group_ok(size_t ssq, size_t den, size_t recA, size_t recB, int r0, int r1)
{
    size_t sl[11] = {lds_slot(ssq), lds_slot(den)};
    int n = 2;
    for (int r = 0; r < 9; ++r) sl[n++] = lds_slot(((r >= r0 && r < r1) ? recA : recB) + r * kIdctStride * sizeof(float));
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (sl[i] == sl[j]) return false;
    return true;
}
#define NS6_OFF(m) offsetof(Pipe6LdsIdct, m)
static_assert(NS6_OFF(base) == 0 && NS6_OFF(x.prod) % 256 == NS6_OFF(x.prod[0][1]) % 256 && NS6_OFF(x.prod) % 256 == NS6_OFF(x.prod[1][0]) % 256 &&
                  NS6_OFF(x.prod) % 256 == NS6_OFF(x.prod[1][1]) % 256 && NS6_OFF(x.prod) % 16 == 0 && (kIdctRow * sizeof(float)) % 16 == 0 &&
                  (NS6_OFF(base.idctT) + kIdctBasisAt * sizeof(float)) % 16 == 0 && kIdctBasisAt + kIdctBasisFloats <= SEA_NMEL * 16 &&
                  NS6_OFF(x.tap[0][1]) % 16 == 0 && NS6_OFF(x.tap[1][1]) + kIdsTapReach * sizeof(float) <= sizeof(Pipe6LdsIdct),
              "the four product records share their slots");
/* lanes 1-3 | 4-9 have stage-0 rows 0-2 | 3-8 (record of den's parity), lanes 20-25 | 17-19 stage-1 rows 3-8 | 0-2 (the other parity) */
static_assert(lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[0].den), NS6_OFF(x.prod[0][0]), NS6_OFF(x.prod[1][1]), 0, 3) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[0].den), NS6_OFF(x.prod[0][0]), NS6_OFF(x.prod[1][1]), 3, 9) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[1].den), NS6_OFF(x.prod[0][1]), NS6_OFF(x.prod[1][0]), 0, 3) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[1].den), NS6_OFF(x.prod[0][1]), NS6_OFF(x.prod[1][0]), 3, 9) &&
                  (kIdctStride * sizeof(float)) % 16 == 0, "n < 28: ssq, den | the rows, in both groups and both parities");
/* FIRP: stage 1's record has the parity of stage 0's */
static_assert(lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[0].den), NS6_OFF(x.prod[0][0]), NS6_OFF(x.prod[1][0]), 0, 3) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[0].den), NS6_OFF(x.prod[0][0]), NS6_OFF(x.prod[1][0]), 3, 9) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[1].den), NS6_OFF(x.prod[0][1]), NS6_OFF(x.prod[1][1]), 0, 3) &&
                  lds_group_ok(NS6_OFF(base.ssq), NS6_OFF(base.rd[1].den), NS6_OFF(x.prod[0][1]), NS6_OFF(x.prod[1][1]), 3, 9),
              "the same with both stages' records of one parity");
static_assert(NS6_OFF(x.zeros) % 16 == 0 && lds_slots_differ(NS6_OFF(x.zeros) + 256 - kIdctRow * sizeof(float), NS6_OFF(base.ssq)) &&
                  lds_slots_differ(NS6_OFF(x.zeros) + 256 - kIdctRow * sizeof(float), NS6_OFF(base.rd[0].den)) &&
                  lds_slots_differ(NS6_OFF(x.zeros) + 256 - kIdctRow * sizeof(float), NS6_OFF(base.rd[1].den)), "28 <= n: the rows' zeros | ssq, den");
static_assert(lds_slots_differ(NS6_OFF(x.zeros) + 512 - 68 * sizeof(float), NS6_OFF(base.ssq)) &&
                  lds_slots_differ(NS6_OFF(x.zeros) + 512 - 68 * sizeof(float), NS6_OFF(base.sdif)) &&
                  lds_slots_differ(NS6_OFF(x.zeros) + 512 - 68 * sizeof(float), NS6_OFF(x.zeros) + 256 - kIdctRow * sizeof(float)),
              "68 <= n: the den and noise lanes' zeros | ssq, sdif, the rows' zeros");
#undef NS6_OFF
static_assert(4 * sizeof(Pipe6LdsIdct) <= 160 * 1024 && 5 * sizeof(Pipe6LdsIdct) <= 160 * 1024, "four workgroups fit a CU; five, for the compiler's occupancy of 7");

/* SLOTS: kSlots for the stage-0 buffer, kSlots1 for the stage-1 buffer */
template <int SLOTS>
__device__ __forceinline__ int window_base(int tick) { return ((tick - 3) & (SLOTS - 1)) * kSlotLen; }

template <int SLOTS>
__device__ __forceinline__ void slot_store(float *circ, int tick, int lane, float a, float b)
{
    const int slot = tick & (SLOTS - 1);
    float *p = circ + slot * kSlotLen + 2 * lane;
    *reinterpret_cast<float2 *>(p) = make_float2(a, b);
    if (slot < 3) *reinterpret_cast<float2 *>(p + SLOTS * kSlotLen) = make_float2(a, b);
}

__device__ __forceinline__ void block_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ void load_back_const(NsConst &C, const sea_ns_tables *t, int lane)
{
    C.melStart = t->melStart[lane];
    C.melLen = t->melLen[lane];
#pragma unroll
    for (int i = 0; i < SEA_MEL_TAPS; ++i) C.melW[i] = t->melW[i][lane];
    C.irWin = t->irWin[lane];
    C.eps = t->eps;
}

template <bool FD, bool LIGHT /* the VAD log leaves S */, bool DIFG1 /* G1 hands over the DC differences */,
          bool STEADY_LOOP /* the flag-free copy of every role's beat on its steady range (run_beats) */,
          bool REDEAL = false /* round 8, the dense kernel: feed-forward work of S and B0 in the waves that wait, and the map that goes with it */,
          bool BIN64 = false /* round 10, the dense kernel: stage-1 bin 64 rides in B0's second component, one domain flag per stage-1 frame */,
          bool IDCTS = false /* round 11, the dense kernel: both stages' IDCT sums ride in the helper wave's idle lanes; X is its LDS */,
          bool PAIRED = false /* round 12, all three kernels: the steady beats two by two, the frame parity a constant of each copy (run_beats) */,
          bool FIRP = false /* round 14, the dense kernel: both 17-tap filters as one pass on G1's two lane halves, off FA (ns_core.h, ns_fir_pair3) */,
          bool LOGP = false /* round 15, the dense kernel: the two VAD logarithms of a steady pair of beats as one pass on N1's lanes (ns_core.h, ns_log_lanes_request) */>
__device__ __forceinline__ void ns_pipe6_body(const NsBatchArgs &a, Pipe6Lds &L, Pipe6Idct *X = nullptr)
{
    static_assert(!REDEAL || (!LIGHT && !DIFG1), "the re-deal is a variant of the dense body");
    static_assert(!BIN64 || (REDEAL && !FD), "the guest of B0's second component is a variant of the re-dealt dense body");
    static_assert(!IDCTS || BIN64, "the IDCT sums in the helper wave are a variant of that body in turn");
    static_assert(!PAIRED || STEADY_LOOP, "the paired beats are the steady copies'");
    static_assert(!FIRP || IDCTS, "the merged filter pass takes both stages' taps from the helper wave");
    static_assert(!LOGP || (REDEAL && PAIRED), "the paired logarithms are N1's (LOG_N1), in the odd copy of its steady pair");
    constexpr unsigned V = (FD ? ns6plan::kFd : 0u) | (LIGHT ? ns6plan::kLight : 0u) | (DIFG1 ? ns6plan::kDifg1 : 0u) | (REDEAL ? ns6plan::kRedeal : 0u) |
                           (BIN64 ? ns6plan::kBin64 : 0u) | (IDCTS ? ns6plan::kIdctS : 0u) | (FIRP ? ns6plan::kFirPair : 0u);
    static_assert(!BIN64 || V == (FIRP ? ns6plan::kVariantDenseFirPair : (IDCTS ? ns6plan::kVariantDenseIdct : ns6plan::kVariantDenseBin64)),
                  "the variants tests/test_ns6_fir_plan_cpu.py, tests/test_ns6_idct_plan_cpu.py and tests/test_ns6_bin64_plan_cpu.py sweep");
    /* IDCTS (profiles/ns6_idct_in_helper.txt): DoMelIDCT's nine in-order sums of 25 terms, twice per frame, cost B0 and G1 25 lane reads,
     * 25 basis reads, 25 multiplications and a chain of 25 dependent additions each, for nine useful lanes.  Here B0 (frame i-2) and G1
     * (frame i-9) stop at the rounded products (ns_idct_products), S adds the rows up one beat later in lanes that only repeated another
     * chain (helper_chains<.., IDS>: the same additions in the same order), and the filters follow one beat after that: FA filters
     * stage-0 frame i-4, so every stage-1 job sits one beat later than the table at kP1Ring has it (kS1), and G1 filters frame i-11 in
     * the beat in which it takes the gains of frame i-9.  The pipeline is three beats deeper (DEPTH). */
    /* FIRP (profiles/ns6_fir_merged.txt): the two filters -- stage-0 frame i-4 in FA, stage-1 frame i-11 in G1 -- were 2 x 68 vector
     * instructions on 40 of 64 lanes, and both become ready at the same beat: S leaves both stages' taps at i-1.  G1, the role with the
     * most slack, runs them as one pass on its two lane halves (ns_fir_pair3: 102 for both, one set of reads, no mirrored taps); FA,
     * workgroup 0's longest role, filters no more.  The filtered stage-0 frame now crosses a frame barrier before FA windows it, so
     * every stage-1 job sits one more beat later (kS1 = 2) and the pipeline is thirteen beats deep. */
    constexpr int kS1 = FIRP ? 2 : (IDCTS ? 1 : 0); /* beats by which stage 1 starts later */
    constexpr int DEPTH = ns6plan::depth_of(V);    /* S stores frame i - DEPTH */
    static_assert(DEPTH == (FIRP ? 13 : (IDCTS ? 12 : kDepth)) && DEPTH == 9 + 2 * (IDCTS ? 1 : 0) + kS1, "the depth the ring depths at kP1Ring are derived for");
    /* the ring of S's denSigSE1 sums, one per tick: FIRP reads it one beat later still and has sixteen (derivation at kP1Ring) */
    constexpr int kDenRing = FIRP ? kDenRing16 : kSlots;
    float *const denRing = FIRP ? X->denSum16 : L.denSum;
    /* BIN64 (profiles/ns6_bin64_in_b0.txt): the Wiener-gain chain ran on the pair (bin lane, bin 64) in B0 and in G1, and the second
     * component is one useful value in 64 identical lanes.  B0, at beat i, takes stage-1 bin 64 of frame g = i-6 into lane 1 of its
     * second component (ns_core.h, NsBin64) and leaves W1[64] in w1hi[g & 3]; G1 computes bins 0..63 with the single-component chain.
     * N1 publishes its fast-division decision of the frame, which G1 and B0 read instead of testing the PSD again.  The mixed pass
     * needs both frames inside the domain; otherwise, and on the four drain beats on which B0 has no stage-0 frame left, the guest
     * goes through plain IEEE division, which gives the same bits inside the domain (sea_selftest_nsdiv).  With int16 input every PSD
     * is inside the domain. */
    /* REDEAL moves two pieces whose inputs do not depend on the recursive state (profiles/ns6_redeal.txt):
     *   LOG_N1  the VAD log-energy: N1, which holds no transform tables and waited 1300 clk per beat, takes it one beat after S left the
     *           sum (LIGHT's timing, with N1 for FA: FA is the register-bound role of the 72-VGPR kernel)
     *   FIR_FA  the stage-0 17-tap filter: B0 stops at the nine IDCT sums, FA windows them and filters in the beat in which it reads the output
     * Same operations in the same order.  With them the roles are near 2400-2950 clk each instead of 1770-3110, and the wave -> role map
     * that was best before is no longer: kRedealPerm. */
    constexpr bool LOG_N1 = REDEAL, FIR_FA = REDEAL;
    const int lane = threadIdx.x & 63;
    /* LIGHT / DIFG1 (the forms for up to two utterances per CU, where the run time is one utterance's chain of frames): the helper
     * wave S was this form's longest role (3397 clk per frame alone, B0 3089, G1 2985, N1 2623, FB 2608, FA 2268): (LIGHT) the VAD's
     * log-energy (NoiseSup.c:391) is taken by the first transform wave FA one beat after S left the frame's sum of squares -- FA has
     * ~1000 clk of slack, the value is consumed by B0 two beats later still; (DIFG1) G1 hands over the DC filter's input differences
     * instead of the filtered frame (ns_gain1_dif), S's own pass over the frame goes.  S 3397 -> 2836, G1 2985 -> 3134,
     * FA 2268 -> 2694: 256 utterances 1.777 -> 1.664 ms.  NOT in the dense form: at four workgroups per CU the step is a throughput
     * limit and the same change costs 2 % there (1.99 against 1.95 ms).
     * The placement of the roles on the SIMDs decides at four utterances per CU (round 3, before the dense form: identity
     * 3.19 ms, 0104352 (B0, S, N1, G1, FA, FB) 2.78 ms, the ten even / odd splits in wave order 2.97-3.26 ms). */
    const int role = ((a.perm6 ? a.perm6 : (REDEAL ? kRedealPerm : kDefaultPerm)) >> (3 * __builtin_amdgcn_readfirstlane(threadIdx.x >> 6))) & 7;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u];
    /* frame counts and counters are 32-bit and scalar: 2^31 frames would be 172 G samples, in and out 687 GB, more than the device's
     * memory holds (a longer length is SILENTLY cut to kMaxFrames frames rather than wrapping: the lengths live in
     * device memory, so the C entry points cannot refuse one without a synchronising copy; PackedBatch.layout, which has them on the
     * host, refuses it).  Byte and sample offsets into the streams are still
     * formed in 64 bits (a single utterance may exceed 2^31 samples). */
    const long long nfr64 = a.lengths[u] / SEA_HOP;
    const int nfr = __builtin_amdgcn_readfirstlane((int)(nfr64 < kMaxFrames ? nfr64 : kMaxFrames));
    const int niter = nfr + DEPTH;
    /* issue priority by remaining frames, the rule of the four-wave form (ns_pipe_kernel.hip): on whenever the
     * launch has more utterances than CUs to put them on and an order whose first entry is the longest */
    const bool lrpt = a.prio_row > 0 && a.order;
    const long long longestFr = lrpt ? a.lengths[a.order[0]] / SEA_HOP : 0;
    const float lrptScale = (float)kPrioLevels / (float)(longestFr > 0 ? longestFr : 1);
    const int lrptBias = lrpt ? (int)blockIdx.x / a.prio_row : 0; /* equal levels: the hardware prefers the oldest wave */
    auto prio_by_remaining = [&](int i) {
        if ((FD ? lrpt : true) && (i & (kPrioStep - 1)) == 0) {
            /* round 13: the beat's own test first and alone, one scalar compare and branch; the empty statement keeps the compiler from
             * merging it with the launch's flag into a lane-mask expression of six instructions per beat.  Not in the _fd kernel, whose
             * G1 gains four moves per pair of beats with it (its period is B0's beat: nothing to win there). */
            if constexpr (!FD) {
                asm volatile("");
                if (!lrpt) return;
            }
            const int L = __builtin_amdgcn_readfirstlane((int)((float)(nfr - i) * lrptScale)) + lrptBias;
            const int pr = (L + (int)(((unsigned)i / kPrioStep) & (kPrioLevels / 4 - 1))) / (kPrioLevels / 4);
            if (pr >= 3) __builtin_amdgcn_s_setprio(3);
            else if (pr == 2) __builtin_amdgcn_s_setprio(2);
            else if (pr == 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
    };

    { /* both buffers, the first members of the record, cleared in one loop */
        static_assert(offsetof(Pipe6Lds, circ0) == 0 && offsetof(Pipe6Lds, circ1) == sizeof(float) * (kCirc + kMirror), "circ0 | circ1 lead the record");
        float *z = reinterpret_cast<float *>(&L);
        for (int i = threadIdx.x; i < kCirc + kCirc1 + 2 * kMirror; i += 64 * kWaves) z[i] = 0.0f;
    }
    if constexpr (!IDCTS)
        for (int i = threadIdx.x; i < SEA_NMEL * 16; i += 64 * kWaves) L.idctT[i] = a.tables->idct[i >> 4][i & 15];
    float *const basisQ = L.idctT + kIdctBasisAt; /* IDCTS: the basis in the product record's layout (ns_idct_products) */
    if (threadIdx.x < 4) L.szero[threadIdx.x] = 0.0f;
    if (threadIdx.x < kSlots) {
        L.frameEn[threadIdx.x] = 0.0f;
        L.frameEnLog[threadIdx.x] = 0.0f;
        L.denSum[threadIdx.x] = 0.0f;
    }
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        L.rd[k].den[65] = L.rd[k].den[66] = L.rd[k].den[67] = 0.0f; /* read as zeros by S */
        L.nzSum[k] = L.alfa[k] = 0.0f;
    }
    if (threadIdx.x < kRnRing) {
        const int k = threadIdx.x;
        L.rn[k].noise[65] = L.rn[k].noise[66] = L.rn[k].noise[67] = 0.0f; /* likewise */
    }
    if (threadIdx.x == 0) L.onset = kNoOnset;
    if constexpr (IDCTS) { /* the basis in the product record's layout, the rows' zero pads, the zero region, the pads of the two mel copies */
        for (int i = threadIdx.x; i < kIdctBasisFloats; i += 64 * kWaves) {
            const int t = i / kIdctRow, f = i % kIdctRow;
            basisQ[i] = (t < 9 && f < SEA_NMEL) ? a.tables->idct[f][t] : 0.0f;
        }
        if (threadIdx.x < kIdsZeros) X->zeros[threadIdx.x] = 0.0f;
        if (FIRP && threadIdx.x < kDenRing16) X->denSum16[threadIdx.x] = 0.0f;
        if (threadIdx.x < 6) L.back[threadIdx.x / 3].mel[SEA_NMEL + threadIdx.x % 3] = 0.0f;
    }
    block_sync();
    NS6_T_DECL;

    if (role == 0) {
        /* ---- FA: input + zero-frame gate (ParmInterface.c:244-251); first half of both transforms ---- */
        Fft2Regs fft;
        load_fft2_regs<false>(fft, &a.tables->fft, lane, nullptr);
        float win8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) win8[k] = a.tables->win8[k][lane];
        const float irWin = (FIR_FA && !IDCTS) ? a.tables->irWin[lane] : 0.0f; /* lane k = 0..8: the Hanning weight of tap 8 +- k (IDCTS: S has it) */
        const uint32_t *in32 = reinterpret_cast<const uint32_t *>(a.in + off);
        uint32_t nextw = (lane < 40 && nfr > 0) ? in32[lane] : 0u;
        int onsetG = kNoOnset; /* index of the first non-zero frame */
        /* Round 13: FA is the one role that WRITES its onset, under the gate's ballot, and the compiler takes the value -- and with
         * it the switch into the steady range, the beat counter, every tick and ring slot -- for lane-dependent: the slot and
         * address arithmetic of its steady copies ran on the vector unit.  The steady copies never change the onset (run_beats),
         * so at the switch they get it, and their pair counter, through v_readfirstlane (every lane holds the same number); from
         * there on counter, ticks, ring slots and the next frame's address are scalar, and the lane's part of an address is
         * formed once in front of the loop.  The general copy keeps onsetG and publishes it exactly as before. */
        int onsetS = kNoOnset;
        typedef const __attribute__((address_space(1))) uint32_t *FramePtr;
        unsigned long long nextFr = 0; /* steady copies: the address of frame i + 1 of the utterance, set at the switch, one frame on per beat */
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            int &onset = *(STEADY && PAIRED ? &onsetS : &onsetG);
            constexpr bool NEXT_S = STEADY && PAIRED; /* the next frame's address as a running scalar */
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if constexpr (LIGHT) { /* the log-energy of the sum S left one beat ago (the frame pushed at i-2 is its tick + 2's "current frame") */
                if (beat_flag<V, ns6plan::FA, 2, 1, STEADY>(i, onset, nfr)) {
                    const int e = (tick_of(i - 2, onset) + 2) & (kSlots - 1);
                    const float en = vad_frame_energy(L.frameEn[e]);
                    if (lane == 0) L.frameEnLog[e] = en;
                }
            }
            int tick = 0; /* frames seen since (and including) the first non-zero one */
            bool actA = false;
            if (STEADY || i < nfr) {
                const uint32_t w = nextw;
                if constexpr (!NEXT_S)
                    if ((STEADY || i + 1 < nfr) && lane < 40) nextw = (in32 + (long long)(i + 1) * 40)[lane];
                if (!STEADY && onset == kNoOnset && __ballot(w != 0u) != 0ull) {
                    onset = i;
                    if (lane == 0) __hip_atomic_store(&L.onset, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (STEADY || i >= onset) {
                    tick = tick_of(i, onset);
                    const float x0 = (float)(short)(w & 0xFFFFu), x1 = (float)(short)(w >> 16);
                    if (lane < 40) {
                        /* steady copies (round 13): the next frame's load under the same lanes' branch as the store, its address in
                         * SGPRs -- counted on from the switch into the range -- and the lane as the load's offset */
                        if constexpr (NEXT_S) nextw = reinterpret_cast<FramePtr>(nextFr)[lane];
                        slot_store<kSlots>(L.circ0, tick, lane, x0, x1);
                    }
                    if constexpr (NEXT_S) { /* outside the lanes' branch, and opaque: or it becomes a pointer per lane, two VGPRs */
                        nextFr += SEA_HOP * 2u;
                        asm("" : "+s"(nextFr));
                    }
                    static_assert(ns6plan::has_flag(V, ns6plan::FA, 0, 3), "frame i exists here: its flag is the tick alone");
                    actA = STEADY || tick >= 3; /* NoiseSup.c:1152 */
                }
            }
            /* stage 1, frame i-3 (B0 finished it at the previous iteration; IDCTS: frame i-4, S did; FIRP: frame i-5, G1 did): NoiseSup.c:1178 <=> tick >= 5 */
            const int t1 = tick_of(i - 3 - kS1, onset);
            const bool actB = beat_flag<V, ns6plan::FA, 3 + kS1, 5, STEADY>(i, onset, nfr);
            if constexpr (FIR_FA && !FIRP) { /* FIRP: G1 filtered frame i-5 at the previous iteration, behind a frame barrier */
                /* stage-0 filter of frame i-3 from the IDCT sums B0 left at the previous iteration; from tick 3, not 5: ticks 3 and 4
                 * leave output that the first stage-1 window reads.  Also in the drain, where FA has no frame of its own. */
                if (beat_flag<V, ns6plan::FA, 3 + kS1, 3, STEADY>(i, onset, nfr)) {
                    float y0, y1;
                    if constexpr (IDCTS) /* the taps S left at the previous iteration */
                        ns_fir_from_idct_taps(X->tap[0][(i - 4) & 1], L.circ0 + window_base<kSlots>(t1), lane, y0, y1);
                    else
                        ns_fir_from_idct_rec(L.tap[(i - 3) & 1].rec, irWin, L.circ0 + window_base<kSlots>(t1), lane, y0, y1);
                    if (lane < 40) slot_store<kSlots1>(L.circ1, t1, lane, y0, y1);
                    wave_sync();
                }
            }
            if (actA || actB) {
                wave_sync();
                float e[8];
                ns_window8(L.circ0 + window_base<kSlots>(tick), actA, L.circ1 + window_base<kSlots1>(t1), actB, win8, lane, e);
                if constexpr (STEADY && PAIRED && !FD) {
                    /* FA is the register-bound role of the 72-VGPR dense and of the 80-VGPR plain kernel: with all twelve address words
                     * of its transform half unpacked (run_beats, PAIRED) it spills five and four VGPRs there.  The four words of the
                     * register-resident start stay packed -- an empty statement that "changes" them every beat, so their halves cannot
                     * be taken out of the loop.  The _fd kernel has the registers (launch bound of two waves per SIMD). */
#pragma unroll
                    for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(fft.head8[q]));
                }
                rfft256_dual_lo<false>(e, L.work[i & 1], fft);
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::FA, PAIRED>(niter, nfr, onsetG, beat, [&](int h) {
            onsetS = __builtin_amdgcn_readfirstlane(onsetG);
            const int hs = __builtin_amdgcn_readfirstlane(h);
            unsigned long long fr = reinterpret_cast<unsigned long long>(in32 + (unsigned long long)(unsigned)(2 * hs + 1) * 40u);
            asm("" : "+s"(fr));
            nextFr = fr;
            return hs;
        });
        NS6_T_FLUSH(role, niter);
        if (FD && a.onset_out && lane == 0) a.onset_out[u] = onsetG == kNoOnset ? nfr : onsetG;
    } else if (role == 1) {
        /* ---- FB: second half of both transforms, FFTtoPSD ---- */
        Fft2Regs fft;
        load_fft2_regs<false>(fft, &a.tables->fft, lane, nullptr);
        int onset = kNoOnset;
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if (!STEADY) onset_poll(onset, &L.onset);
            const int g = i - 1; /* FA's iteration */
            if (STEADY || g >= 0) {
                const int f0 = g, f1 = g - 3 - kS1;
                const bool actA = beat_flag<V, ns6plan::FB, 1, 3, STEADY>(i, onset, nfr);
                const bool actB = beat_flag<V, ns6plan::FB, 4 + kS1, 5, STEADY>(i, onset, nfr);
                float *work = L.work[g & 1];
                if (actA || actB) {
                    float o[8]; /* the last level stays in registers and feeds both PSDs (ns_core.h, psd_from_last_level) */
                    rfft256_dual_hi_keep_last<false>(work, fft, o);
                    psd_from_last_level(o, fft, L.p0[f0 & 1].psd, actA, L.p1[f1 & (kP1Ring - 1)].psd, actB, lane);
                    wave_sync();
                }
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::FB, PAIRED>(niter, nfr, onset, beat);
        NS6_T_FLUSH(role, niter);
    } else if (role == 2) {
        /* ---- B0: BACK of stage 0; its 80 outputs enter the stage-1 buffer ---- */
        NsConst C;
        load_back_const(C, a.tables, lane);
        NsRegs s;
        regs_init(s, C.eps);
        NsFd fd;
        fd_init(fd);
        NsBin64 x; /* BIN64: the guest, stage-1 bin 64 */
        x.den = 0.0f; /* denSigSE2[64] as DoNoiseSupInit leaves it */
        x.W = 0.0f;
        int onset = kNoOnset;
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if (!STEADY) onset_poll(onset, &L.onset);
            const int f = i - 2, g = i - 6 - kS1;
            if constexpr (BIN64) {
                x.psd1 = L.p1[g & (kP1Ring - 1)].psd;
                x.P1 = L.rn[g & (kRnRing - 1)].P;
                x.noise1 = L.rn[g & (kRnRing - 1)].noise;
                x.live = beat_flag<V, ns6plan::B0, 6 + kS1, 5, STEADY>(i, onset, nfr);
                x.done = false;
            }
            if (beat_flag<V, ns6plan::B0, 2, 3, STEADY>(i, onset, nfr)) {
                const RecPsd &r = L.p0[f & 1];
                RecDen &o = L.rd[f & 1];
                const int t = tick_of(f, onset);
                int bits = 0;
                /* the filter taps as scalar operands (v_readlane), the filter's outputs in registers straight
                 * into the stage-1 buffer -- two LDS round trips less on this role's chain (ns_core.h, fir_taps_rl) */
                const float frameEn = ((LIGHT || LOG_N1) ? L.frameEnLog : L.frameEn)[t & (kSlots - 1)];
                if constexpr (IDCTS) { /* as BIN64 below, up to the IDCT's products; S adds them up at the next iteration */
                    ns_back<0, true, FD, true, SEA_NMEL, false, true, true, true>(r.psd, nullptr, L.back[0], s, C, X->prod[0][f & 1], lane, frameEn, o.den,
                                                                                  basisQ, &fd, &bits, nullptr, nullptr, nullptr, &x);
                } else if constexpr (BIN64) { /* as FIR_FA below, with the guest in lane 1 of the second component */
                    ns_back<0, true, FD, true, SEA_NMEL, false, true, true>(r.psd, nullptr, L.back[0], s, C, L.tap[f & 1].rec, lane, frameEn, o.den,
                                                                            L.idctT, &fd, &bits, nullptr, nullptr, nullptr, &x);
                } else if constexpr (FIR_FA) { /* stop at the nine IDCT sums; FA windows them and filters at the next iteration */
                    ns_back<0, true, FD, true, SEA_NMEL, false, true>(r.psd, nullptr, L.back[0], s, C, L.tap[f & 1].rec, lane, frameEn, o.den, L.idctT,
                                                         &fd, &bits);
                    if (FD && lane == 0) L.fdFlags[t & (kSlots - 1)] = bits;
                } else {
                    float y01[2] = {0.0f, 0.0f};
                    ns_back<0, true, FD, true, -1, false, true>(r.psd, L.circ0 + window_base<kSlots>(t), L.back[0], s, C, nullptr, lane, frameEn, o.den,
                                               L.idctT, &fd, &bits, nullptr, y01);
                    if (FD && lane == 0) L.fdFlags[t & (kSlots - 1)] = bits;
                    if (lane < 40) slot_store<kSlots1>(L.circ1, t, lane, y01[0], y01[1]);
                }
            }
            if constexpr (BIN64) {
                if (x.live) {
                    if (!x.done) { /* no stage-0 frame beside it (the drain), or one of the two frames outside the domain: IEEE division */
                        const float W = gain_bin<false>(sqrtf(x.P1[64]), sqrtf(x.psd1[64]), x.noise1[64], x.den);
                        x.W = W;
                    }
                    if (lane == 1) L.w1hi[g & (kW1Ring - 1)] = x.W;
                }
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::B0, PAIRED>(niter, nfr, onset, beat);
        NS6_T_FLUSH(role, niter);
    } else if (role == 3) {
        /* ---- N1: stage-1 noise tracking of frame i-5; gain-factor scalars of frame i-7, whose noise sum S took in between ---- */
        const float eps = a.tables->eps;
        NsRegs s;
        regs_init(s, eps);
        int onset = kNoOnset;
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if (!STEADY) onset_poll(onset, &L.onset);
            const int f = i - 5 - kS1, fg = i - 7 - kS1;
            /* LOGP, the steady pair (2h, 2h+1): nothing for the VAD in the even beat; the odd beat i takes both sums -- slot tick(i-1)
             * in the even lanes (S left it at i-2, B0 reads its log at i+1), slot tick(i) in the odd ones (S: i-1, B0: i+2) -- and
             * requests their table rows here; the pass itself runs behind the noise tracking, which covers the loads.  Both beats of
             * a pair lie in the steady range, so the even beat's flag (2, 1) is this beat's (3, 1): no flag the plan does not have. */
            constexpr bool LOG_PAIR = LOGP && STEADY;
            const bool logNow = LOG_PAIR && (i & 1); /* a constant of each steady copy */
            NsLogLanes lq = {};
            int lqSlot = 0;
            float lqSum = 0.0f;
            if constexpr (LOG_PAIR) {
                if (logNow) {
                    lqSlot = (tick_of(i - 3, onset) + 2 + (lane & 1)) & (kSlots - 1);
                    lqSum = L.frameEn[lqSlot];
                    ns_log_lanes_request(lq, lqSum, true);
                }
            } else if constexpr (LOG_N1) { /* the log-energy of the sum S left one beat ago, as FA takes it with LIGHT; B0 reads it two beats on */
                if (beat_flag<V, ns6plan::N1, 2, 1, STEADY>(i, onset, nfr)) {
                    const int e = (tick_of(i - 2, onset) + 2) & (kSlots - 1);
                    const float en = vad_frame_energy(L.frameEn[e]);
                    if (lane == 0) L.frameEnLog[e] = en;
                }
            }
            if (beat_flag<V, ns6plan::N1, 7 + kS1, 5, STEADY>(i, onset, nfr)) {
                const int t = tick_of(fg, onset);
                /* denEn1[0..2] (NoiseSup.c:595-598) = sums of denSigSE1 of ticks t-2, t-1, t */
                s.denEn0 = denRing[(t - 2) & (kDenRing - 1)];
                s.denEn1 = denRing[(t - 1) & (kDenRing - 1)];
                s.denEn2 = denRing[t & (kDenRing - 1)];
                const int nbNow = s.nbFrame[1]; /* has counted the frames tracked since; this frame's count is t - 4 */
                s.nbFrame[1] = t - 4;
                gain_fact_update(s, L.nzSum[fg & 1]);
                s.nbFrame[1] = nbNow;
                if (lane == 0) L.alfa[fg & 1] = s.alfaGF;
            }
            if (beat_flag<V, ns6plan::N1, 5 + kS1, 5, STEADY>(i, onset, nfr)) {
                const RecPsd &r = L.p1[f & (kP1Ring - 1)]; /* G1 reads it in place three beats later (kP1Ring) */
                RecN &o = L.rn[f & (kRnRing - 1)];
                ns_noise1<BIN64>(r.psd, o.P, o.noise, s, eps, lane);
            }
            if constexpr (LOG_PAIR) {
                if (logNow) {
                    const float en = ns_log_lanes_take(lq, lqSum, true);
                    if (lane < 2) L.frameEnLog[lqSlot] = en;
                }
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::N1, PAIRED>(niter, nfr, onset, beat);
        NS6_T_FLUSH(role, niter);
    } else if (role == 4) {
        /* ---- G1: stage-1 Wiener gains, mel, gain factorisation, IDCT, FIR ---- */
        NsConst C;
        load_back_const(C, a.tables, lane);
        NsRegs s;
        regs_init(s, C.eps);
        float lastIn = 0.0f; /* LIGHT: y[79] of the previous filtered frame (prevSamples, NoiseSup.c:908) */
        int onset = kNoOnset;
        FirPair3 fp = {}; /* FIRP: the lane's part of the merged filter pass's addresses (ns_core.h) */
        if constexpr (FIRP) {
            char *const lds = reinterpret_cast<char *>(&L);
            auto at = [&](const void *q) { return (int)(reinterpret_cast<const char *>(q) - lds); };
            const int j = (lane & 31) < 27 ? (lane & 31) : 26; /* lanes 27..31 of a half repeat lane 26 */
            fp.lds = lds;
            fp.x = (lane < 32 ? at(L.circ0) : at(L.circ1)) + (72 + 3 * j) * (int)sizeof(float);
            fp.tap = lane < 32 ? at(X->tap[0][0]) : at(X->tap[1][0]);
            fp.dst = (lane < 32 ? at(L.circ1) : at(L.ro[0].out)) + 3 * j * (int)sizeof(float);
        }
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if (!STEADY) onset_poll(onset, &L.onset);
            const int f = i - 8 - kS1;
            if constexpr (FIRP) {
                /* both 17-tap filters, from the windowed taps S left at the previous iteration: stage-0 frame i-4 (from tick 3, not 5:
                 * ticks 3 and 4 leave output that the first stage-1 window reads) in lanes 0..31 -> the stage-1 buffer's slot of its
                 * tick, which FA windows from the next iteration on; stage-1 frame i-12 in lanes 32..63 -> ro[].  Both frames have
                 * the same parity, so both tap records are that parity's.  Ahead of the gains of frame i-10, which depend on neither;
                 * in the fill only the low half is live, in the drain only the high half. */
                const int f0 = i - 4, f1 = i - 12;
                const bool live0 = beat_flag<V, ns6plan::G1, 4, 3, STEADY>(i, onset, nfr), live1 = beat_flag<V, ns6plan::G1, 12, 5, STEADY>(i, onset, nfr);
                if (live0 || live1) {
                    const int t0 = tick_of(f0, onset), slot = t0 & (kSlots1 - 1);
                    constexpr int kF = sizeof(float);
                    ns_fir_pair3(fp, window_base<kSlots>(t0) * kF, window_base<kSlots1>(tick_of(f1, onset)) * kF, (f0 & 1) * (int)sizeof(X->tap[0][0]),
                                 slot * kSlotLen * kF, (f1 & 1) * (int)sizeof(RecOut), slot < 3 ? kCirc1 * kF : 0, live0, live1, lane);
                }
            } else if constexpr (IDCTS) {
                /* the 17-tap filter of frame i-11, whose windowed taps S left at the previous iteration, ahead of the
                 * gains of frame i-9: the two do not depend on each other.  Also in the drain, where no gains are left. */
                const int ff = i - 11;
                if (beat_flag<V, ns6plan::G1, 11, 5, STEADY>(i, onset, nfr))
                    ns_fir_from_taps(X->tap[1][ff & 1], L.back[1].fir, L.circ1 + window_base<kSlots1>(tick_of(ff, onset)), L.ro[ff & 1].out, lane);
            }
            if (beat_flag<V, ns6plan::G1, 8 + kS1, 5, STEADY>(i, onset, nfr)) {
                const float *psd = L.p1[f & (kP1Ring - 1)].psd;
                const RecN &r = L.rn[f & (kRnRing - 1)];
                RecOut &o = L.ro[f & 1];
                const int t = tick_of(f, onset);
                const float alfa = L.alfa[f & 1];
                const float *w64 = BIN64 ? &L.w1hi[f & (kW1Ring - 1)] : nullptr; /* B0 left it two beats ago */
                if constexpr (IDCTS)
                    ns_gain1_products(psd, r.P, r.noise, alfa, L.back[1], s, C, X->prod[1][f & 1], lane, basisQ, w64);
                else if (DIFG1)
                    ns_gain1_dif(psd, r.P, r.noise, alfa, L.circ1 + window_base<kSlots1>(t), L.back[1], s, C, o.out, lane, L.idctT, lastIn);
                else
                    ns_gain1<BIN64>(psd, r.P, r.noise, alfa, L.circ1 + window_base<kSlots1>(t), L.back[1], s, C, o.out, lane, L.idctT, w64);
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::G1, PAIRED>(niter, nfr, onset, beat);
        NS6_T_FLUSH(role, niter);
    } else {
        /* ---- S: the lane-grouped scalar chains (helper_chains) ---- */
        uint32_t *out32 = reinterpret_cast<uint32_t *>(a.out + off);
        float *outf = a.out_f32 ? a.out_f32 + off : nullptr;
        float dcX = 0.0f, dcY = 0.0f; /* prevSamples, NoiseSup.c:908-909 */
        int firstOut = -1;
        int onset = kNoOnset;
        HelperIdct ids = {}; /* IDCTS: the lane's constants of helper_chains<.., IDS> */
        if constexpr (IDCTS) {
            static_assert(!IDCTS || !DIFG1, "the DC lanes read sdif");
            char *const lds = reinterpret_cast<char *>(&L);
            auto at = [&](const void *q) { return (int)(reinterpret_cast<const char *>(q) - lds); };
            const int g = lane >> 4, t = (lane - 1) & 15; /* lanes 1 + t and 17 + t, t = 0..8, have row t */
            const bool row = t <= 8 && g <= 1;
            constexpr int kProd = sizeof(X->prod[0][0]), kTap = sizeof(X->tap[0][0]), kRowB = kIdctStride * sizeof(float), kTapB = kIdsTapStride * sizeof(float);
            ids.lds = lds;
            ids.rowZeros = at(X->zeros) - kIdctRow * (int)sizeof(float);
            if (row) { /* stage 0: the records of parity p; stage 1: those of the other parity (FIRP: frame i-11, the same parity as i-3) */
                ids.src0 = (g == 0 ? at(X->prod[0][0]) : at(X->prod[1][FIRP ? 0 : 1])) + kRowB * t;
                ids.srcP = (g == 0 || FIRP) ? kProd : -kProd;
                ids.end = ids.rowZeros;
                ids.tap0 = (g == 0 ? at(X->tap[0][0]) : at(X->tap[1][FIRP ? 0 : 1])) + kTapB * t;
                ids.tapP = (g == 0 || FIRP) ? kTap : -kTap;
            } else {
                ids.src0 = g == 0 ? at(L.ssq) : (g == 1 ? at(L.rd[0].den) : (g == 2 ? at(L.sdif) : at(L.rn[0].noise)));
                ids.srcP = g == 1 ? (int)sizeof(RecDen) : 0;
                ids.srcQ = g == 3 ? (int)sizeof(RecN) : 0;
                ids.end = (g == 1 || g == 3) ? at(X->zeros) - 68 * (int)sizeof(float) : ids.src0;
            }
            ids.hann = a.tables->irWin[t];
            ids.m = g == 2 ? 0.9990234375f : 1.0f;
            ids.acc0 = (g == 0 && !row) ? 64.0f : 0.0f;
        }
        auto beat = [&](auto steady, int i) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            NS6_T_BEGIN;
            prio_by_remaining(i);
            if (!STEADY) onset_poll(onset, &L.onset);
            /* (1) VAD log-energy (NoiseSup.c:386-391) of the frame pushed at i-1 = tick tp ("current frame" of
             *     tick tp+2); (2) in-order sum of denSigSE1 of the frame B0 finished at i-1; (3) DC-offset
             *     filter, int16 cast, store of the frame G1 finished at i-1; (4) in-order sum of the noise
             *     spectrum N1 left at i-1 */
            const int fp = i - 1, fd = i - 3, fn = i - 6 - kS1, fo = i - DEPTH;
            const bool doVad = beat_flag<V, ns6plan::S, 1, 1, STEADY>(i, onset, nfr), doDen = beat_flag<V, ns6plan::S, 3, 3, STEADY>(i, onset, nfr),
                       doNz = beat_flag<V, ns6plan::S, 6 + kS1, 5, STEADY>(i, onset, nfr), produced = beat_flag<V, ns6plan::S, DEPTH, 5, STEADY>(i, onset, nfr);
            bool doIdct1 = false; /* IDCTS: the stage-1 IDCT sums of the frame G1 left its products of at i-1; the stage-0 sums go with doDen */
            if constexpr (IDCTS) doIdct1 = beat_flag<V, ns6plan::S, FIRP ? 11 : 10, 5, STEADY>(i, onset, nfr);
            const int tp = tick_of(fp, onset), td = tick_of(fd, onset);
            const float *denSrc = L.rd[(STEADY || (fd >= 0 && fd < nfr)) ? (fd & 1) : 0].den;
            const float *nzSrc = L.rn[fn & (kRnRing - 1)].noise;
            const bool haveOut = STEADY || (fo >= 0 && fo < nfr);
            float2 vOut = make_float2(0.0f, 0.0f);
            /* The prep of the chains, round 9: lanes 0..39 take samples 2l and 2l + 1 (lanes >= 40 repeat lane 39, stores included:
             * the same values to the same words), and every operand -- the frame's pair for the squares, G1's pair, its predecessor
             * and y2[79] for the differences and the next dcX -- is fetched in ONE batch of LDS reads before the first use.  It
             * used to be four round trips in sequence (64 + 16 lanes, twice).  The reads are unconditional: the slot indices are
             * masked, a record nobody has written yet holds garbage, and what is computed from it is stored under the flags only. */
            const int l2 = (lane < 40) ? lane : 39;
            float2 sqIn = *reinterpret_cast<const float2 *>(L.circ0 + (tp & (kSlots - 1)) * kSlotLen + 2 * l2);
            const float *difS = DIFG1 ? L.ro[fo & 1].out : L.sdif; /* DIFG1: G1 left the differences themselves */
            if constexpr (DIFG1) { /* no difference pass: the square half alone */
                asm volatile("" : "+v"(sqIn.x), "+v"(sqIn.y));
            } else {
                const float *y2 = L.ro[fo & 1].out;
                float2 yIn = *reinterpret_cast<const float2 *>(y2 + 2 * l2);
                float below = y2[(l2 > 0) ? 2 * l2 - 1 : 0], last = y2[79];
                asm volatile("" : "+v"(sqIn.x), "+v"(sqIn.y), "+v"(yIn.x), "+v"(yIn.y), "+v"(below), "+v"(last));
                if (produced) {
                    const float xm1 = (lane == 0) ? dcX : below; /* lane 0's predecessor: prevSamples */
                    *reinterpret_cast<float2 *>(L.sdif + 2 * l2) = make_float2(yIn.x - xm1, yIn.y - yIn.x);
                    dcX = last;
                }
            }
            if (doVad) *reinterpret_cast<float2 *>(L.ssq + 2 * l2) = make_float2(sqIn.x * sqIn.x, sqIn.y * sqIn.y);
            if (doVad || doDen || doNz || doIdct1 || produced) {
                wave_sync();
                float vadSum, denTotal, nzTotal, y = dcY;
                if constexpr (IDCTS) {
                    /* the taps are stored whatever the flags say: a record whose frame does not exist is read by nobody (FA's and
                     * G1's flags are these flags one beat on), and its slot's previous content was read at the previous iteration */
                    static_assert((((FIRP ? 11 : 10) - 3) & 1) == (FIRP ? 0 : 1), "S's two product records of a beat have opposite frame parities; FIRP: the same");
                    ids.p = fd & 1;
                    ids.q = fn & (kRnRing - 1);
                    helper_chains<kSChunks, false, true, true>(L.ssq, denSrc, difS, L.sout, L.szero, vadSum, denTotal, y, lane, nullptr, nullptr,
                                                               nullptr, nzSrc, &nzTotal, &ids);
                } else
                    helper_chains<kSChunks, false, true>(L.ssq, denSrc, difS, L.sout, L.szero, vadSum, denTotal, y, lane, nullptr, nullptr,
                                                         nullptr, nzSrc, &nzTotal);
                if (doVad) {
                    const float en = (LIGHT || LOG_N1) ? vadSum : vad_frame_energy(vadSum); /* FA (LIGHT) or N1 takes the log one beat later */
                    if (lane == 0) L.frameEn[(tp + 2) & (kSlots - 1)] = en;
                }
                if (doDen && lane == 0) denRing[td & (kDenRing - 1)] = denTotal;
                if (doNz && lane == 0) L.nzSum[fn & 1] = nzTotal;
                if (produced) {
                    vOut = dc_verify_take(difS, L.sout, dcY, y, lane); /* check + output in one batch of reads */
                    dcY = y;
                    if (!STEADY && firstOut < 0) firstOut = fo; /* set before S goes steady (RolePlan::settle) */
                }
            }
            if (haveOut) {
                if (lane < 40) {
                    uint32_t packed = 0u;
                    if (produced) {
                        packed = (uint32_t)cast_i16(vOut.x) | ((uint32_t)cast_i16(vOut.y) << 16);
                        if (outf) *reinterpret_cast<float2 *>(outf + (long long)fo * SEA_HOP + 2 * lane) = vOut;
                    }
                    (out32 + (long long)fo * 40)[lane] = packed;
                }
                if constexpr (FD) { /* the speech flags B0 left for this frame seven beats ago: the plan's fifth flag of S */
                    if (beat_flag<V, ns6plan::S, DEPTH, 5, STEADY>(i, onset, nfr) && lane == 0 && a.flags_out)
                        a.flags_out[off / 8 + 10 * (long long)fo] = (unsigned char)L.fdFlags[tick_of(fo, onset) & (kSlots - 1)];
                }
                wave_sync();
            }
            NS6_T_MID;
            block_sync();
            NS6_T_END;
        };
        run_beats<STEADY_LOOP, V, ns6plan::S, PAIRED>(niter, nfr, onset, beat);
        NS6_T_FLUSH(role, niter);
        if (a.first_out && lane == 0) a.first_out[u] = firstOut;
    }
}

} // namespace p6

/* launched for at most two utterances per CU (capi.hip::ns_pick_form): twelve waves per CU, three per SIMD, so the
 * register allocation could use up to 168 VGPRs.  The plain form stays compiled for 80 (measured: 1644 against 1679 ns
 * per frame with the looser bound, which only changes the schedule); the _fd form takes the looser bound, which
 * removes its 7 spilled registers (91 VGPRs).  Today the plain form takes 68 VGPRs, nothing spilled, and the _fd form 93 with 6 SGPRs
 * spilled to lanes (82 and none before round 9's batches), no scratch.
 * STEADY_LOOP: round 7 left it off here -- with the steady copies alone this form ran 2.1 % (256 utterances) and 2.6 % (768) slower, its
 * period is B0's beat, the one role they did not shorten; on in the dense form (-2.9 %) and in the _fd form (-1.9 %),
 * profiles/ns6_steady_loop.txt.  Round 12: on, with the beats paired (PAIRED), in all three: 256 utterances 1.416 -> 1.321 ms, 768
 * 1.566 -> 1.434, the _fd kernel on 512 2.488 -> 2.403 (profiles/ns6_transform_chain.txt).  The plain form now takes its whole bound
 * of 80 VGPRs and the _fd form 95 with 14 SGPRs spilled to lanes; nothing in scratch. */
__global__ __launch_bounds__(384, 6) void ns_denoise_pipe6_kernel(NsBatchArgs a)
{
    __shared__ p6::Pipe6Lds L;
    p6::ns_pipe6_body<false, true, true, true, false, false, false, true>(a, L);
}
/* The same body compiled for SEVEN waves per SIMD (72 VGPRs, two SGPRs spilled to lanes, no scratch; since round 8 with REDEAL and its own
 * wave -> role map): the form for three or four utterances per CU (round 4).  With 80 VGPRs a SIMD holds six waves, four six-wave workgroups are exactly the 24 a CU then holds -- and the
 * dispatcher, which deals the six waves of a workgroup 2 / 2 / 1 / 1 over the SIMDs, does not find room for the fourth: it
 * waited for one of the first three to end (configs[1]: 3.20 ms, which rounds 1-3 read as "the six-wave form loses at four
 * per CU").  One wave slot of slack per SIMD lets all four co-reside: 2.14 ms without priorities, **2.00-2.05 ms** with the
 * issue priority by remaining frames and the wave -> role map below, against 2.08-2.13 for the four-wave form
 * (profiles/r04_ns_six_wave_dense.txt). */
#ifdef SEA_NS6_TIMING
__device__ unsigned g_ns6_wg[16384 * 4]; /* dense form, per workgroup: start, end (constant 100 MHz counter), HW_ID, XCC_ID (tools/ns6_residency.py) */
#endif
__global__ __launch_bounds__(384, 7) void ns_denoise_pipe6_dense_kernel(NsBatchArgs a)
{
    __shared__ p6::Pipe6LdsIdct L;
#ifdef SEA_NS6_TIMING
    if (threadIdx.x == 0 && blockIdx.x < 16384) {
        g_ns6_wg[4 * blockIdx.x] = (unsigned)wall_clock64();
        g_ns6_wg[4 * blockIdx.x + 2] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
        g_ns6_wg[4 * blockIdx.x + 3] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);
    }
#endif
    p6::ns_pipe6_body<false, false, false, true, true, true, true, true, true, true>(a, L.base, &L.x);
#ifdef SEA_NS6_TIMING
    if (threadIdx.x == 0 && blockIdx.x < 16384) g_ns6_wg[4 * blockIdx.x + 1] = (unsigned)wall_clock64();
#endif
}
__global__ __launch_bounds__(384, 2) void ns_denoise_pipe6_fd_kernel(NsBatchArgs a)
{
    __shared__ p6::Pipe6Lds L;
    p6::ns_pipe6_body<true, true, true, true, false, false, false, true>(a, L);
}

} // namespace sea

#ifdef SEA_NS6_TIMING
extern "C" int sea_debug_ns6_timing(unsigned long long *out16)
{
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(sea::p6::g_ns6_timing), 16 * sizeof(unsigned long long));
}
extern "C" int sea_debug_ns6_wg(unsigned *out, int n_wg)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sea::g_ns6_wg), (size_t)n_wg * 4 * sizeof(unsigned));
}
#endif
