/*
 * recording_plan.h -- how a long recording is cut into chunks for BufferDenoise
 * (function/20141106_speech_enhancement/aurora_speech_enhancement/aurora_speech_enhancement.cpp:25-80) and where its stitched
 * result lies in the chunks' outputs.  DESIGN.md 5.20 is the contract.  Integer arithmetic only, no HIP:
 * tests/recording_plan_driver.cpp runs it on a CPU.
 *
 * S samples, chunk length B (a multiple of 80, at least 320), O = 320, T = S / B, R = S % B.  The chunks, in order:
 *   T == 0   one, x[0 : S]
 *   else     x[0 : B];  x[iB - O : iB + B] for i = 1 .. T - 1;  x[TB - O : TB + R]  (it exists when R == 0 too)
 * Every chunk starts on a whole frame and on a multiple of 8.  In the LAYOUT the chunks lie one after the other, each padded
 * to 8 samples, so that a batch kernel which addresses a chunk's input and output by one offset finds both there: S + O T
 * samples and the last chunk's pad.  Neighbouring chunks share O input samples; the layout holds them once per chunk.
 *
 * The stitch: des[t] = out[off[i] + t + O + (i > 0 ? O : 0) - i B] with i = (t + O) / B for 0 <= t < S - O, and 0 for the
 * last O samples -- `out` being the chunks' etsi_denoise outputs in the layout.
 */
#pragma once

namespace sea_capi {

constexpr long long kRecOverlap = 320; /* etsi_offset_points: NoiseSup's latency, the overlap of two chunks */

inline bool rec_chunk_valid(long long B) { return B >= kRecOverlap && B % 80 == 0; }

/* chunks of a recording of S >= kRecOverlap samples */
inline long long rec_chunk_count(long long S, long long B) { return S / B == 0 ? 1 : S / B + 1; }

/* chunk i: its first sample in the recording, its length, its offset in the layout */
inline void rec_chunk(long long S, long long B, long long i, long long *src, long long *len, long long *off)
{
    const long long T = S / B, O = kRecOverlap;
    if (T == 0) {
        *src = 0, *len = S, *off = 0;
        return;
    }
    *src = i == 0 ? 0 : i * B - O;
    *len = i == 0 ? B : (i < T ? B + O : S % B + O);
    *off = i == 0 ? 0 : B + (i - 1) * (B + O); /* every chunk before the last is a multiple of 8 long */
}

/* samples of the layout, the last chunk's pad included */
inline long long rec_layout_samples(long long S, long long B)
{
    long long src, len, off;
    rec_chunk(S, B, rec_chunk_count(S, B) - 1, &src, &len, &off);
    return off + ((len + 7) & ~7LL);
}

/* where des[t] lies in the layout; -1: des[t] is 0 */
inline long long rec_stitch_index(long long S, long long B, long long t)
{
    const long long O = kRecOverlap;
    if (t < 0 || t >= S - O) return -1;
    const long long i = (t + O) / B;
    long long src, len, off;
    rec_chunk(S, B, i, &src, &len, &off);
    return off + t + O + (i > 0 ? O : 0) - i * B;
}

} // namespace sea_capi
