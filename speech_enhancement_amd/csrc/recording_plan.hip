/*
 * recording_plan.hip -- the C ABI of recording_plan.h: the chunk table of a long recording and its stitch map, for callers
 * that run BufferDenoise's chunks themselves (as utterances of sea_denoise_utterances or of a PackedBatch).  Host arithmetic
 * only; no device is touched.
 */
#include "capi_internal.h"
#include "recording_plan.h"

using namespace sea_capi;

extern "C" {

long long sea_recording_plan(long samples, long chunk, long long *chunk_src, long long *chunk_len, long long *chunk_off,
                             long long max_chunks)
{
    if (!rec_chunk_valid(chunk)) {
        fail("sea_recording_plan: chunk %ld (a multiple of 80, at least %lld)", chunk, kRecOverlap);
        return -1;
    }
    if (samples < 0) {
        fail("sea_recording_plan: %ld samples", samples);
        return -1;
    }
    if (samples < kRecOverlap) return 0; /* shorter than the latency: the tool skips such a recording */
    const long long n = rec_chunk_count(samples, chunk);
    for (long long i = 0; i < n && i < max_chunks; ++i) {
        long long src, len, off;
        rec_chunk(samples, chunk, i, &src, &len, &off);
        if (chunk_src) chunk_src[i] = src;
        if (chunk_len) chunk_len[i] = len;
        if (chunk_off) chunk_off[i] = off;
    }
    return n;
}

long long sea_recording_layout_samples(long samples, long chunk)
{
    if (!rec_chunk_valid(chunk) || samples < kRecOverlap) return 0;
    return rec_layout_samples(samples, chunk);
}

int sea_recording_stitch_map(long samples, long chunk, long first, long count, long long *index)
{
    if (!rec_chunk_valid(chunk)) return fail("sea_recording_stitch_map: chunk %ld (a multiple of 80, at least %lld)", chunk, kRecOverlap);
    if (samples < kRecOverlap || first < 0 || count < 0 || first > samples - count)
        return fail("sea_recording_stitch_map: samples [%ld, %ld + %ld) of a recording of %ld", first, first, count, samples);
    if (count > 0 && !index) return fail("sea_recording_stitch_map: index is NULL");
    for (long k = 0; k < count; ++k) index[k] = rec_stitch_index(samples, chunk, first + k);
    return 0;
}

} // extern "C"
