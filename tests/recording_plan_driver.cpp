// Test driver of speech_enhancement_amd/csrc/recording_plan.h (tests/test_recordings_cpu.py builds it with the sanitizers on):
// stdin holds lines "S B"; per line it prints "case <n_chunks> <layout>", the chunks as "src len off" and one line with
// rec_stitch_index of t = -1 .. S.
#include <cstdio>

#include "recording_plan.h"

int main()
{
    long long S, B;
    while (std::scanf("%lld %lld", &S, &B) == 2) {
        if (!sea_capi::rec_chunk_valid(B) || S < sea_capi::kRecOverlap) {
            std::printf("case -1 0\n\n");
            continue;
        }
        const long long n = sea_capi::rec_chunk_count(S, B);
        std::printf("case %lld %lld\n", n, sea_capi::rec_layout_samples(S, B));
        for (long long i = 0; i < n; ++i) {
            long long src, len, off;
            sea_capi::rec_chunk(S, B, i, &src, &len, &off);
            std::printf("%lld %lld %lld\n", src, len, off);
        }
        for (long long t = -1; t <= S; ++t) std::printf("%lld ", sea_capi::rec_stitch_index(S, B, t));
        std::printf("\n");
    }
    return 0;
}
