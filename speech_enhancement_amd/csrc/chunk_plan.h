/*
 * chunk_plan.h -- how the entry points that take a list of utterances from host memory cut it into chunks of whole utterances
 * that fit the device, what sizes their buffers, and how an utterance is packed.  Integer arithmetic
 * only, no HIP: tests/chunk_plan_driver.cpp runs it on a CPU.
 *
 * The list is taken in order, greedily: a chunk grows while its footprint stays within the budget; an utterance that exceeds
 * the budget alone forms a chunk of its own, and hipMalloc reports what does not fit.  A caller describes an utterance by K
 * quantities (padded samples, rows, tiles, ..., bytes); a chunk's are their sums, and its footprint is a function of those sums
 * and of its number of utterances.  The buffers are sized once, by the largest sum of every quantity over the chunks.
 */
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sea_capi {

inline long long align8(long long v) { return (v + 7) & ~7LL; }
inline long long tiles_of(long long n, int per) { return (n + per - 1) / per; }

/* the budget of a chunk: env_text MiB where a SEA_*_SCRATCH_MB variable is set, else 60 % of the free bytes and of those
 * the caller holds and will reuse */
inline long long budget_of(size_t free_bytes, size_t held_bytes, const char *env_text)
{
    return env_text ? atoll(env_text) * (1LL << 20) : (long long)((free_bytes + held_bytes) / 10 * 6);
}

/* an utterance's L elements, then zeros up to a multiple of 8; returns the elements written */
template <class T>
long long pack_padded(T *dst, const T *src, long long L)
{
    const long long Lp = align8(L);
    if (L > 0) memcpy(dst, src, (size_t)L * sizeof(T));
    if (Lp > L) memset(dst + L, 0, (size_t)(Lp - L) * sizeof(T));
    return Lp;
}

template <size_t K>
using Totals = std::array<long long, K>;

template <size_t K>
struct ChunkPlan {
    std::vector<int> cuts;       /* the first utterance of every chunk, then n */
    std::vector<Totals<K>> sum;  /* every chunk's totals */
    Totals<K> max{};             /* their elementwise maximum */
    int max_n = 0;               /* utterances in the longest chunk */
    int chunks() const { return (int)cuts.size() - 1; }
};

/* of (u): the Totals<K> of utterance u; bytes (totals, n_in_chunk): the footprint of a chunk.  n = 0 gives the cuts {0, 0}. */
template <size_t K, class Of, class Bytes>
ChunkPlan<K> plan_chunks(int n, long long budget, Of of, Bytes bytes)
{
    ChunkPlan<K> p;
    p.cuts.push_back(0);
    Totals<K> run{};
    auto close = [&](int end) {
        p.sum.push_back(run);
        for (size_t i = 0; i < K; ++i) p.max[i] = std::max(p.max[i], run[i]);
        p.max_n = std::max(p.max_n, end - p.cuts.back());
        p.cuts.push_back(end);
    };
    for (int u = 0; u < n; ++u) {
        const Totals<K> q = of(u);
        Totals<K> with = run;
        for (size_t i = 0; i < K; ++i) with[i] += q[i];
        if (u > p.cuts.back() && bytes(with, u - p.cuts.back() + 1) > budget) {
            close(u);
            with = q;
        }
        run = with;
    }
    close(n);
    return p;
}

/* the additive footprint: the last quantity is the utterance's bytes, a chunk's footprint their sum */
template <size_t K, class Of>
ChunkPlan<K> plan_chunks(int n, long long budget, Of of)
{
    return plan_chunks<K>(n, budget, of, [](const Totals<K> &c, int) { return c[K - 1]; });
}

} // namespace sea_capi
