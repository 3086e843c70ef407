/* Stand-alone driver of csrc/chunk_plan.h for tests/test_chunk_plan_cpu.py (no HIP, no GPU).
 *   stdin, one case per line:
 *     add <budget> <n> a_0 b_0 .. a_n-1 b_n-1   the additive footprint: utterance u has the quantity a_u and b_u bytes
 *     quad <budget> <A> <B> <n> s_0 .. s_n-1    a footprint of the chunk's totals: A * (sum of s) + B * n_in_chunk^2
 *     budget <text or -> <free> <held>          budget_of; "-" stands for no override
 *     pack <L>                                  pack_padded of 1 .. L into a buffer of align8 (L) + 8 sentinels, as int16 and float
 *   stdout per case:
 *     add, quad:  "cuts ..", "sum .." (every chunk's totals, one after the other), "max ..", "max_n k", "chunks c", then "end"
 *     budget:     "budget v"
 *     pack:       "pack16 <returned> buffer..", "pack32 <returned> buffer.."
 */
#include <stdio.h>
#include <string.h>

#include <vector>

#include "chunk_plan.h"

using namespace sea_capi;

template <size_t K>
static void print_plan(const ChunkPlan<K> &p)
{
    printf("cuts");
    for (int c : p.cuts) printf(" %d", c);
    printf("\nsum");
    for (const auto &t : p.sum)
        for (long long v : t) printf(" %lld", v);
    printf("\nmax");
    for (long long v : p.max) printf(" %lld", v);
    printf("\nmax_n %d\nchunks %d\nend\n", p.max_n, p.chunks());
}

template <class T>
static void pack_case(const char *name, long long L)
{
    const T sentinel = (T)0x7e7e;
    std::vector<T> src((size_t)L), dst((size_t)align8(L) + 8, sentinel); /* L = 0: src.data () may be null, and is not read */
    for (long long i = 0; i < L; ++i) src[(size_t)i] = (T)(i + 1);
    const long long got = pack_padded(dst.data(), L ? src.data() : (const T *)nullptr, L);
    printf("%s %lld", name, got);
    for (T v : dst) printf(" %lld", (long long)v);
    printf("\n");
}

int main()
{
    char what[16], text[64];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "add")) {
            long long budget;
            int n;
            if (scanf("%lld %d", &budget, &n) != 2) return 2;
            std::vector<long long> v(2 * (size_t)n);
            for (auto &x : v)
                if (scanf("%lld", &x) != 1) return 2;
            print_plan(plan_chunks<2>(n, budget, [&](int u) -> Totals<2> { return {v[2 * (size_t)u], v[2 * (size_t)u + 1]}; }));
        } else if (!strcmp(what, "quad")) {
            long long budget, A, B;
            int n;
            if (scanf("%lld %lld %lld %d", &budget, &A, &B, &n) != 4) return 2;
            std::vector<long long> v((size_t)n);
            for (auto &x : v)
                if (scanf("%lld", &x) != 1) return 2;
            print_plan(plan_chunks<1>(
                n, budget, [&](int u) -> Totals<1> { return {v[(size_t)u]}; },
                [&](const Totals<1> &c, int in_chunk) { return A * c[0] + B * in_chunk * in_chunk; }));
        } else if (!strcmp(what, "budget")) {
            unsigned long long free_b, held;
            if (scanf("%63s %llu %llu", text, &free_b, &held) != 3) return 2;
            printf("budget %lld\n", budget_of((size_t)free_b, (size_t)held, strcmp(text, "-") ? text : nullptr));
        } else if (!strcmp(what, "pack")) {
            long long L;
            if (scanf("%lld", &L) != 1 || L < 0) return 2;
            pack_case<short>("pack16", L);
            pack_case<float>("pack32", L);
        } else {
            return 2;
        }
    }
    return 0;
}
