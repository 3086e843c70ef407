/* Stand-alone driver of csrc/slice_plan.h for tests/test_slice_plan_cpu.py (no HIP, no GPU).
 * Without an argument, the plan:
 *   stdin, one case per line:   hop want n len_0 .. len_n-1
 *   stdout per case:            "case", the plan's members one per line, then per slice and offset convention
 *                               "rows <k> <abs|rel> offsets.. | lengths.. | bytes_prefix..", then "end".
 * With the argument "order", RowOrder on that plan's K slices:
 *   stdin, one case per line:   hop want n len_0 .. len_n-1, then the K slices in the order they arrive, then per slice in plan
 *                               order the rows each of its nact[k] pieces emitted
 *   stdout per case:            "case", per arrival "arrive <k>" followed by one "cut <k>" for every slice cut on that arrival,
 *                               then per slice "start <k> start[k][0] .. start[k][nact[k]-1]" in the order the slices were cut,
 *                               then "pos pos[0] .. pos[n-1]" and "end".
 * A slice's counts reach the array RowOrder reads only when the slice arrives, as a download brings them; the start rows are
 * printed after the last arrival through the pointers the cut callback received, as the copy tasks read them. */
#include <stdio.h>
#include <string.h>

#include <utility>

#include <vector>

#include "slice_plan.h"

template <class V>
static void line(const char *name, const V &v)
{
    printf("%s", name);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static int order_cases()
{
    long long hop;
    int want, n;
    while (scanf("%lld %d %d", &hop, &want, &n) == 3) {
        std::vector<long> lengths(n);
        for (auto &l : lengths)
            if (scanf("%ld", &l) != 1) return 2;
        sea_capi::SlicePlan p;
        sea_capi::slice_plan(p, lengths.data(), n, hop, want);
        std::vector<int> arrival(p.K), emitted(p.mbase[p.K] / 2), counts(p.mbase[p.K] / 2, -1000000); /* the callers' size */
        for (auto &a : arrival)
            if (scanf("%d", &a) != 1 || a < 0 || a >= p.K) return 2;
        for (auto &c : emitted)
            if (scanf("%d", &c) != 1) return 2;
        printf("case\n");
        sea_capi::RowOrder order(p.K, n);
        std::vector<std::pair<int, const long long *>> cuts;
        for (int a : arrival) {
            printf("arrive %d\n", a);
            std::copy(emitted.begin() + p.mbase[a] / 2, emitted.begin() + p.mbase[a + 1] / 2, counts.begin() + p.mbase[a] / 2);
            order.arrive(p, a, counts.data(), [&](int k, const long long *st) {
                printf("cut %d\n", k);
                cuts.emplace_back(k, st);
            });
        }
        for (const auto &c : cuts) {
            printf("start %d", c.first);
            for (int j = 0; j < p.nact[c.first]; ++j) printf(" %lld", c.second[j]);
            printf("\n");
        }
        line("pos", order.pos);
        printf("end\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return strcmp(argv[1], "order") ? 2 : order_cases();
    long long hop;
    int want, n;
    while (scanf("%lld %d %d", &hop, &want, &n) == 3) {
        std::vector<long> lengths(n);
        for (auto &l : lengths)
            if (scanf("%ld", &l) != 1) return 2;
        sea_capi::SlicePlan p;
        sea_capi::slice_plan(p, lengths.data(), n, hop, want);
        printf("case\n");
        printf("K %d\ntotal_fr %lld\nmax_fr %lld\n", p.K, p.total_fr, p.max_fr);
        line("idx", p.idx);
        line("inv", p.inv);
        line("nfr", p.nfr);
        line("B", p.B);
        line("nact", p.nact);
        line("foff", p.foff);
        line("mbase", p.mbase);
        for (int k = 0; k < p.K; ++k)
            for (int absolute = 1; absolute >= 0; --absolute) {
                const int na = p.nact[k];
                std::vector<long long> rows(2 * na, -1), bytes(na + 1, -1); /* exactly the sizes the callers allocate */
                sea_capi::slice_rows(p, k, hop, absolute != 0, rows.data(), bytes.data());
                printf("rows %d %s", k, absolute ? "abs" : "rel");
                for (int j = 0; j < 2 * na; ++j) printf("%s %lld", j == na ? " |" : "", rows[j]);
                printf(" |");
                for (auto b : bytes) printf(" %lld", b);
                printf("\n");
                std::vector<long long> again(2 * na, -1);
                sea_capi::slice_rows(p, k, hop, absolute != 0, again.data(), nullptr); /* the prefix is optional */
                if (again != rows) return 3;
            }
        printf("end\n");
    }
    return 0;
}
