/* Stand-alone driver of csrc/slice_plan.h for tests/test_slice_plan_cpu.py (no HIP, no GPU).
 * stdin, one case per line:   hop want n len_0 .. len_n-1
 * stdout per case:            "case", the plan's members one per line, then per slice and offset convention
 *                             "rows <k> <abs|rel> offsets.. | lengths.. | bytes_prefix..", then "end". */
#include <stdio.h>

#include <vector>

#include "slice_plan.h"

template <class V>
static void line(const char *name, const V &v)
{
    printf("%s", name);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main()
{
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
