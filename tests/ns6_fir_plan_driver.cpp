/* Stand-alone driver of csrc/ns6_beat_plan.h for tests/test_ns6_fir_plan_cpu.py (no HIP, no GPU): the variant of the dense kernel in
 * which G1 runs both 17-tap filters as one pass on its two lane halves, kVariantDenseFirPair, which has a table and a depth of its own.
 * stdout:
 *     "variant <value> <kFirPair> <depth_of(value)> <kDepth>", then per role
 *     "flags <role> <ahead> <settle> d:k d:k ..."        the flags that apply in the new variant
 *     "ends <role> <steady_lead> <steady_tail>"
 * then per existing variant v (plain, dense, fd, re-dealt, bin 64, IDCT sums in the helper wave) and role
 *     "old <v> <role> <depth_of(v)> <steady_lead> <steady_tail> <steady_begin(v, role, 7)> <steady_end(v, role, 50)> d:k d:k ..."
 * then per case of the sweep (onset -1 = the gate never opens, 0 .. max_onset; nfr 0 .. max_nfr)
 *     "range <role> <onset> <nfr> <steady_begin> <steady_end>"
 * argv: max_onset max_nfr */
#include <stdio.h>
#include <stdlib.h>

#include "ns6_beat_plan.h"

namespace plan = sea::ns6plan;

constexpr unsigned kV = plan::kVariantDenseFirPair;
/* what the kernel folds at compile time */
static_assert(kV == (plan::kVariantDenseIdct | plan::kFirPair) && (kV & (plan::kFd | plan::kLight | plan::kDifg1)) == 0u, "the dense body plus one bit");
static_assert((plan::kFirPair & (plan::kFd | plan::kLight | plan::kDifg1 | plan::kRedeal | plan::kBin64 | plan::kIdctS)) == 0u && plan::kFirPair != plan::kAlways,
              "a bit of its own");
static_assert(plan::depth_of(kV) == 13 && plan::depth_of(plan::kVariantDenseIdct) == 12 && plan::depth_of(plan::kVariantDenseBin64) == plan::kDepth && plan::kDepth == 9,
              "its own depth");
static_assert(plan::has_flag(kV, plan::G1, 4, 3) && plan::has_flag(kV, plan::G1, 10, 5) && plan::has_flag(kV, plan::G1, 12, 5) && !plan::has_flag(kV, plan::G1, 11, 5) &&
                  !plan::has_flag(kV, plan::G1, 9, 5),
              "G1's three jobs");
static_assert(plan::has_flag(kV, plan::FA, 5, 5) && !plan::has_flag(kV, plan::FA, 4, 3) && !plan::has_flag(kV, plan::FA, 4, 5), "FA filters no more");
static_assert(plan::has_flag(kV, plan::S, 11, 5) && plan::has_flag(kV, plan::S, 13, 5) && !plan::has_flag(kV, plan::S, 12, 5), "S's stage-1 sums and output");
static_assert(plan::has_flag(plan::kVariantDenseIdct, plan::FA, 4, 3) && plan::has_flag(plan::kVariantDenseIdct, plan::G1, 11, 5) &&
                  !plan::has_flag(plan::kVariantDenseIdct, plan::G1, 4, 3) && !plan::has_flag(plan::kVariantPlain, plan::S, 13, 5) &&
                  !plan::has_flag(plan::kVariantFd, plan::G1, 12, 5) && plan::has_flag(plan::kVariantDenseBin64, plan::G1, 8, 5),
              "the other variants keep their table");
static_assert(plan::steady_begin(kV, plan::S, 3) == 21 && plan::steady_end(kV, plan::G1, 10) == 14 && plan::steady_begin(kV, plan::FA, plan::kNoOnset) == plan::kNoOnset,
              "constexpr");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int max_onset = atoi(argv[1]), max_nfr = atoi(argv[2]);
    printf("variant %u %u %d %d\n", kV, plan::kFirPair, plan::depth_of(kV), plan::kDepth);
    for (int role = 0; role < plan::kRoles; ++role) {
        const plan::RolePlan &p = plan::plan_of(kV, role);
        if (p.n > plan::kMaxFlags) return 4;
        if (&p != &plan::kPlanFirPair[role]) return 6;
        printf("flags %d %d %d", role, p.ahead, p.settle);
        for (int j = 0; j < p.n; ++j)
            if (plan::flag_applies(p.f[j], kV)) {
                printf(" %d:%d", p.f[j].d, p.f[j].k);
                if (!plan::has_flag(kV, role, p.f[j].d, p.f[j].k)) return 3;
            }
        printf("\nends %d %d %d\n", role, plan::steady_lead(kV, role), plan::steady_tail(kV, role));
    }
    const unsigned olds[6] = {plan::kVariantPlain, plan::kVariantDense, plan::kVariantFd, plan::kVariantDenseRedeal, plan::kVariantDenseBin64, plan::kVariantDenseIdct};
    for (unsigned v : olds)
        for (int role = 0; role < plan::kRoles; ++role) {
            const plan::RolePlan &p = plan::plan_of(v, role);
            if (&p != ((v & plan::kIdctS) ? &plan::kPlanIdct[role] : &plan::kPlan[role])) return 5;
            printf("old %u %d %d %d %d %d %d", v, role, plan::depth_of(v), plan::steady_lead(v, role), plan::steady_tail(v, role),
                   plan::steady_begin(v, role, 7), plan::steady_end(v, role, 50));
            for (int j = 0; j < p.n; ++j)
                if (plan::flag_applies(p.f[j], v)) printf(" %d:%d", p.f[j].d, p.f[j].k);
            printf("\n");
        }
    for (int role = 0; role < plan::kRoles; ++role)
        for (int onset = -1; onset <= max_onset; ++onset)
            for (int nfr = 0; nfr <= max_nfr; ++nfr) {
                const int on = onset < 0 ? plan::kNoOnset : onset;
                printf("range %d %d %d %d %d\n", role, onset, nfr, plan::steady_begin(kV, role, on), plan::steady_end(kV, role, nfr));
            }
    return 0;
}
