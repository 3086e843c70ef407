/* Stand-alone driver of csrc/ns6_beat_plan.h for tests/test_ns6_bin64_plan_cpu.py (no HIP, no GPU): the variant of the dense kernel in
 * which B0's second component also carries stage-1 bin 64 of frame i-6, kVariantDenseBin64, beside the variant it grew from,
 * kVariantDenseRedeal.  stdout: "variant <value> <kRedeal> <kBin64>", then per role
 *     "flags <role> <ahead> <settle> d:k d:k ..."        the flags that apply in the new variant
 *     "ends <role> <steady_lead> <steady_tail>"
 * then per case of the sweep (onset -1 = the gate never opens, 0 .. max_onset; nfr 0 .. max_nfr)
 *     "range <role> <onset> <nfr> <steady_begin> <steady_end> <steady_begin of kVariantDenseRedeal> <steady_end of it>"
 * argv: max_onset max_nfr */
#include <stdio.h>
#include <stdlib.h>

#include "ns6_beat_plan.h"

namespace plan = sea::ns6plan;

constexpr unsigned kV = plan::kVariantDenseBin64, kOld = plan::kVariantDenseRedeal;
/* what the kernel folds at compile time */
static_assert(kV == (plan::kRedeal | plan::kBin64) && (kV & (plan::kFd | plan::kLight | plan::kDifg1)) == 0u, "the re-dealt dense body plus one bit");
static_assert((plan::kBin64 & (plan::kFd | plan::kLight | plan::kDifg1 | plan::kRedeal)) == 0u && plan::kBin64 != plan::kAlways, "a bit of its own");
static_assert(plan::has_flag(kV, plan::B0, 6, 5) && plan::has_flag(kV, plan::B0, 2, 3), "the new flag beside B0's own");
static_assert(!plan::has_flag(kOld, plan::B0, 6, 5) && !plan::has_flag(plan::kVariantDense, plan::B0, 6, 5) &&
                  !plan::has_flag(plan::kVariantPlain, plan::B0, 6, 5) && !plan::has_flag(plan::kVariantFd, plan::B0, 6, 5),
              "it belongs to no other kernel");
static_assert(plan::steady_begin(kV, plan::B0, 3) == 13 && plan::steady_end(kV, plan::B0, 10) == 12 && plan::steady_begin(kOld, plan::B0, 3) == 7,
              "constexpr");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int max_onset = atoi(argv[1]), max_nfr = atoi(argv[2]);
    printf("variant %u %u %u\n", kV, plan::kRedeal, plan::kBin64);
    for (int role = 0; role < plan::kRoles; ++role) {
        const plan::RolePlan &p = plan::kPlan[role];
        if (p.n > plan::kMaxFlags) return 4;
        printf("flags %d %d %d", role, p.ahead, p.settle);
        for (int j = 0; j < p.n; ++j)
            if (plan::flag_applies(p.f[j], kV)) {
                printf(" %d:%d", p.f[j].d, p.f[j].k);
                if (!plan::has_flag(kV, role, p.f[j].d, p.f[j].k)) return 3;
            }
        printf("\nends %d %d %d\n", role, plan::steady_lead(kV, role), plan::steady_tail(kV, role));
    }
    for (int role = 0; role < plan::kRoles; ++role)
        for (int onset = -1; onset <= max_onset; ++onset)
            for (int nfr = 0; nfr <= max_nfr; ++nfr) {
                const int on = onset < 0 ? plan::kNoOnset : onset;
                printf("range %d %d %d %d %d %d %d\n", role, onset, nfr, plan::steady_begin(kV, role, on), plan::steady_end(kV, role, nfr),
                       plan::steady_begin(kOld, role, on), plan::steady_end(kOld, role, nfr));
            }
    return 0;
}
