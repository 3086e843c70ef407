/* Stand-alone driver of csrc/ns6_beat_plan.h for tests/test_ns6_redeal_plan_cpu.py (no HIP, no GPU): the variant of the re-dealt dense
 * kernel, kVariantDenseRedeal.  stdout: "variant <value> <kRedeal>", then per role
 *     "flags <role> <ahead> <settle> d:k d:k ..."        the flags that apply in that variant
 *     "ends <role> <steady_lead> <steady_tail>"
 * then per case of the sweep (onset -1 = the gate never opens, 0 .. max_onset; nfr 0 .. max_nfr)
 *     "range <role> <onset> <nfr> <steady_begin> <steady_end>"
 * argv: max_onset max_nfr */
#include <stdio.h>
#include <stdlib.h>

#include "ns6_beat_plan.h"

namespace plan = sea::ns6plan;

constexpr unsigned kV = plan::kVariantDenseRedeal;
/* what the kernel folds at compile time */
static_assert(kV == plan::kRedeal && (kV & (plan::kFd | plan::kLight | plan::kDifg1)) == 0u, "the re-deal is the dense body plus one bit");
static_assert(plan::has_flag(kV, plan::FA, 3, 3) && plan::has_flag(kV, plan::N1, 2, 1), "the two new flags");
static_assert(!plan::has_flag(plan::kVariantDense, plan::FA, 3, 3) && !plan::has_flag(plan::kVariantPlain, plan::N1, 2, 1) &&
                  !plan::has_flag(plan::kVariantFd, plan::FA, 3, 3) && !plan::has_flag(plan::kVariantFd, plan::N1, 2, 1),
              "they belong to no other kernel");
static_assert(!plan::has_flag(kV, plan::FA, 2, 1), "LIGHT's flag of FA is not the re-deal's");
static_assert(plan::steady_begin(kV, plan::FA, 3) == 10 && plan::steady_end(kV, plan::FA, 10) == 9 && plan::steady_end(kV, plan::N1, 10) == 12,
              "constexpr");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int max_onset = atoi(argv[1]), max_nfr = atoi(argv[2]);
    printf("variant %u %u\n", kV, plan::kRedeal);
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
                printf("range %d %d %d %d %d\n", role, onset, nfr, plan::steady_begin(kV, role, on), plan::steady_end(kV, role, nfr));
            }
    return 0;
}
