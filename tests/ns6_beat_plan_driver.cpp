/* Stand-alone driver of csrc/ns6_beat_plan.h for tests/test_ns6_beat_plan_cpu.py (no HIP, no GPU).
 * stdout: "depth <kDepth>", then per variant and role
 *     "flags <variant> <role> <ahead> <settle> d:k d:k ..."   the flags that apply in that variant
 * then per case of the sweep (onset -1 = the gate never opens, 0 .. max_onset; nfr 0 .. max_nfr)
 *     "range <variant> <role> <onset> <nfr> <steady_begin> <steady_end>"
 * argv: max_onset max_nfr */
#include <stdio.h>
#include <stdlib.h>

#include "ns6_beat_plan.h"

namespace plan = sea::ns6plan;

/* the kernel takes both ends as compile-time folds of these functions: they must be usable in constant expressions */
static_assert(plan::steady_begin(plan::kVariantDense, plan::S, 3) == 17 && plan::steady_end(plan::kVariantDense, plan::FA, 10) == 9, "constexpr");
static_assert(plan::steady_begin(plan::kVariantFd, plan::G1, plan::kNoOnset) == plan::kNoOnset, "no onset: no steady beat");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int max_onset = atoi(argv[1]), max_nfr = atoi(argv[2]);
    const unsigned variants[3] = {plan::kVariantPlain, plan::kVariantDense, plan::kVariantFd};
    printf("depth %d\n", plan::kDepth);
    for (unsigned v : variants)
        for (int role = 0; role < plan::kRoles; ++role) {
            const plan::RolePlan &p = plan::kPlan[role];
            printf("flags %u %d %d %d", v, role, p.ahead, p.settle);
            for (int j = 0; j < p.n; ++j)
                if (plan::flag_applies(p.f[j], v)) {
                    printf(" %d:%d", p.f[j].d, p.f[j].k);
                    if (!plan::has_flag(v, role, p.f[j].d, p.f[j].k)) return 3;
                }
            printf("\n");
        }
    for (unsigned v : variants)
        for (int role = 0; role < plan::kRoles; ++role)
            for (int onset = -1; onset <= max_onset; ++onset)
                for (int nfr = 0; nfr <= max_nfr; ++nfr) {
                    const int on = onset < 0 ? plan::kNoOnset : onset;
                    printf("range %u %d %d %d %d %d\n", v, role, onset, nfr, plan::steady_begin(v, role, on), plan::steady_end(v, role, nfr));
                }
    return 0;
}
