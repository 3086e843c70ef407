/* Stand-alone driver of csrc/ns6_beat_plan.h for tests/test_ns6_idct_plan_cpu.py (no HIP, no GPU): the variant of the dense kernel in
 * which the helper wave adds up both stages' IDCT sums, kVariantDenseIdct, which has a table and a depth of its own.  stdout:
 *     "variant <value> <kIdctS> <depth_of(value)> <kDepth>", then per role
 *     "flags <role> <ahead> <settle> d:k d:k ..."        the flags that apply in the new variant
 *     "ends <role> <steady_lead> <steady_tail>"
 * then per existing variant v (plain, dense, fd, re-dealt, bin 64) and role
 *     "old <v> <role> <depth_of(v)> <steady_lead> <steady_tail> <steady_begin(v, role, 7)> <steady_end(v, role, 50)> d:k d:k ..."
 * then per case of the sweep (onset -1 = the gate never opens, 0 .. max_onset; nfr 0 .. max_nfr)
 *     "range <role> <onset> <nfr> <steady_begin> <steady_end>"
 * argv: max_onset max_nfr */
#include <stdio.h>
#include <stdlib.h>

#include "ns6_beat_plan.h"

namespace plan = sea::ns6plan;

constexpr unsigned kV = plan::kVariantDenseIdct;
/* what the kernel folds at compile time */
static_assert(kV == (plan::kRedeal | plan::kBin64 | plan::kIdctS) && (kV & (plan::kFd | plan::kLight | plan::kDifg1)) == 0u, "the dense body plus one bit");
static_assert((plan::kIdctS & (plan::kFd | plan::kLight | plan::kDifg1 | plan::kRedeal | plan::kBin64)) == 0u && plan::kIdctS != plan::kAlways, "a bit of its own");
static_assert(plan::depth_of(kV) == 12 && plan::depth_of(plan::kVariantDenseBin64) == plan::kDepth && plan::kDepth == 9, "its own depth");
static_assert(plan::has_flag(kV, plan::G1, 11, 5) && plan::has_flag(kV, plan::G1, 9, 5) && !plan::has_flag(kV, plan::G1, 8, 5), "G1's two jobs");
static_assert(plan::has_flag(kV, plan::S, 10, 5) && plan::has_flag(kV, plan::S, 12, 5) && !plan::has_flag(kV, plan::S, 9, 5), "S's stage-1 sums and output");
static_assert(!plan::has_flag(plan::kVariantDenseBin64, plan::G1, 11, 5) && !plan::has_flag(plan::kVariantPlain, plan::S, 10, 5) &&
                  !plan::has_flag(plan::kVariantFd, plan::S, 12, 5) && plan::has_flag(plan::kVariantDenseBin64, plan::G1, 8, 5),
              "the other kernels keep their table");
static_assert(plan::steady_begin(kV, plan::S, 3) == 20 && plan::steady_end(kV, plan::G1, 10) == 19 && plan::steady_begin(kV, plan::FA, plan::kNoOnset) == plan::kNoOnset,
              "constexpr");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int max_onset = atoi(argv[1]), max_nfr = atoi(argv[2]);
    printf("variant %u %u %d %d\n", kV, plan::kIdctS, plan::depth_of(kV), plan::kDepth);
    for (int role = 0; role < plan::kRoles; ++role) {
        const plan::RolePlan &p = plan::plan_of(kV, role);
        if (p.n > plan::kMaxFlags) return 4;
        printf("flags %d %d %d", role, p.ahead, p.settle);
        for (int j = 0; j < p.n; ++j)
            if (plan::flag_applies(p.f[j], kV)) {
                printf(" %d:%d", p.f[j].d, p.f[j].k);
                if (!plan::has_flag(kV, role, p.f[j].d, p.f[j].k)) return 3;
            }
        printf("\nends %d %d %d\n", role, plan::steady_lead(kV, role), plan::steady_tail(kV, role));
    }
    const unsigned olds[5] = {plan::kVariantPlain, plan::kVariantDense, plan::kVariantFd, plan::kVariantDenseRedeal, plan::kVariantDenseBin64};
    for (unsigned v : olds)
        for (int role = 0; role < plan::kRoles; ++role) {
            const plan::RolePlan &p = plan::plan_of(v, role);
            if (&p != &plan::kPlan[role]) return 5;
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
