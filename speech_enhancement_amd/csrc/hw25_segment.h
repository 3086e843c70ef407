/*
 * hw25_segment.h -- the label propagation that both of the Hu-Wang estimator's segmentations share: initGroup's
 * (hw25_pitch_kernel.hip) and finalSeg's reSegmentation (hw25_am_kernel.hip).  One wave per utterance.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "sea_tables.h"

namespace sea {

constexpr int kHw25None = 0x7fffffff;

/* lab [F][25]: the unit's own index where it is marked, kHw25None elsewhere.  On return every marked unit holds the smallest
 * unit index of its 4-connected component.  Lane = channel; a frame takes the label of the frame before it in sweep direction
 * (carried in registers), then every run of marked channels takes its minimum.  Forward and backward sweeps until neither
 * changes anything.  The caller fences before and after. */
__device__ __forceinline__ void hw25_label_components(int *lab, int F, int lane)
{
    constexpr int kCh = SEA_HW25_NCHAN;
    constexpr unsigned kChanBits = (1u << kCh) - 1u;
    constexpr int kNone = kHw25None;
    bool again = true;
    while (again) {
        bool changed = false;
        for (int dir = 0; dir < 2; ++dir) {
            int carry = kNone;
            for (int k = 0; k < F; ++k) {
                const int f = dir ? F - 1 - k : k;
                const int old = lane < kCh ? lab[f * kCh + lane] : kNone;
                int v = old;
                if (v != kNone && carry < v) v = carry;
                const unsigned m = (unsigned)__ballot(v != kNone) & kChanBits;
                /* the run [start, end] of marked channels around this lane */
                const unsigned below = ~m & ((1u << (lane & 31)) - 1u);
                const int start = below ? 32 - __clz((int)below) : 0;
                const unsigned above = lane < 31 ? (~m >> (lane + 1)) : 1u;
                const int end = lane + (__ffs((int)above) - 1);
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) {
                    const int o = __shfl_up(v, d);
                    if (lane - d >= start && o < v) v = o;
                }
                const int r = __shfl(v, end & 63);
                if (old != kNone) {
                    v = r;
                    if (v != old) {
                        lab[f * kCh + lane] = v;
                        changed = true;
                    }
                } else {
                    v = kNone;
                }
                carry = v;
            }
        }
        again = __any(changed);
    }
}

} // namespace sea
