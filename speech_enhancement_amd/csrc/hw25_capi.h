/*
 * hw25_capi.h -- what the translation units behind the Hu-Wang C ABI share (hw_bank_capi.hip, hw25_resynth_capi.hip,
 * hw64_resynth_capi.hip): the refusal of outputs that are inputs and the single-utterance forms' batch of one.  What differs
 * between the two banks is in hw_bank.h.
 */
#pragma once
#include <initializer_list>

#include "capi_internal.h"

namespace sea_capi {

/* nonzero when one of the n outputs (null: not given) is one of the inputs or another output */
inline int shared_buffer(const void *const *outs, int n, std::initializer_list<const void *> ins)
{
    for (int i = 0; i < n; ++i) {
        if (!outs[i]) continue;
        for (const void *in : ins)
            if (outs[i] == in) return 1;
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return 1;
    }
    return 0;
}

/* One utterance from host memory as a batch of one: the samples zero-padded to Lp = L rounded up to 8 on the device, and
 * the three words a batch call takes as offsets, lengths and row_offsets (0, L, 0).  F = L / hop frames (80 samples on the
 * 25-channel bank, 160 on the 64-channel one); rows = F, but at least 1, is what the frame outputs are allocated for. */
struct Hw25Single {
    long long Lp = 0, F = 0, rows = 1;
    const float *d_in = nullptr;
    const long long *d_offsets = nullptr, *d_lengths = nullptr, *d_row_offsets = nullptr;

    int load(const float *x, long L, int hop = SEA_HW25_HOP) /* L > 0; 0 or fail() */
    {
        Lp = align8(L);
        F = L / hop;
        rows = F > 0 ? F : 1;
        HIP_TRY(in_.alloc((size_t)Lp));
        HIP_TRY(meta_.alloc(3));
        const long long meta[3] = {0, L, 0};
        HIP_TRY(hipMemset(in_.p, 0, (size_t)Lp * sizeof(float)));
        HIP_TRY(hipMemcpy(in_.p, x, (size_t)L * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(meta_.p, meta, sizeof meta, hipMemcpyHostToDevice));
        d_in = in_.p;
        d_offsets = meta_.p;
        d_lengths = meta_.p + 1;
        d_row_offsets = meta_.p + 2;
        return 0;
    }

    /* the F rows of `width` elements at d_src to host memory, where the caller asked for them and there is a frame */
    template <typename T>
    int rows_back(T *dst, const T *d_src, size_t width) const
    {
        if (dst && F > 0) HIP_TRY(hipMemcpy(dst, d_src, (size_t)F * width * sizeof(T), hipMemcpyDeviceToHost));
        return 0;
    }

private:
    DevBuf<float> in_;
    DevBuf<long long> meta_;
};

} // namespace sea_capi
