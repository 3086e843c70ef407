/*
 * capi_internal.h -- what the translation units behind the C ABI share: the per-thread error string and HIP_TRY, the
 * per-device context with the constant tables, the launch order and the NoiseSup form, and the HIP half of the chunked host
 * lists (chunk_plan.h holds the integer half): DevBuf, the chunk budget (scratch_budget), an RAII set of timing events
 * (EventSet) and a device buffer with its host staging (Staged).
 */
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/sea_mi355x.h"
#include "chunk_plan.h"
#include "sea_kernels.h"

namespace sea_capi {

int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *last_error();

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return ::sea_capi::fail("%s: %s", #expr, hipGetErrorString(e_));          \
    } while (0)

struct DeviceCtx {
    bool ready = false;
    sea_ns_tables *ns = nullptr;
    sea_cc_tables *cc = nullptr;
    sea_gt_tables *gt = nullptr;
    sea_ns16k_tables *ns16 = nullptr;
    sea_wb_tables *wb = nullptr;
    sea_hw25_tables *hw25 = nullptr;
    sea_hw64_tables *hw64 = nullptr;
    float *hw25_tw = nullptr; /* SEA_HW25_TWIDDLES (re, im) pairs: sea_build_hw25_twiddles (.., 1) */
    int n_cu = 256;
};

/* per-device context for the CURRENT device; uploads the constant tables on first use */
int ctx(DeviceCtx **out);

template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T) + 16); }
};

/* the budget of a chunk of a host list: the MiB that the variable env_name gives, else 60 % of the
 * HBM that is free now plus the held bytes the caller will reuse; env_name == nullptr: no override */
inline int scratch_budget(const char *env_name, long long *budget, size_t held = 0)
{
    const char *e = env_name ? getenv(env_name) : nullptr;
    size_t free_b = 0, total_b = 0;
    if (!e) HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = budget_of(free_b, held, e);
    return 0;
}

/* N device events; add_ms() after the synchronisation that follows the later one */
template <int N>
struct EventSet {
    hipEvent_t e[N] = {};
    ~EventSet()
    {
        for (hipEvent_t ev : e)
            if (ev) (void)hipEventDestroy(ev);
    }
    int create()
    {
        for (hipEvent_t &ev : e) HIP_TRY(hipEventCreate(&ev));
        return 0;
    }
    int add_ms(int from, int to, double *sum) const
    {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e[from], e[to]));
        *sum += ms;
        return 0;
    }
};

/* a device buffer and the host staging of the same n elements (none with host = false); the copies stay with the callers */
template <class T>
struct Staged {
    DevBuf<T> d;
    std::vector<T> h;
    hipError_t alloc(size_t n, bool host = true)
    {
        const hipError_t e = d.alloc(n);
        if (e == hipSuccess && host) h.resize(n);
        return e;
    }
};

/* launch order of the utterance-per-workgroup kernels: longest first, every other row of n_cu reversed */
void launch_order(const long long *lens, int n, int n_cu, int *order);
/* grid y of the Hu-Wang frame kernels: eight workgroups per CU over the batch, 1..1024; 0: no utterance, or fail() */
int per_utterance(int n_utt);

/* NoiseSup kernel form for a batch of n_inflight utterances sharing the device (capi.hip::sea_ns_denoise_batch):
 * 3 six-wave, 6 dense six-wave, 4 four-wave / tables in LDS, 2 four-wave; honours sea_ns_kernel_form / SEA_NS_KERNEL */
int ns_pick_form(int n_inflight, int n_cu);
/* one launch of that form over a.n_utt utterances; returns 0 or fail() */
int ns_launch(const sea::NsBatchArgs &a, int form, hipStream_t stream);

} // namespace sea_capi
