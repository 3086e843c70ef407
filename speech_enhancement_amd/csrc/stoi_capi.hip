/*
 * stoi_capi.hip -- the C ABI of the short-time objective intelligibility measure (include/sea_mi355x.h, DESIGN.md section
 * 5.24): lists of utterances from host memory, staged in chunks of whole utterances that fit the device, scored by the kernels
 * of stoi_kernel.hip.  Host pointers only.  No host synchronisation inside a chunk: the number of kept frames stays on the
 * device and every later launch covers the upper bound F.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "stoi_kernels.h"

using namespace sea_capi;

namespace {

thread_local int t_last_chunks = 0;
constexpr int kStages = SEA_STOI_STAGE_COUNT;
thread_local double t_stage_ms[kStages] = {};

/* what the tables and the buffers of a chunk are sized by */
struct Shape {
    long long L10, F, S;
    Shape(long long L, int rate)
    {
        const int q = rate == 16000 ? 8 : 4;
        L10 = (5 * L + q - 1) / q;
        F = L10 < 256 ? 0 : (L10 - 256) / 128 + 1;
        S = F > sea::kStoiSegment - 1 ? F - (sea::kStoiSegment - 1) : 0;
    }
    long long x_pad() const { return (L10 + 3) & ~3LL; }
};

constexpr int kTables = 7; /* tables of n + 1 entries in the meta block, after offsets [n] and lengths [n] */

/* of an utterance: padded samples, what the kTables tables are the prefix sums of, bytes */
constexpr size_t kSizes = 1 + kTables + 1;
using Sizes = Totals<kSizes>;
enum { S, X, F, G, ITEMS /* tiles of L10: the longest of the item lists */ };

} // namespace

extern "C" {

int sea_stoi_last_chunks(void) { return t_last_chunks; }

double sea_stoi_last_stage_ms(int stage) { return stage >= 0 && stage < kStages ? t_stage_ms[stage] : -1.0; }

/* Device footprint of a chunk: per padded input sample 4 B (ref and est), per resampled sample 8 B, per frame its energy, its
 * keep entry and two rows of 15 bands, per possible segment 15 terms, per utterance nine table entries and its results
 * (the basis, 448 KB, is there whatever the cut and is not counted) */
int sea_stoi_utterances(const short *const *ref, const short *const *est, const long *lengths, int n_utt, int rate, double *stoi_sum,
                        long long *stoi_terms, int *frames_kept, float *const *d_out)
{
    t_last_chunks = 0;
    if (n_utt < 0) return fail("stoi: n_utt = %d", n_utt);
    if (rate != 16000 && rate != 8000) return fail("stoi: rate = %d (16000 or 8000)", rate);
    if (n_utt == 0) return 0;
    if (!ref || !est || !lengths || !stoi_sum || !stoi_terms || !frames_kept) return fail("stoi: a required argument is NULL");
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0 || (long long)lengths[u] > 0x7fffffffLL) return fail("stoi: utterance %d has %ld samples (0 .. 2^31 - 1)", u, lengths[u]);
        if (lengths[u] > 0 && (!ref[u] || !est[u])) return fail("stoi: utterance %d has a NULL buffer", u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    long long budget;
    if (scratch_budget("SEA_SCORE_SCRATCH_MB", &budget)) return 1;
    auto of = [&](int u) -> Sizes {
        const Shape sh(lengths[u], rate);
        const long long s = align8(lengths[u]);
        return {s, sh.x_pad(), sh.F, sh.S, tiles_of(sh.L10, sea::kStoiItems), tiles_of(sh.F, sea::kStoiItems),
                tiles_of(sh.F, sea::kStoiTileRows), tiles_of(sh.S * sea::kStoiBands, sea::kStoiItems),
                s * 4 + sh.x_pad() * 8 + sh.F * (8 + 2 * sea::kStoiBands * 4) + sh.S * sea::kStoiBands * 4 + 160};
    };
    const ChunkPlan<kSizes> plan = plan_chunks<kSizes>(n_utt, budget, of);
    const size_t max_s = (size_t)plan.max[S], max_f = (size_t)plan.max[F], max_g = (size_t)plan.max[G], max_n = (size_t)plan.max_n;
    if (plan.max[ITEMS] > 0x7fffffffLL) return fail("stoi: %lld items in one launch", plan.max[ITEMS]);
    Staged<short> b_ref, b_est;
    Staged<float> b_d;
    Staged<long long> b_meta;
    Staged<int> b_kept;
    DevBuf<float> d_x, d_energy, d_bands, d_basis;
    DevBuf<uint32_t> d_emax;
    DevBuf<int> d_keep;
    DevBuf<double> d_sum;
    HIP_TRY(b_ref.alloc(max_s));
    HIP_TRY(b_est.alloc(max_s));
    HIP_TRY(d_x.alloc(2 * (size_t)plan.max[X]));
    HIP_TRY(d_energy.alloc(max_f));
    HIP_TRY(d_keep.alloc(max_f));
    HIP_TRY(d_bands.alloc(2 * max_f * sea::kStoiBands));
    HIP_TRY(b_d.alloc(max_g * sea::kStoiBands, d_out != nullptr));
    HIP_TRY(d_basis.alloc((size_t)sea::kStoiBasisRows * 256));
    HIP_TRY(b_meta.alloc(2 * max_n + kTables * (max_n + 1)));
    HIP_TRY(d_emax.alloc(max_n));
    HIP_TRY(b_kept.alloc(max_n));
    HIP_TRY(d_sum.alloc(max_n));
    hipStream_t stream = nullptr;
    EventSet<kStages + 1> ev;
    if (ev.create()) return 1;
    for (double &ms : t_stage_ms) ms = 0.0;
    hipLaunchKernelGGL(sea::stoi_basis_kernel, dim3(sea::kStoiBasisRows), dim3(256), 0, stream, d_basis.p);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < plan.chunks(); ++k) {
        const int u0 = plan.cuts[k], n = plan.cuts[k + 1] - u0;
        long long *offs = b_meta.h.data(), *lens = offs + n, *tab[kTables];
        for (int t = 0; t < kTables; ++t) tab[t] = lens + n + t * ((size_t)n + 1);
        long long s = 0, run[kTables] = {};
        for (int j = 0; j < n; ++j) {
            const Sizes q = of(u0 + j);
            offs[j] = s, lens[j] = lengths[u0 + j];
            for (int t = 0; t < kTables; ++t) tab[t][j] = run[t], run[t] += q[1 + t];
            pack_padded(b_ref.h.data() + s, ref[u0 + j], lens[j]);
            pack_padded(b_est.h.data() + s, est[u0 + j], lens[j]);
            s += q[S];
        }
        for (int t = 0; t < kTables; ++t) tab[t][n] = run[t];
        if (s > 0) {
            HIP_TRY(hipMemcpyAsync(b_ref.d.p, b_ref.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(b_est.d.p, b_est.h.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
        }
        const size_t meta_used = 2 * (size_t)n + kTables * ((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(b_meta.d.p, b_meta.h.data(), meta_used * sizeof(long long), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_emax.p, 0, (size_t)n * sizeof(uint32_t), stream));
        sea::StoiArgs a;
        const long long *dt = b_meta.d.p + 2 * (size_t)n;
        a.ref = b_ref.d.p, a.est = b_est.d.p, a.offsets = b_meta.d.p, a.lengths = b_meta.d.p + n;
        a.x_offsets = dt, a.frame_cum = dt + (n + 1), a.seg_cum = dt + 2 * (n + 1), a.x_tiles = dt + 3 * (n + 1);
        a.e_tiles = dt + 4 * (n + 1), a.band_tiles = dt + 5 * (n + 1), a.seg_tiles = dt + 6 * (n + 1);
        a.x10 = d_x.p, a.energy = d_energy.p, a.emax = d_emax.p, a.keep = d_keep.p, a.kept = b_kept.d.p, a.bands = d_bands.p;
        a.basis = d_basis.p, a.d = b_d.d.p, a.stoi_sum = d_sum.p;
        a.n_utt = n, a.rate = rate;
        /* the grids are the work: flat item lists over the utterances, found by bisection in the kernels */
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_RESAMPLE], stream));
        if (run[3] > 0) hipLaunchKernelGGL(sea::stoi_resample_kernel, dim3((unsigned)run[3], 2), dim3(256), 0, stream, a);
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_ENERGY], stream));
        if (run[4] > 0) hipLaunchKernelGGL(sea::stoi_energy_kernel, dim3((unsigned)run[4]), dim3(256), 0, stream, a);
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_COMPACT], stream));
        hipLaunchKernelGGL(sea::stoi_compact_kernel, dim3((unsigned)n), dim3(256), 0, stream, a);
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_BAND], stream));
        if (run[5] > 0) hipLaunchKernelGGL(sea::stoi_band_kernel, dim3((unsigned)run[5], 2), dim3(256), 0, stream, a);
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_SEGMENT], stream));
        if (run[6] > 0) hipLaunchKernelGGL(sea::stoi_segment_kernel, dim3((unsigned)run[6]), dim3(256), 0, stream, a);
        HIP_TRY(hipEventRecord(ev.e[SEA_STOI_STAGE_FINISH], stream));
        hipLaunchKernelGGL(sea::stoi_finish_kernel, dim3((unsigned)n), dim3(64), 0, stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[kStages], stream));
        HIP_TRY(hipMemcpyAsync(stoi_sum + u0, d_sum.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(b_kept.h.data(), b_kept.d.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (d_out && run[2] > 0)
            HIP_TRY(hipMemcpyAsync(b_d.h.data(), b_d.d.p, (size_t)run[2] * sea::kStoiBands * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int st = 0; st < kStages; ++st)
            if (ev.add_ms(st, st + 1, &t_stage_ms[st])) return 1;
        for (int j = 0; j < n; ++j) {
            const long long M = b_kept.h[j], S = M > sea::kStoiSegment - 1 ? M - (sea::kStoiSegment - 1) : 0;
            frames_kept[2 * (size_t)(u0 + j)] = (int)(tab[1][j + 1] - tab[1][j]);
            frames_kept[2 * (size_t)(u0 + j) + 1] = (int)M;
            stoi_terms[u0 + j] = S * sea::kStoiBands;
            if (d_out && d_out[u0 + j] && S > 0)
                memcpy(d_out[u0 + j], b_d.h.data() + tab[2][j] * sea::kStoiBands, (size_t)S * sea::kStoiBands * sizeof(float));
        }
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
