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

struct Events {
    hipEvent_t e[kStages + 1] = {};
    ~Events()
    {
        for (hipEvent_t ev : e)
            if (ev) (void)hipEventDestroy(ev);
    }
    int create()
    {
        for (hipEvent_t &ev : e) HIP_TRY(hipEventCreate(&ev));
        return 0;
    }
};

long long tiles_of(long long n, int per) { return (n + per - 1) / per; }

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
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    long long budget = (long long)(free_b / 10 * 6);
    if (const char *e = getenv("SEA_SCORE_SCRATCH_MB")) budget = atoll(e) * (1LL << 20);

    std::vector<int> cuts(1, 0);
    {
        long long run = 0;
        for (int u = 0; u < n_utt; ++u) {
            const Shape sh(lengths[u], rate);
            const long long b = align8(lengths[u]) * 4 + sh.x_pad() * 8 + sh.F * (8 + 2 * sea::kStoiBands * 4) + sh.S * sea::kStoiBands * 4 + 160;
            if (u > cuts.back() && run + b > budget) {
                cuts.push_back(u);
                run = 0;
            }
            run += b;
        }
        cuts.push_back(n_utt);
    }
    const int nchunk = (int)cuts.size() - 1;
    long long max_s = 0, max_x = 0, max_f = 0, max_g = 0, max_items = 0;
    int max_n = 0;
    for (int k = 0; k < nchunk; ++k) {
        long long s = 0, x = 0, f = 0, g = 0, items = 0;
        for (int u = cuts[k]; u < cuts[k + 1]; ++u) {
            const Shape sh(lengths[u], rate);
            s += align8(lengths[u]), x += sh.x_pad(), f += sh.F, g += sh.S;
            items += tiles_of(sh.L10, sea::kStoiItems); /* the longest of the item lists */
        }
        max_s = std::max(max_s, s), max_x = std::max(max_x, x), max_f = std::max(max_f, f), max_g = std::max(max_g, g);
        max_items = std::max(max_items, items), max_n = std::max(max_n, cuts[k + 1] - cuts[k]);
    }
    if (max_items > 0x7fffffffLL) return fail("stoi: %lld items in one launch", max_items);
    const size_t meta_n = 2 * (size_t)max_n + kTables * ((size_t)max_n + 1);
    DevBuf<short> d_ref, d_est;
    DevBuf<float> d_x, d_energy, d_bands, d_basis, d_d;
    DevBuf<long long> d_meta;
    DevBuf<uint32_t> d_emax;
    DevBuf<int> d_keep, d_kept;
    DevBuf<double> d_sum;
    HIP_TRY(d_ref.alloc((size_t)max_s));
    HIP_TRY(d_est.alloc((size_t)max_s));
    HIP_TRY(d_x.alloc(2 * (size_t)max_x));
    HIP_TRY(d_energy.alloc((size_t)max_f));
    HIP_TRY(d_keep.alloc((size_t)max_f));
    HIP_TRY(d_bands.alloc(2 * (size_t)max_f * sea::kStoiBands));
    HIP_TRY(d_d.alloc((size_t)max_g * sea::kStoiBands));
    HIP_TRY(d_basis.alloc((size_t)sea::kStoiBasisRows * 256));
    HIP_TRY(d_meta.alloc(meta_n));
    HIP_TRY(d_emax.alloc((size_t)max_n));
    HIP_TRY(d_kept.alloc((size_t)max_n));
    HIP_TRY(d_sum.alloc((size_t)max_n));
    std::vector<short> h_ref((size_t)max_s), h_est((size_t)max_s);
    std::vector<float> h_d(d_out ? (size_t)max_g * sea::kStoiBands : 0);
    std::vector<long long> h_meta(meta_n);
    std::vector<int> h_kept((size_t)max_n);
    hipStream_t stream = nullptr;
    Events ev;
    if (ev.create()) return 1;
    for (double &ms : t_stage_ms) ms = 0.0;
    hipLaunchKernelGGL(sea::stoi_basis_kernel, dim3(sea::kStoiBasisRows), dim3(256), 0, stream, d_basis.p);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < nchunk; ++k) {
        const int u0 = cuts[k], n = cuts[k + 1] - u0;
        long long *offs = h_meta.data(), *lens = offs + n, *tab[kTables];
        for (int t = 0; t < kTables; ++t) tab[t] = lens + n + t * ((size_t)n + 1);
        long long s = 0, run[kTables] = {};
        for (int j = 0; j < n; ++j) {
            const long long L = lengths[u0 + j], Lp = align8(L);
            const Shape sh(L, rate);
            offs[j] = s, lens[j] = L;
            for (int t = 0; t < kTables; ++t) tab[t][j] = run[t];
            if (L > 0) {
                memcpy(h_ref.data() + s, ref[u0 + j], (size_t)L * sizeof(short));
                memcpy(h_est.data() + s, est[u0 + j], (size_t)L * sizeof(short));
            }
            if (Lp > L) {
                memset(h_ref.data() + s + L, 0, (size_t)(Lp - L) * sizeof(short));
                memset(h_est.data() + s + L, 0, (size_t)(Lp - L) * sizeof(short));
            }
            s += Lp;
            run[0] += sh.x_pad(), run[1] += sh.F, run[2] += sh.S;
            run[3] += tiles_of(sh.L10, sea::kStoiItems), run[4] += tiles_of(sh.F, sea::kStoiItems);
            run[5] += tiles_of(sh.F, sea::kStoiTileRows), run[6] += tiles_of(sh.S * sea::kStoiBands, sea::kStoiItems);
        }
        for (int t = 0; t < kTables; ++t) tab[t][n] = run[t];
        if (s > 0) {
            HIP_TRY(hipMemcpyAsync(d_ref.p, h_ref.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_est.p, h_est.data(), (size_t)s * sizeof(short), hipMemcpyHostToDevice, stream));
        }
        const size_t meta_used = 2 * (size_t)n + kTables * ((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(d_meta.p, h_meta.data(), meta_used * sizeof(long long), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_emax.p, 0, (size_t)n * sizeof(uint32_t), stream));
        sea::StoiArgs a;
        const long long *dt = d_meta.p + 2 * (size_t)n;
        a.ref = d_ref.p, a.est = d_est.p, a.offsets = d_meta.p, a.lengths = d_meta.p + n;
        a.x_offsets = dt, a.frame_cum = dt + (n + 1), a.seg_cum = dt + 2 * (n + 1), a.x_tiles = dt + 3 * (n + 1);
        a.e_tiles = dt + 4 * (n + 1), a.band_tiles = dt + 5 * (n + 1), a.seg_tiles = dt + 6 * (n + 1);
        a.x10 = d_x.p, a.energy = d_energy.p, a.emax = d_emax.p, a.keep = d_keep.p, a.kept = d_kept.p, a.bands = d_bands.p;
        a.basis = d_basis.p, a.d = d_d.p, a.stoi_sum = d_sum.p;
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
        HIP_TRY(hipMemcpyAsync(h_kept.data(), d_kept.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (d_out && run[2] > 0)
            HIP_TRY(hipMemcpyAsync(h_d.data(), d_d.p, (size_t)run[2] * sea::kStoiBands * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int st = 0; st < kStages; ++st) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.e[st], ev.e[st + 1]));
            t_stage_ms[st] += ms;
        }
        for (int j = 0; j < n; ++j) {
            const long long M = h_kept[j], S = M > sea::kStoiSegment - 1 ? M - (sea::kStoiSegment - 1) : 0;
            frames_kept[2 * (size_t)(u0 + j)] = (int)(tab[1][j + 1] - tab[1][j]);
            frames_kept[2 * (size_t)(u0 + j) + 1] = (int)M;
            stoi_terms[u0 + j] = S * sea::kStoiBands;
            if (d_out && d_out[u0 + j] && S > 0)
                memcpy(d_out[u0 + j], h_d.data() + tab[2][j] * sea::kStoiBands, (size_t)S * sea::kStoiBands * sizeof(float));
        }
        t_last_chunks = k + 1;
    }
    return 0;
}

} // extern "C"
