/*
 * capi.hip -- the C ABI of libsea_mi355x.so (include/sea_mi355x.h): context, launches, and the
 * host-buffer drop-ins that keep the reference's own signatures.
 */
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "capi_internal.h"

namespace sea_capi {

namespace {
thread_local char g_err[512] = "";
}

int fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}
const char *last_error() { return g_err; }

namespace {
constexpr int kMaxDev = 64;
DeviceCtx g_ctx[kMaxDev];
std::mutex g_mu;
sea_ns_tables g_ns_host;
sea_cc_tables g_cc_host;
sea_gt_tables g_gt_host;
sea_ns16k_tables g_ns16_host;
sea_wb_tables g_wb_host;
sea_hw25_tables g_hw25_host;
sea_hw64_tables g_hw64_host;
std::vector<float> g_hw25_tw; /* the forward FFT's twiddles; the inverse's are checked to be their conjugates */
bool g_hw25_tw_conjugate = false;
bool g_host_ready = false;

void host_tables()
{
    if (g_host_ready) return;
    sea_build_ns_tables(&g_ns_host);
    sea_build_cc_tables(&g_cc_host);
    sea_build_gt_tables(&g_gt_host);
    sea_build_ns16k_tables(&g_ns16_host);
    sea_build_wb_tables(&g_wb_host);
    sea_build_hw25_tables(&g_hw25_host);
    sea_build_hw64_tables(&g_hw64_host);
    {
        std::vector<float> inv(2 * (size_t)SEA_HW25_TWIDDLES);
        g_hw25_tw.resize(2 * (size_t)SEA_HW25_TWIDDLES);
        sea_build_hw25_twiddles(g_hw25_tw.data(), 1);
        sea_build_hw25_twiddles(inv.data(), -1);
        g_hw25_tw_conjugate = true;
        for (size_t i = 0; i < (size_t)SEA_HW25_TWIDDLES; ++i)
            if (inv[2 * i] != g_hw25_tw[2 * i] || inv[2 * i + 1] != -g_hw25_tw[2 * i + 1]) g_hw25_tw_conjugate = false;
    }
    g_host_ready = true;
}
} // namespace

int ctx(DeviceCtx **out)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDev) return fail("device index %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceCtx &c = g_ctx[dev];
    if (!c.ready) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail("device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
        c.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        host_tables();
        HIP_TRY(hipMalloc(&c.ns, sizeof(sea_ns_tables)));
        HIP_TRY(hipMalloc(&c.cc, sizeof(sea_cc_tables)));
        HIP_TRY(hipMalloc(&c.gt, sizeof(sea_gt_tables)));
        HIP_TRY(hipMalloc(&c.ns16, sizeof(sea_ns16k_tables)));
        HIP_TRY(hipMalloc(&c.wb, sizeof(sea_wb_tables)));
        HIP_TRY(hipMalloc(&c.hw25, sizeof(sea_hw25_tables)));
        HIP_TRY(hipMalloc(&c.hw64, sizeof(sea_hw64_tables)));
        HIP_TRY(hipMemcpy(c.ns, &g_ns_host, sizeof g_ns_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.cc, &g_cc_host, sizeof g_cc_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.gt, &g_gt_host, sizeof g_gt_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.ns16, &g_ns16_host, sizeof g_ns16_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.wb, &g_wb_host, sizeof g_wb_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.hw25, &g_hw25_host, sizeof g_hw25_host, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.hw64, &g_hw64_host, sizeof g_hw64_host, hipMemcpyHostToDevice));
        if (!g_hw25_tw_conjugate) return fail("hw25: the inverse FFT's twiddles are not the conjugates of the forward ones");
        HIP_TRY(hipMalloc(&c.hw25_tw, g_hw25_tw.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(c.hw25_tw, g_hw25_tw.data(), g_hw25_tw.size() * sizeof(float), hipMemcpyHostToDevice));
        c.ready = true;
    }
    *out = &c;
    return 0;
}

/* launch order of the utterance-per-workgroup kernels: longest first, every other row of n_cu reversed
 * (workgroups b, b + n_cu, ... share a CU; see speech_enhancement_amd/engine.py::launch_order) */
void launch_order(const long long *lens, int n, int n_cu, int *order)
{
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    for (int start = 0, row = 0; start < n; start += n_cu, ++row) {
        const int end = start + n_cu < n ? start + n_cu : n;
        if (row & 1) std::reverse(idx.begin() + start, idx.begin() + end);
    }
    for (int i = 0; i < n; ++i) order[i] = idx[i];
}

/* Grid y of the Hu-Wang frame kernels (hw_bank_capi.hip): a fixed number of workgroups (or waves) per utterance walks its
 * frames, about eight per CU over the batch and at most 1024; the utterances go on grid x (y ends at 65535).  The lengths stay
 * on the device, so the number is the same for every utterance.  0: no utterance, or fail(). */
int per_utterance(int n_utt)
{
    DeviceCtx *c;
    if (n_utt <= 0 || ctx(&c)) return 0;
    int per_utt = (8 * c->n_cu + n_utt - 1) / n_utt;
    per_utt = per_utt < 1 ? 1 : (per_utt > 1024 ? 1024 : per_utt);
    return per_utt;
}

void gammatone_host_tables(float *cf64, float *bw64, float *midEar64)
{
    std::lock_guard<std::mutex> lk(g_mu);
    host_tables();
    memcpy(cf64, g_gt_host.cf, sizeof g_gt_host.cf);
    memcpy(bw64, g_gt_host.bw, sizeof g_gt_host.bw);
    memcpy(midEar64, g_gt_host.midEar, sizeof g_gt_host.midEar);
}

/* diagnostic (tools/ns6_perm_sweep.py): wave -> role map of the six-wave forms, three bits per wave, wave 0 lowest; 0 = the
 * kernel's own.  The kernels take the map as it comes, and a map that leaves a role unstaffed or doubled gives wrong output without
 * any error, so only 0 and permutations of the roles 0..5 get past this function. */
static bool ns6_perm_valid(int perm)
{
    if (perm == 0) return true;
    if ((unsigned)perm >> 18) return false;
    unsigned seen = 0;
    for (int w = 0; w < 6; ++w) seen |= 1u << ((perm >> (3 * w)) & 7);
    return seen == 0x3Fu;
}
/* initialised from SEA_NS6_PERM (octal); an invalid value is reported once and ignored */
static std::atomic<int> g_ns6_perm{[] {
    const char *e = getenv("SEA_NS6_PERM");
    const int perm = e ? (int)strtol(e, nullptr, 8) : 0;
    if (ns6_perm_valid(perm)) return perm;
    fprintf(stderr, "sea: SEA_NS6_PERM=%s is not a permutation of the six roles 0..5 (octal digits); ignored\n", e);
    return 0;
}()};
/* Forms of the same arithmetic (identical results), chosen by how many utterances share a CU:
 *   <= 3 per CU  six waves per utterance: shortest frame period (the run time is one utterance's
 *                chain of frames; 768 utterances: 1.74 ms against 1.85 for the dense form)   SEA_NS_KERNEL=pipe6
 *   <= 4 per CU  six waves per utterance compiled for seven waves per SIMD, so that four workgroups
 *                co-reside on a CU (round 4; ns_pipe6_kernel.hip; 896: 1.89 ms against 2.44)   SEA_NS_KERNEL=pipe6d
 *   more         four waves, tables in LDS: six workgroups per CU     SEA_NS_KERNEL=big
 *   (not chosen) four waves, transform address tables in VGPRs: the form for <= 4 per CU until round 4, 4 % behind the
 *                dense six-wave form there; the time-slice launches of the host pipelines run on it   SEA_NS_KERNEL=pipe
 * Removed after measurement (source at 24082b1; M frames/s on the configs[4] shard, against 465 for the big form then):
 *   form 1, one wave per utterance, the round-1 kernel: 190-219
 *   form 5, two utterances per workgroup, lane-sparse phases packed: 434 (profiles/r04_ns_pair_form_experiment.txt)
 *   form 7, one wave per utterance, the roles in sequence: 363 (profiles/r04_ns_six_wave_dense.txt) */
int ns_pick_form(int n_inflight, int n_cu)
{
    const int forced = sea_ns_kernel_form(-1);
    return forced ? forced : (n_inflight <= 3 * n_cu ? 3 : (n_inflight <= 4 * n_cu ? 6 : 4));
}

int ns_launch(const sea::NsBatchArgs &a, int form, hipStream_t stream)
{
    if (a.n_utt <= 0) return 0;
    if (a.state) { /* time slices: the four-wave forms only */
        if (form == 4)
            hipLaunchKernelGGL(sea::ns_denoise_pipe_big_slice_kernel, dim3(a.n_utt), dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL(sea::ns_denoise_pipe_slice_kernel, dim3(a.n_utt), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (form == 3 || form == 6) {
        sea::NsBatchArgs b = a;
        const int perm = g_ns6_perm.load(); /* diagnostic: the wave -> role map of the six-wave form (sea_debug_ns6_perm / SEA_NS6_PERM) */
        if (perm) b.perm6 = perm;
        if (form == 6) hipLaunchKernelGGL(sea::ns_denoise_pipe6_dense_kernel, dim3(a.n_utt), dim3(384), 0, stream, b);
        else hipLaunchKernelGGL(sea::ns_denoise_pipe6_kernel, dim3(a.n_utt), dim3(384), 0, stream, b);
    } else if (form == 4)
        hipLaunchKernelGGL(sea::ns_denoise_pipe_big_kernel, dim3(a.n_utt), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(sea::ns_denoise_pipe_kernel, dim3(a.n_utt), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace sea_capi

using namespace sea_capi;

extern "C" {

const char *sea_last_error(void) { return last_error(); }
const char *sea_version(void) { return "sea_mi355x 0.1 (gfx950)"; }

int sea_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sea_init(int device)
{
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    DeviceCtx *c;
    return ctx(&c);
}

int sea_tables_host(float *sigWindow200, float *irWindow17, float *idct25x25, int *melStart25,
                    int *melLen25, float *melData25x16, float *hamming100, float *dct12x23,
                    int *ccStart23, int *ccLen23, float *ccData23x32)
{
    sea_ns_plain_tables(sigWindow200, irWindow17, idct25x25, melStart25, melLen25, melData25x16);
    sea_cc_plain_tables(hamming100, dct12x23, ccStart23, ccLen23, ccData23x32);
    return 0;
}

/* diagnostic (tests/test_host_cpu.py, no GPU): the lane map of the tiled CompCeps kernels' mel pass (sea_tables.h, melLaneBase) */
extern "C" int sea_debug_cc_mel_lanes(int *base64, int *fb64, float *w24x64)
{
    std::lock_guard<std::mutex> lk(g_mu);
    host_tables();
    memcpy(base64, g_cc_host.melLaneBase, sizeof g_cc_host.melLaneBase);
    memcpy(fb64, g_cc_host.melLaneFb, sizeof g_cc_host.melLaneFb);
    memcpy(w24x64, g_cc_host.melLaneW, sizeof g_cc_host.melLaneW);
    return 0;
}

int sea_gammatone_channels(float *cf64, float *bw64, float *midEar64)
{
    gammatone_host_tables(cf64, bw64, midEar64);
    return 0;
}

/* ------------------------------------------------------------------------------------------- */
/* stores a valid map (ns6_perm_valid) and returns the one it replaces; any other value only reads, as sea_ns_kernel_form */
extern "C" int sea_debug_ns6_perm(int perm)
{
    return ns6_perm_valid(perm) ? g_ns6_perm.exchange(perm) : g_ns6_perm.load();
}

/* kernel form override: 0 = by batch size; initialised from SEA_NS_KERNEL on first use */
static std::atomic<int> g_ns_form{-1};
static int ns_form()
{
    int f = g_ns_form.load();
    if (f < 0) {
        const char *e = getenv("SEA_NS_KERNEL");
        f = 0;
        if (e && !strcmp(e, "pipe")) f = 2;
        if (e && !strcmp(e, "pipe6")) f = 3;
        if (e && !strcmp(e, "big")) f = 4;
        if (e && !strcmp(e, "pipe6d")) f = 6;
        g_ns_form.store(f);
    }
    return f;
}

/* diagnostic (tools/): resident workgroups per CU of NoiseSup kernel form f as the runtime computes them (0: unknown form) */
int sea_debug_ns_occupancy(int form)
{
    int n = 0;
    hipError_t e = hipErrorInvalidValue;
    if (form == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, sea::ns_denoise_pipe_kernel, 256, 0);
    if (form == 3) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, sea::ns_denoise_pipe6_kernel, 384, 0);
    if (form == 6) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, sea::ns_denoise_pipe6_dense_kernel, 384, 0);
    if (form == 4) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, sea::ns_denoise_pipe_big_kernel, 256, 0);
    if (form == 16) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, sea::ns16k_pipe_kernel, 512, 0);
    return e == hipSuccess ? n : -1;
}

int sea_ns_kernel_form(int form)
{
    const int prev = ns_form();
    if (form == 0 || form == 2 || form == 3 || form == 4 || form == 6) g_ns_form.store(form);
    return prev;
}

int sea_ns_denoise_batch(const short *d_in, short *d_out, float *d_out_f32,
                         const long long *d_offsets, const long long *d_lengths, const int *d_order,
                         int *d_first_out, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsBatchArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.out_f32 = d_out_f32;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    a.first_out = d_first_out;
    a.tables = c->ns;
    a.n_utt = n_utt;
    const int form = ns_pick_form(n_utt, c->n_cu);
    if (form == 2 || form == 3 || form == 6) a.prio_row = (d_order && n_utt > c->n_cu) ? c->n_cu : 0; /* rows of the longest-first launch order */
    return ns_launch(a, form, (hipStream_t)stream);
}

/* One TIME SLICE of a batch: see include/sea_mi355x.h */
int sea_ns_denoise_batch_slice(const short *d_in, short *d_out, float *d_out_f32, const long long *d_offsets,
                               const long long *d_lengths, const int *d_order, int *d_first_out, float *d_state, int n_utt,
                               int frame_base, int resume, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_state) return fail("sea_ns_denoise_batch_slice: d_state is required");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsBatchArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.out_f32 = d_out_f32;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    a.first_out = d_first_out;
    a.tables = c->ns;
    a.n_utt = n_utt;
    a.state = d_state;
    a.resume = resume;
    a.frame_base = frame_base;
    const int form = (n_utt <= 4 * c->n_cu) ? 2 : 4;
    if (form == 2) a.prio_row = (d_order && n_utt > c->n_cu) ? c->n_cu : 0;
    return ns_launch(a, form, (hipStream_t)stream);
}

int sea_ns_slice_state_floats(void) { return sea::kNsPipeStateFloats; }

/* ------------------------------------------------------------------------------------------- */
int sea_ns_denoise_batch_fd(const short *d_in, short *d_out, float *d_out_f32,
                            const long long *d_offsets, const long long *d_lengths, const int *d_order,
                            int *d_first_out, unsigned char *d_flags, int *d_onset, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_out_f32 || !d_first_out || !d_flags || !d_onset)
        return fail("ns_denoise_batch_fd: the float stream, first_out, flags and onset outputs are all required");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsBatchArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.out_f32 = d_out_f32;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    a.first_out = d_first_out;
    a.tables = c->ns;
    a.n_utt = n_utt;
    a.flags_out = d_flags;
    a.onset_out = d_onset;
    if (n_utt <= 2 * c->n_cu)
        hipLaunchKernelGGL(sea::ns_denoise_pipe6_fd_kernel, dim3(n_utt), dim3(384), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sea::ns_denoise_pipe_fd_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* the arguments the four feature-chain entry points have in common (sea_kernels.h, AfeArgs) */
static void afe_args(sea::AfeArgs *a, const DeviceCtx *c, const float *d_den_f32, const unsigned char *d_flags,
                     const long long *d_offsets, const long long *d_lengths, const int *d_first_out, const int *d_onset,
                     const long long *d_ceps_cum, float *d_feat_cc, float *d_feat_pp, const long long *d_feat_cum, float *d_feat15,
                     int *d_n_feat, int *d_n_ceps, int n_utt)
{
    *a = {};
    a->den_f32 = d_den_f32;
    a->flags = d_flags;
    a->offsets = d_offsets;
    a->lengths = d_lengths;
    a->first_out = d_first_out;
    a->onset = d_onset;
    a->ceps_cum = d_ceps_cum;
    a->feat_cc = d_feat_cc;
    a->feat_pp = d_feat_pp;
    a->feat_cum = d_feat_cum;
    a->feat15 = d_feat15;
    a->n_feat = d_n_feat;
    a->n_ceps = d_n_ceps;
    a->tables = c->cc;
    a->n_utt = n_utt;
}

int sea_afe_features_batch(const float *d_den_f32, const unsigned char *d_flags, const long long *d_offsets,
                           const long long *d_lengths, const int *d_first_out, const int *d_onset,
                           const long long *d_ceps_cum, long long total_ceps, float *d_feat_cc, float *d_feat_pp,
                           const long long *d_feat_cum, float *d_feat15, int *d_n_feat, int *d_n_ceps, int n_utt,
                           void *stream)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::AfeArgs a;
    afe_args(&a, c, d_den_f32, d_flags, d_offsets, d_lengths, d_first_out, d_onset, d_ceps_cum, d_feat_cc, d_feat_pp, d_feat_cum,
             d_feat15, d_n_feat, d_n_ceps, n_utt);
    if (total_ceps > 0) {
        const long long nslot = total_ceps / 8 + n_utt; /* tile slots of 8 frames (cc_kernel.hip, kAfeT) */
        constexpr long long kAfeGrid = 8192; /* waves of the launch */
        const long long want = nslot < kAfeGrid ? nslot : kAfeGrid;
        hipLaunchKernelGGL(sea::afe_ceps_kernel, dim3((unsigned)want), dim3(64), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::afe_vad_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* The 8 kHz feature chain in TIME SLICES: see include/sea_mi355x.h.  Step 1: sea_ns_denoise_batch_slice + what
 * sea_ns_denoise_batch_fd stores.  One kernel form, the four-wave one, at every batch size. */
int sea_ns_denoise_batch_slice_fd(const short *d_in, short *d_out, float *d_out_f32, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int *d_first_out,
                                  unsigned char *d_flags, int *d_onset, float *d_state, int n_utt,
                                  int frame_base, int resume, void *stream)
{
    const char *who = "sea_ns_denoise_batch_slice_fd";
    if (n_utt <= 0) return 0;
    if (!d_state) return fail("%s: d_state is required", who);
    if (!d_in || !d_out || !d_offsets || !d_lengths) return fail("%s: input, output, offsets and lengths are required", who);
    if (!d_out_f32 || !d_first_out || !d_flags || !d_onset)
        return fail("%s: the float stream, first_out, flags and onset outputs are all required", who);
    if (frame_base < 0) return fail("%s: frame_base must not be negative", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsBatchArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.out_f32 = d_out_f32;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    a.first_out = d_first_out;
    a.tables = c->ns;
    a.n_utt = n_utt;
    a.flags_out = d_flags;
    a.onset_out = d_onset;
    a.state = d_state;
    a.resume = resume != 0;
    a.frame_base = frame_base;
    a.prio_row = (d_order && n_utt > c->n_cu) ? c->n_cu : 0; /* by launch row, as sea_ns_denoise_batch_slice's form 2 */
    hipLaunchKernelGGL(sea::ns_denoise_pipe_fd_slice_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_afe_slice_state_floats(void) { return sea::kAfeStateFloats; }

/* Step 2 over one TIME SLICE: two launches as in sea_afe_features_batch, each the slice form of its kernel
 * (afe_slice_kernel.hip); the second one also stores what the next slice starts from. */
int sea_afe_features_batch_slice(const float *d_den_f32, const unsigned char *d_flags, const long long *d_offsets,
                                 const long long *d_lengths, const int *d_first_out, const int *d_onset,
                                 const unsigned char *d_final, const long long *d_ceps_cum, long long total_ceps,
                                 float *d_feat_cc, float *d_feat_pp, const long long *d_feat_cum, float *d_feat15,
                                 int *d_n_feat, int *d_n_ceps, float *d_afe_state, int n_utt, int frame_base,
                                 int resume, void *stream)
{
    const char *who = "sea_afe_features_batch_slice";
    if (n_utt <= 0) return 0;
    if (!d_afe_state) return fail("%s: d_afe_state is required", who);
    if (!d_den_f32 || !d_flags || !d_first_out || !d_onset)
        return fail("%s: the float stream, the flags, first_out and onset are required", who);
    if (!d_offsets || !d_lengths || !d_ceps_cum || !d_feat_cc || !d_feat_cum || !d_feat15 || !d_n_feat)
        return fail("%s: offsets, lengths, both prefix sums, feat_cc, feat15 and n_feat are required", who);
    if (total_ceps < 0) return fail("%s: total_ceps must not be negative", who);
    if (frame_base < 0) return fail("%s: frame_base must not be negative", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::AfeSliceArgs s = {};
    sea::AfeArgs &a = s.a;
    afe_args(&a, c, d_den_f32, d_flags, d_offsets, d_lengths, d_first_out, d_onset, d_ceps_cum, d_feat_cc, d_feat_pp, d_feat_cum,
             d_feat15, d_n_feat, d_n_ceps, n_utt);
    s.final = d_final;
    s.state = d_afe_state;
    s.frame_base = frame_base;
    s.resume = resume != 0;
    if (total_ceps > 0) {
        const long long nslot = total_ceps / 8 + n_utt; /* tile slots of 8 frames, as sea_afe_features_batch */
        constexpr long long kAfeGrid = 8192;
        const long long want = nslot < kAfeGrid ? nslot : kAfeGrid;
        hipLaunchKernelGGL(sea::afe_ceps_slice_kernel, dim3((unsigned)want), dim3(64), 0, (hipStream_t)stream, s);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::afe_vad_slice_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- the ETSI wideband (16 kHz) mode: QMF split + NoiseSup on the low band (wb_kernel.hip, ns_pipe_kernel.hip) ---- */
int sea_wb_tables_host(float *qmfLp118, float *qmfHp118, int *hpMelStart3, int *hpMelLen3, float *hpMelW3x64, float *dct12x26)
{
    sea_wb_plain_tables(qmfLp118, qmfHp118, hpMelStart3, hpMelLen3, hpMelW3x64, dct12x26);
    return 0;
}

long long sea_wb_rows(long long total_padded_samples) { return total_padded_samples > 0 ? total_padded_samples / SEA_WB_HOP + 1 : 1; }

/* scratch layout: [low band: total / 2 floats][high band: total / 2 floats][raw onset: n_utt ints] */
long long sea_wb_scratch_bytes(long long total_padded_samples, int n_utt)
{
    if (total_padded_samples < 0 || n_utt < 0) return 0;
    return align8(total_padded_samples / 2) * 2 * (long long)sizeof(float) + align8(n_utt) * (long long)sizeof(int);
}

/* both wideband NoiseSup entry points: d_flag_rows != nullptr selects the frame loop that records the speech flags */
static int wb_denoise_launch(const char *who, const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                             const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                             unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                             long long total_padded_samples, int n_utt, void *stream)
{
    if (!d_in || !d_out_lp || !d_offsets || !d_lengths || !d_scratch)
        return fail("%s: input, low-band output, offsets, lengths and scratch are required", who);
    if ((d_hp_rows == nullptr) != (d_code_rows == nullptr)) return fail("%s: the high-band rows and the code rows come together", who);
    if (total_padded_samples < 0 || (total_padded_samples & 7)) return fail("%s: total_padded_samples must be a multiple of 8", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const long long half = align8(total_padded_samples / 2);
    float *lp = static_cast<float *>(d_scratch), *hp = lp + half;
    int *onset = reinterpret_cast<int *>(hp + half);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(onset, 0x7f, (size_t)n_utt * sizeof(int), st)); /* 0x7f7f7f7f: beyond any frame count */
    sea::WbQmfArgs q = {};
    q.in = d_in;
    q.offsets = d_offsets;
    q.lengths = d_lengths;
    q.lp = lp;
    q.hp = hp;
    q.onset = onset;
    q.tables = c->wb;
    q.n_utt = n_utt;
    /* blockIdx.y strides over an utterance's frames: about two frames per workgroup for an utterance of average length */
    long long rows = total_padded_samples / SEA_WB_HOP / n_utt / 2 + 1;
    if (rows > 1024) rows = 1024;
    hipLaunchKernelGGL(sea::wb_qmf_kernel, dim3((unsigned)n_utt, (unsigned)rows), dim3(sea::kWbQmfThreads), 0, st, q);
    HIP_TRY(hipGetLastError());
    sea::NsWbArgs a = {};
    a.b.out = d_out_lp;
    a.b.out_f32 = d_out_f32;
    a.b.offsets = d_offsets;
    a.b.lengths = d_lengths;
    a.b.order = d_order;
    a.b.first_out = d_first_out;
    a.b.onset_out = d_onset;
    a.b.tables = c->ns;
    a.b.n_utt = n_utt;
    a.in_f32 = lp;
    a.onset = onset;
    a.b.flags_out = d_flag_rows;
    if (d_flag_rows)
        hipLaunchKernelGGL(sea::ns_denoise_pipe_wb_fd_kernel, dim3(n_utt), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(sea::ns_denoise_pipe_wb_kernel, dim3(n_utt), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (d_hp_rows) { /* the high band: needs the two QMF streams and the onset only */
        sea::WbHbArgs h = {};
        h.lp = lp;
        h.hp = hp;
        h.offsets = d_offsets;
        h.lengths = d_lengths;
        h.onset = onset;
        h.hp_rows = d_hp_rows;
        h.code_rows = d_code_rows;
        h.ns = c->ns;
        h.wb = c->wb;
        h.n_utt = n_utt;
        /* one wave per workgroup, about two output frames each (eight each: 2.53 ms against 2.43 on the 2048-utterance workload) */
        hipLaunchKernelGGL(sea::wb_hb_kernel, dim3((unsigned)n_utt, (unsigned)rows), dim3(64), 0, st, h);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(sea::wb_specsub_kernel, dim3((unsigned)((n_utt + 63) / 64)), dim3(64), 0, st, h);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int sea_wb_denoise_batch(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                         const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset, float *d_hp_rows,
                         float *d_code_rows, void *d_scratch, long long total_padded_samples, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    return wb_denoise_launch("sea_wb_denoise_batch", d_in, d_out_lp, d_out_f32, d_offsets, d_lengths, d_order, d_first_out, d_onset,
                             nullptr, d_hp_rows, d_code_rows, d_scratch, total_padded_samples, n_utt, stream);
}

int sea_wb_denoise_batch_fd(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                            const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                            unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                            long long total_padded_samples, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_out_f32 || !d_first_out || !d_onset || !d_flag_rows)
        return fail("sea_wb_denoise_batch_fd: the float stream, first_out, onset and the flag rows are all required");
    return wb_denoise_launch("sea_wb_denoise_batch_fd", d_in, d_out_lp, d_out_f32, d_offsets, d_lengths, d_order, d_first_out, d_onset,
                             d_flag_rows, d_hp_rows, d_code_rows, d_scratch, total_padded_samples, n_utt, stream);
}

/* One TIME SLICE of a wideband batch: see include/sea_mi355x.h.  Four launches as in wb_denoise_launch, each the slice form of
 * its kernel; the last one also stores what the next slice starts from. */
static int wb_slice_launch(const char *who, const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                           const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                           unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                           long long total_padded_samples, float *d_state, int n_utt, int frame_base, int resume, void *stream)
{
    if (!d_state) return fail("%s: d_state is required", who);
    if (!d_in || !d_out_lp || !d_offsets || !d_lengths || !d_scratch)
        return fail("%s: input, low-band output, offsets, lengths and scratch are required", who);
    if ((d_hp_rows == nullptr) != (d_code_rows == nullptr)) return fail("%s: the high-band rows and the code rows come together", who);
    if (total_padded_samples < 0 || (total_padded_samples & 7)) return fail("%s: total_padded_samples must be a multiple of 8", who);
    if (frame_base < 0) return fail("%s: frame_base must not be negative", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const long long half = align8(total_padded_samples / 2);
    float *lp = static_cast<float *>(d_scratch), *hp = lp + half;
    int *onset = reinterpret_cast<int *>(hp + half);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(onset, 0x7f, (size_t)n_utt * sizeof(int), st)); /* sea::kWbNoOnset */
    sea::WbSliceArgs w = {};
    w.q.in = d_in;
    w.q.offsets = d_offsets;
    w.q.lengths = d_lengths;
    w.q.lp = lp;
    w.q.hp = hp;
    w.q.onset = onset;
    w.q.tables = c->wb;
    w.q.n_utt = n_utt;
    w.hp_rows = d_hp_rows;
    w.code_rows = d_code_rows;
    w.ns = c->ns;
    w.state = d_state;
    w.frame_base = frame_base;
    w.resume = resume != 0;
    long long rows = total_padded_samples / SEA_WB_HOP / n_utt / 2 + 1; /* as wb_denoise_launch */
    if (rows > 1024) rows = 1024;
    hipLaunchKernelGGL(sea::wb_qmf_slice_kernel, dim3((unsigned)n_utt, (unsigned)rows), dim3(sea::kWbQmfThreads), 0, st, w);
    HIP_TRY(hipGetLastError());
    sea::NsWbArgs a = {};
    a.b.out = d_out_lp;
    a.b.out_f32 = d_out_f32;
    a.b.offsets = d_offsets;
    a.b.lengths = d_lengths;
    a.b.order = d_order;
    a.b.first_out = d_first_out;
    a.b.onset_out = d_onset;
    a.b.tables = c->ns;
    a.b.n_utt = n_utt;
    a.b.state = d_state;
    a.b.resume = resume != 0;
    a.b.frame_base = frame_base;
    a.b.prio_row = (d_order && n_utt > c->n_cu) ? c->n_cu : 0; /* by launch row, as the 8 kHz slices */
    a.in_f32 = lp;
    a.onset = onset;
    a.b.flags_out = d_flag_rows;
    if (d_flag_rows)
        hipLaunchKernelGGL(sea::ns_denoise_pipe_wb_fd_slice_kernel, dim3(n_utt), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(sea::ns_denoise_pipe_wb_slice_kernel, dim3(n_utt), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (d_hp_rows) {
        hipLaunchKernelGGL(sea::wb_hb_slice_kernel, dim3((unsigned)n_utt, (unsigned)rows), dim3(64), 0, st, w);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::wb_slice_end_kernel, dim3((unsigned)n_utt), dim3(128), 0, st, w);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_wb_denoise_batch_slice(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                               const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                               float *d_hp_rows, float *d_code_rows, void *d_scratch, long long total_padded_samples,
                               float *d_state, int n_utt, int frame_base, int resume, void *stream)
{
    if (n_utt <= 0) return 0;
    return wb_slice_launch("sea_wb_denoise_batch_slice", d_in, d_out_lp, d_out_f32, d_offsets, d_lengths, d_order, d_first_out,
                           d_onset, nullptr, d_hp_rows, d_code_rows, d_scratch, total_padded_samples, d_state, n_utt, frame_base,
                           resume, stream);
}

/* the same slice + the speech flags of its output frames: what sea_wb_afe_features_batch_slice reads */
int sea_wb_denoise_batch_slice_fd(const short *d_in, short *d_out_lp, float *d_out_f32, const long long *d_offsets,
                                  const long long *d_lengths, const int *d_order, int *d_first_out, int *d_onset,
                                  unsigned char *d_flag_rows, float *d_hp_rows, float *d_code_rows, void *d_scratch,
                                  long long total_padded_samples, float *d_state, int n_utt, int frame_base, int resume,
                                  void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_out_f32 || !d_first_out || !d_onset || !d_flag_rows || !d_hp_rows || !d_code_rows)
        return fail("sea_wb_denoise_batch_slice_fd: the float stream, first_out, onset, the flag rows, the high-band rows and the "
                    "code rows are all required");
    return wb_slice_launch("sea_wb_denoise_batch_slice_fd", d_in, d_out_lp, d_out_f32, d_offsets, d_lengths, d_order, d_first_out,
                           d_onset, d_flag_rows, d_hp_rows, d_code_rows, d_scratch, total_padded_samples, d_state, n_utt,
                           frame_base, resume, stream);
}

int sea_wb_slice_state_floats(void) { return sea::kWbSliceStateFloats; }

int sea_wb_afe_slice_state_floats(void) { return sea::kWbAfeStateFloats; }

/* The feature chain over one TIME SLICE: see include/sea_mi355x.h.  Two launches as in sea_wb_afe_features_batch, each the slice
 * form of its kernel (afe_slice_kernel.hip); the second one also stores what the next slice starts from. */
int sea_wb_afe_features_batch_slice(const float *d_out_f32, const unsigned char *d_flag_rows, const float *d_hp_rows,
                                    const float *d_code_rows, const long long *d_offsets, const long long *d_lengths,
                                    const int *d_first_out, const int *d_onset, const unsigned char *d_final,
                                    const long long *d_ceps_cum, long long total_ceps, float *d_feat_cc, float *d_feat_pp,
                                    const long long *d_feat_cum, float *d_feat15, int *d_n_feat, int *d_n_ceps, float *d_afe_state,
                                    int n_utt, int frame_base, int resume, void *stream)
{
    const char *who = "sea_wb_afe_features_batch_slice";
    if (n_utt <= 0) return 0;
    if (!d_afe_state) return fail("%s: d_afe_state is required", who);
    if (!d_out_f32 || !d_flag_rows || !d_hp_rows || !d_code_rows || !d_first_out || !d_onset)
        return fail("%s: the float stream, the flag rows, the high-band rows, the code rows, first_out and onset are required", who);
    if (!d_offsets || !d_lengths || !d_ceps_cum || !d_feat_cc || !d_feat_cum || !d_feat15 || !d_n_feat)
        return fail("%s: offsets, lengths, both prefix sums, feat_cc, feat15 and n_feat are required", who);
    if (total_ceps < 0) return fail("%s: total_ceps must not be negative", who);
    if (frame_base < 0) return fail("%s: frame_base must not be negative", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::WbAfeSliceArgs s = {};
    sea::AfeArgs &a = s.w.a;
    afe_args(&a, c, d_out_f32, d_flag_rows, d_offsets, d_lengths, d_first_out, d_onset, d_ceps_cum, d_feat_cc, d_feat_pp, d_feat_cum,
             d_feat15, d_n_feat, d_n_ceps, n_utt);
    s.w.hp_rows = d_hp_rows;
    s.w.code_rows = d_code_rows;
    s.w.wb = c->wb;
    s.final = d_final;
    s.state = d_afe_state;
    s.frame_base = frame_base;
    s.resume = resume != 0;
    if (total_ceps > 0) {
        const long long nslot = total_ceps / 8 + n_utt; /* tile slots of 8 frames, as sea_wb_afe_features_batch */
        constexpr long long kAfeGrid = 8192;
        const long long want = nslot < kAfeGrid ? nslot : kAfeGrid;
        hipLaunchKernelGGL(sea::afe_wb_ceps_slice_kernel, dim3((unsigned)want), dim3(64), 0, (hipStream_t)stream, s);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::afe_wb_vad_slice_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_wb_afe_features_batch(const float *d_out_f32, const unsigned char *d_flag_rows, const float *d_hp_rows,
                              const float *d_code_rows, const long long *d_offsets, const long long *d_lengths,
                              const int *d_first_out, const int *d_onset, const long long *d_ceps_cum, long long total_ceps,
                              float *d_feat_cc, float *d_feat_pp, const long long *d_feat_cum, float *d_feat15, int *d_n_feat,
                              int *d_n_ceps, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (!d_out_f32 || !d_flag_rows || !d_hp_rows || !d_code_rows || !d_first_out || !d_onset)
        return fail("sea_wb_afe_features_batch: the float stream, the flag rows, the high-band rows, the code rows, first_out and onset are required");
    if (!d_offsets || !d_lengths || !d_ceps_cum || !d_feat_cc || !d_feat_cum || !d_feat15 || !d_n_feat)
        return fail("sea_wb_afe_features_batch: offsets, lengths, both prefix sums, feat_cc, feat15 and n_feat are required");
    if (total_ceps < 0) return fail("sea_wb_afe_features_batch: total_ceps must not be negative");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::WbAfeArgs w = {};
    sea::AfeArgs &a = w.a;
    afe_args(&a, c, d_out_f32, d_flag_rows, d_offsets, d_lengths, d_first_out, d_onset, d_ceps_cum, d_feat_cc, d_feat_pp, d_feat_cum,
             d_feat15, d_n_feat, d_n_ceps, n_utt);
    w.hp_rows = d_hp_rows;
    w.code_rows = d_code_rows;
    w.wb = c->wb;
    if (total_ceps > 0) {
        const long long nslot = total_ceps / 8 + n_utt; /* tile slots of 8 frames, as sea_afe_features_batch */
        constexpr long long kAfeGrid = 8192;
        const long long want = nslot < kAfeGrid ? nslot : kAfeGrid;
        hipLaunchKernelGGL(sea::afe_wb_ceps_kernel, dim3((unsigned)want), dim3(64), 0, (hipStream_t)stream, w);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::afe_wb_vad_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_wb_compceps_batch(const float *d_out_f32, const long long *d_offsets, const long long *d_lengths, const int *d_first_out,
                          const float *d_hp_rows, const float *d_code_rows, const long long *d_ceps_cum, long long total_frames,
                          float *d_ceps, int *d_n_ceps, int n_utt, void *stream)
{
    if (n_utt <= 0 || total_frames <= 0) return 0;
    if (!d_out_f32 || !d_first_out || !d_hp_rows || !d_code_rows)
        return fail("sea_wb_compceps_batch: the float stream, first_out, the high-band rows and the code rows are required");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::WbCepsArgs a = {};
    a.c.den_f32 = d_out_f32;
    a.c.offsets = d_offsets;
    a.c.lengths = d_lengths;
    a.c.first_out = d_first_out;
    a.c.ceps_cum = d_ceps_cum;
    a.c.ceps = d_ceps;
    a.c.n_ceps = d_n_ceps;
    a.c.tables = c->cc;
    a.c.n_utt = n_utt;
    a.hp_rows = d_hp_rows;
    a.code_rows = d_code_rows;
    a.wb = c->wb;
    const long long nslot = total_frames / 16 + n_utt; /* tile slots of 16 frames, as sea_compceps_batch */
    const long long grid = nslot < 16384 ? nslot : 16384;
    hipLaunchKernelGGL(sea::compceps_wb_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_wb_denoise(const short *in, long n, short *out_lp)
{
    const long nfr = n > 0 ? n / SEA_WB_HOP : 0;
    if (nfr <= 0) return 0;
    if (!in || !out_lp) return fail("sea_wb_denoise: null buffer");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const long long total = align8(n);
    const long long meta[2] = {0, (long long)n};
    DevBuf<short> d_in, d_out;
    DevBuf<long long> d_meta;
    DevBuf<char> d_scr;
    HIP_TRY(d_in.alloc((size_t)total));
    HIP_TRY(d_out.alloc((size_t)total / 2));
    HIP_TRY(d_meta.alloc(2));
    HIP_TRY(d_scr.alloc((size_t)sea_wb_scratch_bytes(total, 1)));
    HIP_TRY(hipMemcpy(d_in.p, in, (size_t)n * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_meta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    if (sea_wb_denoise_batch(d_in.p, d_out.p, nullptr, d_meta.p, d_meta.p + 1, nullptr, nullptr, nullptr, nullptr, nullptr, d_scr.p, total, 1,
                             nullptr))
        return 1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_lp, d_out.p, (size_t)nfr * SEA_HOP * sizeof(short), hipMemcpyDeviceToHost));
    return 0;
}

int sea_rfft256_batch(const float *d_in, float *d_out, long long nframes, void *stream)
{
    if (nframes <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const long long npair = (nframes + 1) / 2; /* one wave transforms two frames at a time */
    const long long grid = npair < 16LL * c->n_cu ? npair : 16LL * c->n_cu;
    hipLaunchKernelGGL(sea::rfft256_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, d_in,
                       d_out, nframes, &c->ns->fft);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_compceps_frames(const float *d_data201, float *d_coef14, long long nframes, void *stream)
{
    if (nframes <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    const long long ntile = (nframes + 15) / 16; /* one wave per tile of 16 frames (cc_kernel.hip, kCcT) */
    const long long grid = ntile < 8192 ? ntile : 8192;
    hipLaunchKernelGGL(sea::compceps_frames_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream,
                       d_data201, d_coef14, nframes, c->cc);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_compceps_batch(const float *d_den_f32, const long long *d_offsets, const long long *d_lengths,
                       const int *d_first_out, const long long *d_ceps_cum, long long total_frames,
                       float *d_ceps, int *d_n_ceps, int n_utt, void *stream)
{
    if (n_utt <= 0 || total_frames <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::CepsArgs a;
    a.den_f32 = d_den_f32;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.first_out = d_first_out;
    a.ceps_cum = d_ceps_cum;
    a.ceps = d_ceps;
    a.n_ceps = d_n_ceps;
    a.tables = c->cc;
    a.n_utt = n_utt;
    const long long nslot = total_frames / 16 + n_utt; /* tile slots of 16 frames (cc_kernel.hip, kCcT) */
    /* waves of the launch (3072 are resident): 8192 0.63 ms, 13312-24576 0.59-0.61, 3072 (every wave its share of the tiles, all in step) 1.0 */
    constexpr long long kCcGrid = 16384;
    const long long grid = nslot < kCcGrid ? nslot : kCcGrid;
    hipLaunchKernelGGL(sea::compceps_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* The plain CompCeps over one TIME SLICE, both rates: see include/sea_mi355x.h.  Two launches: the tiles of the cepstral frames
 * that complete in the slice (cc_slice_kernel.hip; none where the slice holds no whole frame), then one wave per utterance that
 * writes the slice's counts and the state for the next slice.  The second one always runs: sea_compceps_batch's early return
 * on total_frames <= 0 would leave the counts and the state of a ragged tail's slice unwritten. */
static int cc_slice_launch(const char *who, bool wb, const float *d_f32, const long long *d_offsets, const long long *d_lengths,
                           const int *d_first_out, const float *d_hp_rows, const float *d_code_rows, const long long *d_ceps_cum,
                           long long total_frames, float *d_ceps, int *d_n_ceps, float *d_cc_state, int n_utt, int frame_base,
                           int resume, void *stream)
{
    if (!d_cc_state) return fail("%s: d_cc_state is required", who);
    if (!d_f32 || !d_first_out) return fail("%s: the float stream and first_out are required", who);
    if (wb && (!d_hp_rows || !d_code_rows)) return fail("%s: the high-band rows and the code rows are required", who);
    if (!d_offsets || !d_lengths || !d_ceps_cum || !d_ceps || !d_n_ceps)
        return fail("%s: offsets, lengths, the prefix sums, ceps and n_ceps are required", who);
    if (total_frames < 0) return fail("%s: total_frames must not be negative", who);
    if (frame_base < 0) return fail("%s: frame_base must not be negative", who);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::CcSliceArgs s = {};
    s.c.den_f32 = d_f32;
    s.c.offsets = d_offsets;
    s.c.lengths = d_lengths;
    s.c.first_out = d_first_out;
    s.c.ceps_cum = d_ceps_cum;
    s.c.ceps = d_ceps;
    s.c.n_ceps = d_n_ceps;
    s.c.tables = c->cc;
    s.c.n_utt = n_utt;
    s.hp_rows = wb ? d_hp_rows : nullptr;
    s.code_rows = wb ? d_code_rows : nullptr;
    s.wb = c->wb;
    s.state = d_cc_state;
    s.stride = wb ? sea::kWbCcStateFloats : sea::kCcStateFloats;
    s.frame_base = frame_base;
    s.resume = resume != 0;
    if (total_frames > 0) {
        const long long nslot = total_frames / 16 + n_utt; /* tile slots of 16 frames, as sea_compceps_batch */
        const long long grid = nslot < 16384 ? nslot : 16384;
        if (wb)
            hipLaunchKernelGGL(sea::compceps_wb_slice_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, s);
        else
            hipLaunchKernelGGL(sea::compceps_slice_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, s);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sea::compceps_carry_slice_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_compceps_batch_slice(const float *d_den_f32, const long long *d_offsets, const long long *d_lengths,
                             const int *d_first_out, const long long *d_ceps_cum, long long total_frames, float *d_ceps,
                             int *d_n_ceps, float *d_cc_state, int n_utt, int frame_base, int resume, void *stream)
{
    if (n_utt <= 0) return 0;
    return cc_slice_launch("sea_compceps_batch_slice", false, d_den_f32, d_offsets, d_lengths, d_first_out, nullptr, nullptr,
                           d_ceps_cum, total_frames, d_ceps, d_n_ceps, d_cc_state, n_utt, frame_base, resume, stream);
}

int sea_cc_slice_state_floats(void) { return sea::kCcStateFloats; }

int sea_wb_compceps_batch_slice(const float *d_out_f32, const long long *d_offsets, const long long *d_lengths,
                                const int *d_first_out, const float *d_hp_rows, const float *d_code_rows,
                                const long long *d_ceps_cum, long long total_frames, float *d_ceps, int *d_n_ceps,
                                float *d_cc_state, int n_utt, int frame_base, int resume, void *stream)
{
    if (n_utt <= 0) return 0;
    return cc_slice_launch("sea_wb_compceps_batch_slice", true, d_out_f32, d_offsets, d_lengths, d_first_out, d_hp_rows,
                           d_code_rows, d_ceps_cum, total_frames, d_ceps, d_n_ceps, d_cc_state, n_utt, frame_base, resume, stream);
}

int sea_wb_cc_slice_state_floats(void) { return sea::kWbCcStateFloats; }

int etsi_denoise(short *p_data, short *p_denoised, long i_frame)
{
    const short *in[1] = {p_data};
    short *out[1] = {p_denoised};
    long len[1] = {i_frame};
    if (sea_denoise_utterances(in, out, len, 1)) {
        fprintf(stderr, "ERROR:   etsi_denoise (MI355X): %s\r\n", last_error());
        return 1; /* TRUE == fault, AdvFrontEnd.c:207-209 */
    }
    return 0;
}

int etsi_denoise_synchronization(short *p_data, short *p_denoised, long i_frame)
{ /* AdvFrontEnd.c:213-226: copies out only when etsi_denoise reports a fault */
    std::vector<short> tmp((size_t)(i_frame > 0 ? i_frame : 1));
    (void)p_denoised;
    return etsi_denoise(p_data, tmp.data(), i_frame);
}

int etsi_denoise_16k(short *p_data, short *p_denoised, long i_frame)
{
    (void)p_data;
    (void)p_denoised;
    (void)i_frame;
    fprintf(stderr, "ERROR:   etsi_denoise_16k: the reference's 16 kHz mode is defective (heap over-read) and is not provided\r\n");
    return fail("etsi_denoise_16k is not provided");
}

int etsi_denoise_16k_synchronization(short *p_data, short *p_denoised, long i_frame)
{ /* AdvFrontEnd.c:316-329 calls the 8 kHz-mode etsi_denoise, exactly like the non-16k twin */
    return etsi_denoise_synchronization(p_data, p_denoised, i_frame);
}

/* nframes transforms rfft (x, n, m) in place on device memory: [nframes][n] floats.  (256, 8) -- the hot path's size --
 * runs the streaming kernel; every other size the reference's routine takes (n = 2^q <= 16384, 2^m <= n;
 * etsi/cpp/rfft.c:45-180) the one-workgroup schedule walker.  The schedule of a size is built once per device. */
int sea_rfft_batch(float *d_x, int n, int m, long long nframes, void *stream)
{
    if (nframes <= 0) return 0;
    if (n == 256 && m == 8) return sea_rfft256_batch(d_x, d_x, nframes, stream);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    struct Sched {
        int device, n, m;
        unsigned *d;
    };
    static std::mutex mu;
    static std::vector<Sched> cache;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    unsigned *d_sched = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const Sched &e : cache)
            if (e.device == dev && e.n == n && e.m == m) d_sched = e.d;
        if (!d_sched) {
            unsigned long words = 0;
            unsigned *h = sea_rfft_schedule(n, m, &words);
            if (!h) return fail("rfft: size n=%d, m=%d is outside what etsi/cpp/rfft.c:45-180 can take here (n a power of two <= %d, 2^m <= n)", n, m, (int)SEA_RFFT_MAXN);
            hipError_t e = hipMalloc((void **)&d_sched, words * sizeof(unsigned));
            if (e == hipSuccess) e = hipMemcpy(d_sched, h, words * sizeof(unsigned), hipMemcpyHostToDevice);
            free(h);
            if (e != hipSuccess) {
                if (d_sched) (void)hipFree(d_sched);
                return fail("rfft: schedule upload: %s", hipGetErrorString(e));
            }
            cache.push_back(Sched{dev, n, m, d_sched});
        }
    }
    const long long grid = nframes < 8LL * c->n_cu ? nframes : 8LL * c->n_cu;
    hipLaunchKernelGGL(sea::rfft_any_kernel, dim3((unsigned)grid), dim3(256), (size_t)n * sizeof(float), (hipStream_t)stream, d_x,
                       d_sched, nframes);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* etsi/cpp/rfft.h:19.  The reference's routine returns nothing and cannot fail; here a size it could not take either
 * (n not a power of two: its digit-reverse counter does not terminate properly; 2^m > n: it indexes past x) or that does
 * not fit this engine (n > 16384), or a missing device, leaves x UNTOUCHED, prints the reason to stderr and sets
 * sea_last_error() -- it no longer abort()s the caller's process. */
void rfft(float *x, int n, int m)
{
    if (!x || n < 2) return;
    DevBuf<float> d;
    const size_t bytes = (size_t)n * sizeof(float);
    bool ok = d.alloc((size_t)n) == hipSuccess && hipMemcpy(d.p, x, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = sea_rfft_batch(d.p, n, m, 1, nullptr) == 0;
    else fail("rfft: no usable gfx950 device or allocation failure");
    if (ok) ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(x, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) fprintf(stderr, "ERROR:   rfft (MI355X): n=%d, m=%d not transformed: %s\r\n", n, m, last_error());
}

int sea_compceps_frame(const float *Data, float *Coef14)
{
    DevBuf<float> din, dout;
    HIP_TRY(din.alloc(201));
    HIP_TRY(dout.alloc(14));
    HIP_TRY(hipMemcpy(din.p, Data - 1, 201 * sizeof(float), hipMemcpyHostToDevice));
    if (sea_compceps_frames(din.p, dout.p, 1, nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(Coef14, dout.p, 14 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

/* ------------------------------------------------------------------------------------------- */
long long sea_resynth_scratch_bytes(long long total_padded_samples, int n_utt)
{ /* [sample][64] floats, plus 8 time steps per utterance for rounding up to whole 16-step tiles */
    return (total_padded_samples + 8LL * (n_utt > 0 ? n_utt : 0)) * 64 * (long long)sizeof(float);
}

int sea_resynth64_batch(const short *d_in, short *d_out, const long long *d_offsets,
                        const long long *d_lengths, const float *d_mask,
                        const long long *d_mask_offsets, float *d_inter, const int *d_order,
                        int n_utt, int binary, void *stream)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::ResynthArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.mask = d_mask;
    a.mask_offsets = d_mask_offsets;
    a.inter = d_inter;
    a.order = d_order;
    a.tables = c->gt;
    a.n_utt = n_utt;
    a.binary = binary;
    /* both passes of an utterance in one workgroup */
    hipLaunchKernelGGL(sea::resynth_fused_kernel, dim3(n_utt), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_resynth64(const short *in, long L, const float *mask, int F, int binary, short *out)
{
    const long minL = (binary & 2) ? 160 : 320;
    if (L < minL) return fail("resynth64: L=%ld is shorter than %ld samples", L, minL);
    if (F != (int)((binary & 2) ? L / 160 : (L - 320) / 160 + 1)) return fail("resynth64: F=%d does not match L=%ld", F, L);
    const long long Lp = align8(L);
    DevBuf<short> din, dout;
    DevBuf<float> dmask, dinter;
    DevBuf<long long> dmeta;
    HIP_TRY(din.alloc((size_t)Lp));
    HIP_TRY(dout.alloc((size_t)Lp));
    HIP_TRY(dmask.alloc((size_t)F * 64));
    HIP_TRY(dinter.alloc((size_t)sea_resynth_scratch_bytes(Lp, 1) / sizeof(float)));
    HIP_TRY(dmeta.alloc(3));
    const long long meta[3] = {0, L, 0};
    HIP_TRY(hipMemcpy(din.p, in, (size_t)L * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmask.p, mask, (size_t)F * 64 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmeta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    if (sea_resynth64_batch(din.p, dout.p, dmeta.p, dmeta.p + 1, dmask.p, dmeta.p + 2, dinter.p, nullptr, 1,
                            binary, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)L * sizeof(short), hipMemcpyDeviceToHost));
    return 0;
}

int sea_subband64_batch(const short *d_in, short *d_out, const long long *d_offsets, const long long *d_lengths,
                        const int *d_order, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::SubbandArgs a;
    a.in = d_in;
    a.out = d_out;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.order = d_order;
    a.tables = c->gt;
    a.n_utt = n_utt;
    hipLaunchKernelGGL(sea::subband_kernel, dim3(n_utt), dim3(384), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_subband64(const short *in, long L, short *out)
{
    if (L <= 0) return fail("subband64: L=%ld", L);
    const long long Lp = align8(L);
    DevBuf<short> din, dout;
    DevBuf<long long> dmeta;
    HIP_TRY(din.alloc((size_t)Lp));
    HIP_TRY(dout.alloc((size_t)Lp * 64));
    HIP_TRY(dmeta.alloc(2));
    const long long meta[2] = {0, L};
    HIP_TRY(hipMemcpy(din.p, in, (size_t)L * sizeof(short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmeta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    if (sea_subband64_batch(din.p, dout.p, dmeta.p, dmeta.p + 1, nullptr, 1, nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy2D(out, (size_t)L * sizeof(short), dout.p, (size_t)Lp * sizeof(short), (size_t)L * sizeof(short), 64,
                        hipMemcpyDeviceToHost));
    return 0;
}

int sea_irm_target_batch(const short *d_pure64, const short *d_noise64, const long long *d_offsets, const long long *d_lengths,
                         const long long *d_row_offsets, float *d_irm, int window, int n_utt, void *stream)
{
    if (n_utt <= 0) return 0;
    if (window < 0 || window > 2) return fail("irm_target: window %d (0 rectangular, 1 Hamming, 2 Hanning)", window);
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::IrmArgs a;
    a.pure = d_pure64;
    a.noise = d_noise64;
    a.offsets = d_offsets;
    a.lengths = d_lengths;
    a.row_offsets = d_row_offsets;
    a.irm = d_irm;
    a.fft = &c->ns->fft;
    a.n_utt = n_utt;
    a.window = window;
    hipLaunchKernelGGL(sea::irm_target_kernel, dim3((unsigned)n_utt * 64u), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_irm_target(const short *pure64, const short *noise64, long L, int window, float *irm)
{
    if (L < 320) return fail("irm_target: L=%ld is shorter than one 320-sample frame", L);
    const long long Lp = align8(L), F = (L - 320) / 160 + 1;
    DevBuf<short> dp, dn;
    DevBuf<float> dirm;
    DevBuf<long long> dmeta;
    HIP_TRY(dp.alloc((size_t)Lp * 64));
    HIP_TRY(dn.alloc((size_t)Lp * 64));
    HIP_TRY(dirm.alloc((size_t)F * 64));
    HIP_TRY(dmeta.alloc(3));
    const long long meta[3] = {0, L, 0};
    HIP_TRY(hipMemcpy2D(dp.p, (size_t)Lp * sizeof(short), pure64, (size_t)L * sizeof(short), (size_t)L * sizeof(short), 64,
                        hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy2D(dn.p, (size_t)Lp * sizeof(short), noise64, (size_t)L * sizeof(short), (size_t)L * sizeof(short), 64,
                        hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmeta.p, meta, sizeof meta, hipMemcpyHostToDevice));
    if (sea_irm_target_batch(dp.p, dn.p, dmeta.p, dmeta.p + 1, dmeta.p + 2, dirm.p, window, 1, nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(irm, dirm.p, (size_t)F * 64 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_gammatone_filter(const float *input, float *output, int chan, long sigLength)
{
    if (chan < 0 || chan >= 64) return fail("gammatone: channel %d out of range", chan);
    if (sigLength <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> din, dout;
    HIP_TRY(din.alloc((size_t)sigLength));
    HIP_TRY(dout.alloc((size_t)sigLength));
    HIP_TRY(hipMemcpy(din.p, input, (size_t)sigLength * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::gammatone_kernel, dim3(1), dim3(64), 0, nullptr, din.p, dout.p, chan,
                       (long long)sigLength, c->gt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(output, dout.p, (size_t)sigLength * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

/* ------------------------------------------------------------------------------------------- */
struct sea_ns_stream {
    float *state = nullptr;  /* kNsStateFloats, device */
    float *h_io = nullptr;   /* pinned, device-visible: 80 in | 80 out | produced flag -- the kernel reads and writes it
                              * over PCIe (324 B per push), so a push is ONE launch and ONE stream wait, no copy calls */
    float *d_io = nullptr;   /* the device's address of h_io */
    hipStream_t stream = nullptr;
    int fresh = 1;
};

sea_ns_stream *sea_ns_stream_alloc(void)
{ /* DoNoiseSupAlloc, NoiseSup.c:859-868: NULL on allocation failure */
    sea_ns_stream *s = new (std::nothrow) sea_ns_stream();
    if (!s) return nullptr;
    if (hipMalloc(&s->state, sea::kNsStateFloats * sizeof(float)) != hipSuccess ||
        hipHostMalloc((void **)&s->h_io, 164 * sizeof(float), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->d_io, s->h_io, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        fail("sea_ns_stream_alloc: device allocation failed");
        sea_ns_stream_delete(s);
        return nullptr;
    }
    return s;
}

void sea_ns_stream_init(sea_ns_stream *s)
{ /* DoNoiseSupInit, NoiseSup.c:884-1009: the next push starts from the initial state */
    if (s) s->fresh = 1;
}

int sea_ns_stream_push(sea_ns_stream *s, const float *in80, float *out80)
{
    DeviceCtx *c;
    if (!s || ctx(&c)) {
        fprintf(stderr, "ERROR:   DoNoiseSup (MI355X): %s\r\n", s ? last_error() : "NULL stream");
        exit(1); /* the reference's DoNoiseSup path ends the process on failure (NoiseSup.c:983-987: exit(0));
                  * a device fault must not look like success to the caller's shell, so the status is non-zero */
    }
    sea::NsStreamArgs a = {};
    a.in = s->d_io;
    a.out = s->d_io + 80;
    a.produced = reinterpret_cast<int *>(s->d_io + 160);
    a.state = s->state;
    a.tables = c->ns;
    a.nframes = 1;
    a.reset = s->fresh;
    memcpy(s->h_io, in80, 80 * sizeof(float));
    hipLaunchKernelGGL(sea::ns_stream_kernel, dim3(1), dim3(64), 0, s->stream, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
        fprintf(stderr, "ERROR:   DoNoiseSup (MI355X): device failure\r\n");
        exit(1);
    }
    const int produced = *reinterpret_cast<const volatile int *>(s->h_io + 160);
    if (produced) memcpy(out80, s->h_io + 80, 80 * sizeof(float));
    s->fresh = 0;
    return produced;
}

void sea_ns_stream_delete(sea_ns_stream *s)
{
    if (!s) return;
    if (s->state) (void)hipFree(s->state);
    if (s->h_io) (void)hipHostFree(s->h_io);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

/* batched form of the above on device pointers: B streams x nframes frames */
int sea_ns_streams_push(const float *d_in, float *d_out, int *d_produced, float *d_state, int n_streams,
                        int nframes, int reset, void *stream)
{
    if (n_streams <= 0 || nframes <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsStreamArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.produced = d_produced;
    a.state = d_state;
    a.tables = c->ns;
    a.nframes = nframes;
    a.reset = reset;
    hipLaunchKernelGGL(sea::ns_stream_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_ns_streams_push_fd(const float *d_in, float *d_out, int *d_produced, unsigned char *d_flags,
                           int *d_frame_counter, float *d_state, int n_streams, int nframes, int reset, void *stream)
{
    if (n_streams <= 0 || nframes <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::NsStreamArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.produced = d_produced;
    a.state = d_state;
    a.tables = c->ns;
    a.nframes = nframes;
    a.reset = reset;
    a.flags = d_flags;
    a.frame_counter = d_frame_counter;
    hipLaunchKernelGGL(sea::ns_stream_fd_kernel, dim3(n_streams), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_ns_state_floats(void) { return sea::kNsStateFloats; }

/* ---- the 16 k-native variant (ns16k_pipe_kernel.hip) ---- */
int sea_ns16k_streams_push(const float *d_in, float *d_out, int *d_produced, unsigned char *d_flags, int *d_frame_counter,
                           float *d_wiener, float *d_state, int n_streams, int nframes, int reset, void *stream)
{
    if (n_streams <= 0 || nframes <= 0) return 0;
    if (!d_in || !d_out || !d_produced || !d_state) return fail("sea_ns16k_streams_push: NULL buffer");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    sea::Ns16StreamArgs a = {};
    a.in = d_in;
    a.out = d_out;
    a.produced = d_produced;
    a.flags = d_flags;
    a.frame_counter = d_frame_counter;
    a.wiener = d_wiener;
    a.state = d_state;
    a.tables = c->ns16;
    a.nframes = nframes;
    a.reset = reset;
    a.n_streams = n_streams;
    /* four pipelined waves per stream (round 3's one-wave-per-stream form was removed after measurement, source at 24082b1:
     * 54 against 181 M frames/s at 1024 x 400, profiles/r03_ns16k_time.txt / r04_ns16k_time.txt) */
    constexpr int G = sea::kNs16PipeStreamsPerGroup;
    hipLaunchKernelGGL(sea::ns16k_pipe_kernel, dim3((n_streams + G - 1) / G), dim3(256 * G), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sea_ns16k_state_floats(void) { return sea::kNs16StateFloats; }

/* the 16 k-native variant's transform, DoGamma and DoGammaIDCT on the device, piece by piece (host pointers): see
 * ns16k_selftest_kernel; fft512_a / _b: [nfft][512], gamma25: [ngain][25], idct9: [ngain][9] (rows 0..8, before the window) */
int sea_selftest_ns16k_pieces(const float *frames512, int nfft, float *fft512_a, float *fft512_b, const float *gains129, int ngain,
                              float *gamma25, float *idct9)
{
    if (nfft < 0 || ngain < 0) return fail("sea_selftest_ns16k_pieces: negative count");
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> dfr, da, db, dg, dgam, did;
    HIP_TRY(dfr.alloc((size_t)(nfft > 0 ? nfft : 1) * 512));
    HIP_TRY(da.alloc((size_t)(nfft > 0 ? nfft : 1) * 512));
    HIP_TRY(db.alloc((size_t)(nfft > 0 ? nfft : 1) * 512));
    HIP_TRY(dg.alloc((size_t)(ngain > 0 ? ngain : 1) * 129));
    HIP_TRY(dgam.alloc((size_t)(ngain > 0 ? ngain : 1) * 25));
    HIP_TRY(did.alloc((size_t)(ngain > 0 ? ngain : 1) * 9));
    if (nfft) HIP_TRY(hipMemcpy(dfr.p, frames512, (size_t)nfft * 512 * sizeof(float), hipMemcpyHostToDevice));
    if (ngain) HIP_TRY(hipMemcpy(dg.p, gains129, (size_t)ngain * 129 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::ns16k_selftest_kernel, dim3(1), dim3(64), 0, nullptr, c->ns16, dfr.p, nfft, da.p, db.p, dg.p, ngain, dgam.p, did.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (nfft) {
        HIP_TRY(hipMemcpy(fft512_a, da.p, (size_t)nfft * 512 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(fft512_b, db.p, (size_t)nfft * 512 * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (ngain) {
        HIP_TRY(hipMemcpy(gamma25, dgam.p, (size_t)ngain * 25 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(idct9, did.p, (size_t)ngain * 9 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}

int sea_ns16k_tables_host(float *sigWindow480, float *irWindow17, int *gammaStart25, float *gamma25x128, float *idct25x25)
{
    sea_ns16k_plain_tables(sigWindow480, irWindow17, gammaStart25, gamma25x128, idct25x25);
    return 0;
}

/* ------------------------------------------------------------------------------------------- */
int sea_selftest_pi4(unsigned long long *n_mismatch)
{
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<unsigned long long> d;
    HIP_TRY(d.alloc(1));
    HIP_TRY(hipMemset(d.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(sea::selftest_pi4_kernel, dim3(4096), dim3(256), 0, nullptr, d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(n_mismatch, d.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_div(unsigned long long *out2)
{
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<unsigned long long> d;
    HIP_TRY(d.alloc(2));
    HIP_TRY(hipMemset(d.p, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(sea::selftest_div_kernel, dim3(4096), dim3(256), 0, nullptr, c->gt, d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out2, d.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_nsdiv(unsigned long long *out4)
{
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<unsigned long long> d;
    HIP_TRY(d.alloc(4));
    HIP_TRY(hipMemset(d.p, 0, 4 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(sea::selftest_nsdiv_kernel, dim3(4096), dim3(256), 0, nullptr, d.p, 1024);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out4, d.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_dc(const float *dif, const float *y0, float *out, int *fellback, int ncases)
{
    if (ncases <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> dd, dy, dout;
    DevBuf<int> df;
    HIP_TRY(dd.alloc((size_t)ncases * 80));
    HIP_TRY(dy.alloc(ncases));
    HIP_TRY(dout.alloc((size_t)ncases * 80));
    HIP_TRY(df.alloc(ncases));
    HIP_TRY(hipMemcpy(dd.p, dif, (size_t)ncases * 80 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy.p, y0, ncases * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::selftest_dc_kernel, dim3(ncases < 1024 ? ncases : 1024), dim3(64), 0, nullptr, dd.p, dy.p,
                       dout.p, df.p, ncases);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)ncases * 80 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fellback, df.p, ncases * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log(const float *x, double *ln_out, int n)
{
    if (n <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> dx;
    DevBuf<double> dout;
    HIP_TRY(dx.alloc(n));
    HIP_TRY(dout.alloc(n));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::selftest_log_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dx.p, dout.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ln_out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log_dd(const double *x, double *hi, double *lo, int n)
{
    if (n <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<double> dx, dhi, dlo;
    HIP_TRY(dx.alloc(n));
    HIP_TRY(dhi.alloc(n));
    HIP_TRY(dlo.alloc(n));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::selftest_log_dd_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dx.p, dhi.p, dlo.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hi, dhi.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lo, dlo.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log_sites(const float *x, float *site1, float *site2, int n)
{
    if (n <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> dx, d1, d2;
    HIP_TRY(dx.alloc(n));
    HIP_TRY(d1.alloc(n));
    HIP_TRY(d2.alloc(n));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::selftest_log_sites_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dx.p, d1.p, d2.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(site1, d1.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(site2, d2.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log_nonfinite(const float *x, float *site1, float *site2, float *logf, int n)
{
    if (n <= 0) return 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<float> dx, d1, d2, d3;
    HIP_TRY(dx.alloc(n));
    HIP_TRY(d1.alloc(n));
    HIP_TRY(d2.alloc(n));
    HIP_TRY(d3.alloc(n));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sea::selftest_log_nonfinite_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dx.p, d1.p, d2.p, d3.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(site1, d1.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(site2, d2.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(logf, d3.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log_guard(int site, unsigned long long *stats8, float *hits3, int cap)
{
    if (site != 1 && site != 2) return fail("selftest_log_guard: site must be 1 or 2");
    if (cap < 0) cap = 0;
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<unsigned long long> ds;
    DevBuf<float> dh;
    HIP_TRY(ds.alloc(8));
    HIP_TRY(dh.alloc((size_t)3 * (cap > 0 ? cap : 1)));
    HIP_TRY(hipMemset(ds.p, 0, 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(dh.p, 0, (size_t)3 * (cap > 0 ? cap : 1) * sizeof(float)));
    hipLaunchKernelGGL(sea::selftest_log_guard_kernel, dim3(4096), dim3(256), 0, nullptr, site, ds.p, dh.p, cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(stats8, ds.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (cap > 0 && hits3) HIP_TRY(hipMemcpy(hits3, dh.p, (size_t)3 * cap * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int sea_selftest_log_lanes(int all_vad, unsigned long long *stats8)
{
    DeviceCtx *c;
    if (ctx(&c)) return 1;
    DevBuf<unsigned long long> ds;
    HIP_TRY(ds.alloc(8));
    HIP_TRY(hipMemset(ds.p, 0, 8 * sizeof(unsigned long long)));
    if (all_vad)
        hipLaunchKernelGGL(sea::selftest_log_lanes_kernel<true>, dim3(4096), dim3(256), 0, nullptr, ds.p);
    else
        hipLaunchKernelGGL(sea::selftest_log_lanes_kernel<false>, dim3(4096), dim3(256), 0, nullptr, ds.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(stats8, ds.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
