/*
 * hostpipe.hip -- the host-buffer batch entry points as a copy / compute pipeline.
 *
 *   sea_denoise_utterances   what etsi/cpp/main.cpp:43-67 does per file (read, etsi_denoise, write) and
 *                            function/20141106_speech_enhancement/aurora_speech_enhancement/aurora_speech_enhancement.cpp:25-80
 *                            does from a thread pool, for a whole list of utterances in host memory
 *   sea_resynth_utterances   the same for resynth() (resyth_64sub_ori/cpp/main.cpp:84-145)
 *
 * PCIe is the slow link of these entry points (160 B per NoiseSup frame each way against 320 B of HBM traffic
 * on the device), so the list is cut into pieces that travel down a pipeline:
 *
 *   pool threads   pack piece k+1 into pinned staging            | unpack piece k-1 into the caller's buffers
 *   copy engines   H2D piece k+1                                 | D2H piece k-1
 *   device         kernel over piece k
 *
 * NoiseSup (sea_denoise_utterances) and the wideband mode (sea_wb_denoise_utterances): the pieces are TIME SLICES of the
 * whole list -- frames [B_k, B_k+1) of every utterance, one launch per slice, the recursion carried in a state blob per
 * utterance.  A launch over whole utterances lasts as long as its longest utterance's chain of frames whatever its size; a
 * slice lasts as long as its own frames.  Resynthesis (sea_resynth_utterances; its second pass runs backwards over the
 * utterance) and SEA_HOST_MODE=chunks: the pieces are chunks of whole utterances, sorted longest first, one launch per chunk
 * on its own part of ONE device buffer.  Results do not depend on either cut.
 *
 * NoiseSup + the plain CompCeps (sea_denoise_ceps_utterances where the plan cuts the list, sea_wb_denoise_ceps_utterances) and the
 * feature chains (sea_features_utterances, sea_wb_features_utterances) ride the same slices: per slice the denoiser's slice call
 * and the cepstrum's or the chain's on the kernel stream, the float stream on the device sized for one slice.
 *
 * What the entry points share lives once: the cut along the time axis and the in-order placement of emitted rows in
 * slice_plan.h (the cut is also sea_packed_plan's), the event-driven loop in run_pipeline, the NoiseSup launch over a slice in
 * ns_launch_slice, and for the six calls over time slices everything but the kernels in run_slices: staging layout, packing,
 * the three streams, upload / record / wait, the audio download, the unpacking tasks and the lifetime of what those tasks
 * read.  Such an entry point is its argument checks, its "too small to cut" rule, its buffer sizes and three callables: launch,
 * extra_download, unpack_piece.  The feature chains are features_slices<WB>, the cepstrum pipelines denoise_ceps_slices<WB>.
 * The chunk pipelines (SEA_HOST_MODE=chunks, resynthesis) and sea_packed_denoise sit on run_pipeline / the events directly.
 * Staging, device buffers, streams and events are grow-only and belong to the calling host thread (the reference's
 * batch tool calls etsi_denoise from N threads); the packing threads are one pool per device.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "capi_internal.h"
#include "slice_plan.h"

using namespace sea_capi;

namespace {

/* ---- packing threads ------------------------------------------------------------------------------ */
/* One pool PER DEVICE (round 4): one device keeps eight packing threads busy, so a process-wide pool of
 * eight capped the file drivers' device threads at one device's worth of packing on an 8-GPU node.  A pool is created by
 * the first host thread that runs a pipeline on that device -- never from a static constructor, and without a HIP call:
 * the device index comes from the caller's PipeWs -- and host threads that share a device (SEA_DEVICES=3 on one GPU) share
 * its pool.  SEA_HOST_THREADS = threads per device (default min(8, (cores - 1) / devices in use so far), at least 2). */
class Pool {
  public:
    static constexpr int kMaxDev = 64;
    static Pool &get(int device)
    {
        static std::mutex m;
        static Pool *pools[kMaxDev] = {};
        static int n_pools = 0;
        const int d = (device >= 0 && device < kMaxDev) ? device : 0;
        std::lock_guard<std::mutex> lk(m);
        if (!pools[d]) pools[d] = new Pool(++n_pools); /* lives until process exit: its threads block on the queue */
        return *pools[d];
    }
    int size() const { return (int)th_.size(); }
    void submit(std::function<void()> f)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }

  private:
    explicit Pool(int n_pools_now)
    {
        int n = 0;
        if (const char *e = getenv("SEA_HOST_THREADS")) n = atoi(e);
        if (n <= 0) {
            const unsigned hw = std::thread::hardware_concurrency();
            n = hw > 2 ? (int)std::min(8u, std::max(2u, (hw - 1) / (unsigned)n_pools_now)) : 1;
        }
        for (int i = 0; i < n; ++i) th_.emplace_back([this] { run(); });
    }
    ~Pool()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return; /* stop requested and nothing left */
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool stop_ = false;
};

/* memcpy for the packing threads: the destination (pinned staging the copy engine reads next, or the caller's output
 * buffer) is not read again by this core, so it is written with non-temporal stores -- no read-for-ownership of the
 * destination lines, a third less memory traffic than memcpy's cached stores at these sizes (pieces of ~16 KB, far
 * below glibc's non-temporal threshold).  SEA_HOST_NT=0 switches back to memcpy. */
#if defined(__x86_64__)
#include <emmintrin.h>
inline bool use_nt()
{
    static const bool v = [] {
        const char *e = getenv("SEA_HOST_NT");
        return !(e && e[0] == '0');
    }();
    return v;
}
inline void copy_stream(void *dst, const void *src, size_t n)
{
    if (n < 256 || !use_nt()) {
        memcpy(dst, src, n);
        return;
    }
    char *d = (char *)dst;
    const char *s = (const char *)src;
    const size_t head = (16 - ((uintptr_t)d & 15)) & 15;
    if (head) {
        memcpy(d, s, head);
        d += head;
        s += head;
        n -= head;
    }
    const size_t blocks = n / 64;
    for (size_t i = 0; i < blocks; ++i, d += 64, s += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i *)s), b = _mm_loadu_si128((const __m128i *)(s + 16));
        const __m128i c = _mm_loadu_si128((const __m128i *)(s + 32)), e = _mm_loadu_si128((const __m128i *)(s + 48));
        _mm_stream_si128((__m128i *)d, a);
        _mm_stream_si128((__m128i *)(d + 16), b);
        _mm_stream_si128((__m128i *)(d + 32), c);
        _mm_stream_si128((__m128i *)(d + 48), e);
    }
    n -= blocks * 64;
    if (n) memcpy(d, s, n);
}
inline void copy_fence() { _mm_sfence(); }
#else
inline void copy_stream(void *dst, const void *src, size_t n) { memcpy(dst, src, n); }
inline void copy_fence() {}
#endif

/* counts outstanding tasks; wait() returns when all are done */
struct Latch {
    std::mutex m;
    std::condition_variable cv;
    int pending = 0;
    void add(int n)
    {
        std::lock_guard<std::mutex> lk(m);
        pending += n;
    }
    void done()
    {
        std::lock_guard<std::mutex> lk(m);
        if (--pending == 0) cv.notify_all();
    }
    bool ready()
    {
        std::lock_guard<std::mutex> lk(m);
        return pending == 0;
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [this] { return pending == 0; });
    }
    template <class Rep, class Period>
    bool wait_for(std::chrono::duration<Rep, Period> d)
    {
        std::unique_lock<std::mutex> lk(m);
        return cv.wait_for(lk, d, [this] { return pending == 0; });
    }
};

/* copies [j0, j1) of a job list on the pool (or inline when the job is small), cut into ~1 MB tasks; `piece` (may be null)
 * and `all` count the tasks */
template <class Copy>
void run_copies(Pool &pool, int j0, int j1, const long long *bytes_prefix, Latch *piece, Latch *all, bool inline_, Copy copy)
{
    if (j0 >= j1) return;
    if (inline_) {
        for (int j = j0; j < j1; ++j) copy(j);
        copy_fence();
        return;
    }
    const long long kTask = 1 << 20;
    int a = j0;
    while (a < j1) {
        int b = a + 1;
        while (b < j1 && bytes_prefix[b] - bytes_prefix[a] < kTask) ++b;
        if (piece) piece->add(1);
        all->add(1);
        pool.submit([=] {
            for (int j = a; j < b; ++j) copy(j);
            copy_fence(); /* non-temporal stores are visible to the copy engine / the caller before the task counts as done */
            if (piece) piece->done();
            all->done();
        });
        a = b;
    }
}

/* ---- per-thread workspace -------------------------------------------------------------------------- */
constexpr int kMaxStreams = 8;
int n_streams()
{
    static const int n = [] {
        const char *e = getenv("SEA_HOST_STREAMS");
        const int v = e ? atoi(e) : 4;
        return v < 1 ? 1 : (v > kMaxStreams ? kMaxStreams : v);
    }();
    return n;
}
#define kStreams n_streams()
constexpr int kMaxChunks = 64; /* pieces of one call: the workspace has that many events of each kind */
static_assert(kMaxSlices <= kMaxChunks, "a time slice is a piece");

template <class T>
struct Grow { /* a pinned and a device buffer, grow-only, each with a capacity of its own: a user may need only one half */
    T *h = nullptr, *d = nullptr;
    size_t hcap = 0, dcap = 0;
    Grow() = default;
    Grow(const Grow &) = delete;
    Grow &operator=(const Grow &) = delete;
    ~Grow() { release(); }
    void release()
    {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr;
        hcap = dcap = 0;
    }
    static size_t roomy(size_t n) { return n + n / 4 + 4096; }
    hipError_t ensure_host(size_t n, unsigned flags = hipHostMallocDefault) /* (write-combined staging: no gain) */
    {
        if (n <= hcap) return hipSuccess;
        if (h) (void)hipHostFree(h);
        h = nullptr;
        hcap = 0;
        const hipError_t e = hipHostMalloc((void **)&h, roomy(n) * sizeof(T), flags);
        if (e == hipSuccess) hcap = roomy(n);
        return e;
    }
    hipError_t ensure_device(size_t n) { return ensure_device(n, roomy(n)); }
    hipError_t ensure_device(size_t n, size_t alloc) /* alloc >= n: what to allocate when n no longer fits */
    {
        if (n <= dcap) return hipSuccess;
        if (d) (void)hipFree(d);
        d = nullptr;
        dcap = 0;
        const hipError_t e = hipMalloc((void **)&d, alloc * sizeof(T) + 16);
        if (e == hipSuccess) dcap = alloc;
        return e;
    }
    hipError_t ensure(size_t n)
    {
        const hipError_t e = ensure_host(n);
        return e == hipSuccess ? ensure_device(n) : e;
    }
};

struct PipeWs {
    Grow<short> in, out;
    Grow<float> mask;      /* resynth: mask rows */
    Grow<long long> meta;  /* offsets | lengths | mask offsets, in launch order */
    Grow<float> f32, ceps; /* sea_denoise_ceps_utterances: the float NoiseSup stream (device side used only), the cepstra */
    Grow<int> ints;        /* the same: first_out | n_ceps | order */
    Grow<float> wb_rows;   /* sea_wb_denoise_utterances: per frame 3 high-band energies, then per frame 9 code values */
    Grow<char> inter;      /* device only: resynth / wideband QMF scratch, allocated as asked for */
    Grow<float> state;     /* device only: the recursion per utterance between two launches of a time-slice pipeline */
    Grow<float> feat, afe_state;      /* sea_wb_features_utterances, sea_features_utterances: the emitted rows of every slice; device only: the chain's
                                       * state (the cepstrum pipelines: sea_compceps_batch_slice's) */
    Grow<unsigned char> flag_rows, fin; /* the same: device only, a slice's speech flags; per slice the utterances that end with it */
    hipStream_t stream[kMaxStreams] = {};
    hipEvent_t ev_meta = nullptr, ev_done[kMaxChunks] = {}, ev_kernel[kMaxChunks] = {}, ev_h2d[kMaxChunks] = {};
    int device = -1;
    ~PipeWs() { release(); }
    template <class... G>
    static void release_all(G &...g) { (g.release(), ...); }
    template <class F>
    hipError_t each_event(F f) /* f on every event until one call fails */
    {
        hipError_t e = f(ev_meta);
        for (hipEvent_t *evs : {ev_done, ev_kernel, ev_h2d})
            for (int i = 0; i < kMaxChunks && e == hipSuccess; ++i) e = f(evs[i]);
        return e;
    }
    void release()
    {
        int cur = -1;
        const bool sw = device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != device;
        if (sw) (void)hipSetDevice(device); /* the buffers belong to `device`, whatever the thread uses now */
        release_all(in, out, mask, meta, f32, ceps, ints, wb_rows, inter, state, feat, afe_state, flag_rows, fin);
        for (auto &s : stream) {
            if (s) (void)hipStreamDestroy(s);
            s = nullptr;
        }
        (void)each_event([](hipEvent_t &e) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
            return hipSuccess;
        });
        if (sw) (void)hipSetDevice(cur);
        device = -1;
    }
    hipError_t bind()
    {
        int dev = -1;
        hipError_t e;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
        if (dev != device) { /* the thread moved to another device: nothing of the old one is usable */
            if (device >= 0) release();
            device = dev;
        }
        for (int i = 0; i < kStreams; ++i)
            if (!stream[i] && (e = hipStreamCreateWithFlags(&stream[i], hipStreamNonBlocking)) != hipSuccess) return e;
        return each_event([](hipEvent_t &ev) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); });
    }
    hipError_t ensure_inter(size_t bytes) { return inter.ensure_device(bytes, bytes); }
    hipError_t ensure_state(size_t floats) { return state.ensure_device(floats, floats + floats / 4); }
    void drain()
    {
        for (auto &s : stream)
            if (s) (void)hipStreamSynchronize(s);
    }
};
thread_local PipeWs t_ws;
thread_local int t_last_slices = 0; /* launches the calling thread's last time-slice pipeline call was cut into */

/* On every exit path: no pool task may outlive the buffers it copies from / to, no stream may still be copying. */
struct Scope {
    Latch all;
    PipeWs *ws;
    bool ok = false;
    explicit Scope(PipeWs *w) : ws(w) {}
    ~Scope()
    {
        all.wait();
        if (!ok) ws->drain();
    }
};

/* hipEventQuery as a three-way answer: 1 when the event has completed, 0 while the work before it is still running
 * (hipErrorNotReady), -1 after fail() for ANYTHING else -- a failed kernel or copy, an invalid event.  The pipelines below
 * poll events; treating every non-success as "not yet" would spin for ever on a fault instead of returning the reference's
 * fault code.  g_event_query is hipEventQuery except under sea_selftest_hostpipe_fault. */
typedef hipError_t (*EventQueryFn)(hipEvent_t);
EventQueryFn g_event_query = hipEventQuery;
int evq(hipEvent_t e, const char *what)
{
    const hipError_t r = g_event_query(e);
    if (r == hipSuccess) return 1;
    if (r == hipErrorNotReady) return 0;
    (void)hipGetLastError(); /* the sticky copy of an asynchronous fault must not fail the caller's next, unrelated call */
    fail("%s: %s", what, hipGetErrorString(r));
    return -1;
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

long long env_mb(const char *name, long long dflt)
{
    if (const char *e = getenv(name)) {
        const long long v = atoll(e);
        if (v > 0) return v;
    }
    return dflt;
}

/* cut the (sorted) list into at most max_chunks contiguous chunks of about `target` weight each */
std::vector<int> cut_chunks(const std::vector<long long> &weight_prefix, int n, long long target, int max_chunks)
{
    const long long total = weight_prefix[n];
    int nchunk = (int)std::min<long long>(max_chunks, std::max<long long>(1, (total + target - 1) / target));
    nchunk = std::min(nchunk, n);
    std::vector<int> cuts(1, 0);
    for (int k = 1; k < nchunk; ++k) {
        const long long want = total * k / nchunk;
        int j = (int)(std::lower_bound(weight_prefix.begin(), weight_prefix.begin() + n + 1, want) - weight_prefix.begin());
        j = std::max(j, cuts.back() + 1);
        if (j >= n) break;
        cuts.push_back(j);
    }
    cuts.push_back(n);
    return cuts;
}

/* SEA_HOST_TRACE=n: from the process's n-th pipeline call of more than one piece on (calls of one piece: with n <= 0) */
bool trace_this_call(int n_pieces)
{
    static std::atomic<int> n_cut{0};
    const char *tr = getenv("SEA_HOST_TRACE");
    return tr && (n_pieces == 1 ? atoi(tr) <= 0 : n_cut++ >= atoi(tr));
}

/* The event-driven loop of every pipeline here.  Piece k of packed.size() goes through
 *     packed[k] (the latch of its packing tasks)
 *     issue(k)      upload + launch on the caller's streams; records ev_h2d[k] after the upload, ev_kernel[k] after the launch
 *     download(k)   once ev_kernel[k] has completed; records ev_done[k]
 *     unpack(k)     once ev_done[k] has completed: pool tasks into the caller's buffers, counted in scope.all
 * in that order, pieces in turn.  A copy is only handed to the runtime when everything it depends on has finished: the copy
 * engines' queues are in order, so a D2H copy queued behind its still-running kernel would hold up the H2D copies of later
 * pieces (measured: piece k+2's upload waited for piece k's kernel).  uploads_in_turn: piece k is issued when piece k - 1's
 * upload has completed -- concurrent uploads share the link, and the first kernel should start as early as it can.
 * issue and download return 0 or fail().  An event that answers anything but "done" / "not ready" ends the call with 1 as well,
 * at once: the caller's Scope then waits for the pool and drains the streams.  Returns 0 with everything unpacked and
 * scope.ok set.
 * SEA_HOST_TRACE: the host-clock timeline of the call on stderr. */
template <class Issue, class Download, class Unpack>
int run_pipeline(PipeWs &w, Scope &scope, std::vector<Latch> &packed, const char *piece, bool uploads_in_turn, Issue issue,
                 Download download, Unpack unpack)
{
    const int n = (int)packed.size();
    const bool trace = trace_this_call(n);
    const double t0 = now_ms();
    enum { kWaitPack, kComputing, kDownloading, kUnpacking };
    std::vector<char> state(n, kWaitPack);
    int next = 0, finished = 0;
    while (finished < n) {
        bool progressed = false;
        int r = 0;
        if (next < n && packed[next].ready() &&
            (!uploads_in_turn || next == 0 || (r = evq(w.ev_h2d[next - 1], "hostpipe: upload event")) != 0)) {
            if (r < 0) return 1;
            const int k = next++;
            if (trace) fprintf(stderr, "[hostpipe] %7.3f ms  %s %d of %d packed, issuing\n", now_ms() - t0, piece, k, n);
            if (issue(k)) return 1;
            state[k] = kComputing;
            progressed = true;
        }
        for (int k = 0; k < next; ++k) {
            if (state[k] == kComputing && (r = evq(w.ev_kernel[k], "hostpipe: kernel event")) != 0) {
                if (r < 0) return 1;
                if (trace) fprintf(stderr, "[hostpipe] %7.3f ms  %s %d computed, downloading\n", now_ms() - t0, piece, k);
                if (download(k)) return 1;
                state[k] = kDownloading;
                progressed = true;
            }
            if (state[k] == kDownloading && (r = evq(w.ev_done[k], "hostpipe: download event")) != 0) {
                if (r < 0) return 1;
                if (trace) fprintf(stderr, "[hostpipe] %7.3f ms  %s %d on the host, unpacking\n", now_ms() - t0, piece, k);
                unpack(k);
                state[k] = kUnpacking;
                finished++;
                progressed = true;
            }
        }
        if (!progressed) {
            if (next < n && !packed[next].ready()) packed[next].wait_for(std::chrono::microseconds(30));
            else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    scope.all.wait();
    if (trace) fprintf(stderr, "[hostpipe] %7.3f ms  all unpacked (%d %ss)\n", now_ms() - t0, n, piece);
    scope.ok = true;
    return 0;
}

/* The rows of every slice of a plan into the meta staging (slice k's at p.mbase[k]); returns per slice the byte prefix of its
 * pieces, for task sizing. */
std::vector<std::vector<long long>> fill_slice_rows(const SlicePlan &p, long long hop, bool absolute, long long *meta_h)
{
    std::vector<std::vector<long long>> bpre(p.K);
    for (int k = 0; k < p.K; ++k) {
        bpre[k].resize(p.nact[k] + 1);
        slice_rows(p, k, hop, absolute, meta_h + p.mbase[k], bpre[k].data());
    }
    return bpre;
}

/* One NoiseSup launch over slice k of K on the workspace's in / out buffers: d_rows = the slice's offsets | lengths rows on
 * the device, nact utterances.  A list that is cut carries the recursion in w.state and runs on the four-wave forms, which
 * load and store it (2; 4, the tables in LDS, above four utterances per CU); a list in one piece runs as
 * sea_ns_denoise_batch would.  The list is sorted longest first, so form 2's issue priority goes by rows of n_cu without an
 * order array. */
int ns_launch_slice(PipeWs &w, DeviceCtx *dc, const long long *d_rows, int nact, int K, int k, int frame_base, hipStream_t s)
{
    sea::NsBatchArgs a = {};
    a.in = w.in.d;
    a.out = w.out.d;
    a.offsets = d_rows;
    a.lengths = d_rows + nact;
    a.tables = dc->ns;
    a.n_utt = nact;
    int form;
    if (K > 1) {
        a.state = w.state.d;
        a.resume = k > 0;
        a.frame_base = frame_base;
        form = (nact <= 4 * dc->n_cu) ? 2 : 4;
    } else
        form = ns_pick_form(nact, dc->n_cu);
    if (form == 2 && nact > dc->n_cu) a.prio_row = dc->n_cu;
    return ns_launch(a, form, s);
}

/* ---- the time-slice pipelines ------------------------------------------------------------------------ */
/* The list cut along the TIME axis: slice k holds the frames [B_k, B_k+1) of every utterance that has them, packed like a
 * batch of its own, and is one launch (or launch group) over all those utterances, the recursion travelling in a state blob
 * per utterance.  A launch then lasts as long as ITS frames take -- a chunk of whole utterances lasts as long as its longest
 * utterance, whatever its size -- so the pipeline
 *     pool threads  pack slice k+1            | unpack slice k-1
 *     copy engines  H2D slice k+1             | D2H slice k-1
 *     device        kernel over slice k
 * has short fill and drain phases: the first kernel starts after 1/K of the upload, the last download carries 1/K of the
 * output.  Slice boundaries (slice_plan.h) equalise the slices' sample counts (SEA_HOST_SLICES of them, default 8: measured on the
 * 1024-utterance bench corpus, tools/host_slices_sweep.sh, alternating on one box -- chunks of whole utterances 7.4 ms,
 * 4 slices 6.2-6.5, 6: 5.9-6.0, 8: 4.8-5.7, 10: 5.6-5.7, 12: 5.3-5.8, 16: 5.8 ms; what is left is the pool's memcpy
 * rate: 2 x 131 MB packed and unpacked in that time).
 * Three streams, one per job -- uploads (after the meta rows, same stream), kernels (in order: slice k needs slice k - 1's
 * state), downloads: with one stream per slice, reused round robin, a slice's download ended up queued behind a later slice's
 * kernel (calls of 13-20 ms among the 6 ms ones). */

/* slice k as the callables launch and extra_download of run_slices see it */
struct SliceView {
    int k, n;                /* the slice, its utterances (nact[k]) */
    long long f0, fr;        /* its first frame in the staging buffers (foff[k]), its frames */
    size_t i0;               /* the number of its first piece among the pieces of all slices in plan order (mbase[k] / 2) */
    const long long *d_rows; /* its offsets | lengths rows on the device */
    int frame_base;          /* its first frame in every utterance (B[k]) */
    bool resume;             /* k > 0: the recursion continues from the state blob */
    hipStream_t sKern, sDown;
};

/* one utterance's piece of a slice as the callable unpack_piece sees it */
struct SlicePiece {
    int u;           /* the utterance */
    size_t i;        /* the piece's number among the pieces of all slices in plan order (mbase[k] / 2 + j) */
    long long b;     /* its first frame in the utterance (B[k]) */
    long long f0, n; /* its first frame in the staging buffers, its frames */
    long long start; /* rows the utterance's earlier slices emitted: where this piece's rows go (0 without row counts) */
};

/* One call of a time-slice pipeline on plan p (p.K > 0) of the list `in`, frames of hop_in samples up.  The caller has sized
 * the workspace's buffers and written what it keeps in w.meta.h behind the slices' offsets | lengths rows (meta_n long longs
 * are uploaded in all); the rows themselves are written here, offsets absolute (the device sees ONE in and ONE out buffer) or
 * from each slice's start (a slice is a batch of its own).  Per slice:
 *     upload of its input, then on the kernel stream   launch(view)          returns 0 or fail()
 *     download of its int16 audio (frames of hop_out samples, where want_out), then on the download stream
 *                                                      extra_download(view)  returns 0 or fail()
 *     per utterance, in a pool task                    unpack_piece(piece)   copied into the tasks: it holds pointers only
 * h_cnt, where given: the pinned array extra_download brings the pieces' emitted row counts to (piece i's at h_cnt[i]); the
 * slices are then unpacked in slice order (RowOrder, slice_plan.h), piece.start says where the rows go, and after the run
 * n_rows[u] is the total of every utterance with a whole frame.  Returns run_pipeline's result. */
template <class Launch, class ExtraDownload, class UnpackPiece>
int run_slices(PipeWs &w, Pool &pool, const SlicePlan &p, const char *piece, const short *const *in, long long hop_in,
               long long hop_out, bool want_out, bool absolute, bool small, size_t meta_n, const int *h_cnt, int *n_rows,
               Launch launch, ExtraDownload extra_download, UnpackPiece unpack_piece)
{
    const int K = p.K;
    /* The lifetime rule of every pipeline here: what a pool task dereferences -- bpre, order.start, packed -- is declared
     * BEFORE scope, whose destructor waits for the pool on every exit path.  (p is the caller's and outlives this call.) */
    const std::vector<std::vector<long long>> bpre = fill_slice_rows(p, hop_in, absolute, w.meta.h);
    RowOrder order(h_cnt ? K : 0, h_cnt ? (int)p.idx.size() : 0);
    std::vector<Latch> packed(K);
    Scope scope(&w);
    short *h_in = w.in.h;
    const int *ix = p.idx.data();
    for (int k = 0; k < K; ++k) {
        const long long *offs = w.meta.h + p.mbase[k], *lens = offs + p.nact[k];
        const long long b0 = hop_in * p.B[k], s0 = absolute ? 0 : hop_in * p.foff[k];
        run_copies(pool, 0, p.nact[k], bpre[k].data(), &packed[k], &scope.all, small,
                   [=](int j) { copy_stream(h_in + s0 + offs[j], in[ix[j]] + b0, (size_t)lens[j] * sizeof(short)); });
    }
    hipStream_t sUp = w.stream[0], sKern = w.stream[1], sDown = w.stream[2];
    HIP_TRY(hipMemcpyAsync(w.meta.d, w.meta.h, meta_n * sizeof(long long), hipMemcpyHostToDevice, sUp));
    auto view = [&](int k) {
        return SliceView{k, p.nact[k], p.foff[k], p.foff[k + 1] - p.foff[k], p.mbase[k] / 2, w.meta.d + p.mbase[k], (int)p.B[k], k > 0,
                         sKern, sDown};
    };
    auto cut = [&](int k, const long long *st) { /* the copy tasks of slice k */
        const long long *offs = w.meta.h + p.mbase[k], *lens = offs + p.nact[k];
        const long long bk = p.B[k], s0 = absolute ? 0 : p.foff[k];
        const size_t i0 = p.mbase[k] / 2;
        run_copies(pool, 0, p.nact[k], bpre[k].data(), nullptr, &scope.all, small, [=](int j) {
            unpack_piece(SlicePiece{ix[j], i0 + (size_t)j, bk, s0 + offs[j] / hop_in, lens[j] / hop_in, st ? st[j] : 0});
        });
    };

    const int rc = run_pipeline(
        w, scope, packed, piece, true,
        [&](int k) {
            const SliceView v = view(k);
            HIP_TRY(hipMemcpyAsync(w.in.d + hop_in * v.f0, h_in + hop_in * v.f0, (size_t)(v.fr * hop_in) * sizeof(short),
                                   hipMemcpyHostToDevice, sUp));
            HIP_TRY(hipEventRecord(w.ev_h2d[k], sUp));
            HIP_TRY(hipStreamWaitEvent(sKern, w.ev_h2d[k], 0));
            if (launch(v)) return 1;
            HIP_TRY(hipEventRecord(w.ev_kernel[k], sKern));
            return 0;
        },
        [&](int k) {
            const SliceView v = view(k);
            if (want_out)
                HIP_TRY(hipMemcpyAsync(w.out.h + hop_out * v.f0, w.out.d + hop_out * v.f0, (size_t)(v.fr * hop_out) * sizeof(short),
                                       hipMemcpyDeviceToHost, sDown));
            if (extra_download(v)) return 1;
            HIP_TRY(hipEventRecord(w.ev_done[k], sDown));
            return 0;
        },
        [&](int k) {
            if (h_cnt) order.arrive(p, k, h_cnt, cut);
            else cut(k, nullptr);
        });
    if (rc) return rc;
    if (n_rows) /* every slice has arrived, so every slice is cut: pos is the utterance's total */
        for (size_t j = 0; j < p.idx.size(); ++j)
            if (p.nfr[j] > 0) n_rows[ix[j]] = (int)order.pos[j];
    return 0;
}

/* the plan of a call: one slice for a list too small to cut, SEA_HOST_SLICES (default 8) otherwise */
void plan_call(SlicePlan &p, const long *lengths, int n_utt, long long hop, bool small)
{
    slice_plan(p, lengths, n_utt, hop, small ? 1 : (int)env_mb("SEA_HOST_SLICES", 8));
}

/* The FEATURES from host buffers, both rates: per slice sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice (WB:
 * sea_wb_denoise_batch_slice_fd + sea_wb_afe_features_batch_slice) on the kernel stream.  Slice k is a batch of its own on the
 * device (offsets from the slice's start), so what the chain reads of a slice -- the float stream, the flag bytes (8 kHz: one
 * per 8 samples), the cepstra before PostProc, and the wideband mode's QMF scratch, high-band and code rows -- lives in device
 * buffers of one slice's size, reused by the next slice (the kernels run in order on one stream) and never downloaded.  What
 * travels back is a slice's block of emitted rows (its frames + 6 per utterance), the counts, and the int16 audio where the
 * caller asks for it.  d_final is set where an utterance's last planned slice is this one.  An utterance without a whole frame
 * is in no slice: its result is DoVADFlush on the initial state, six zero rows, written here.
 * The state is used even for a list that is not cut: there is one path here, the slice kernels'. */
template <bool WB>
int features_slices(const char *who, const short *const *in, short *const *out, float *const *feats, int *n_feat,
                    const long *lengths, int n_utt)
{
    if (n_utt <= 0) return 0;
    if (!in || !feats || !n_feat || !lengths) return fail("%s: in, feats, n_feat and lengths are required", who);
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0) return fail("%s: negative length for utterance %d", who, u);
        if (!feats[u]) return fail("%s: feats[%d] is NULL", who, u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    constexpr long long kIn = WB ? SEA_WB_HOP : SEA_HOP, kOut = SEA_HOP; /* samples per frame up / down */
    const long long total_fr = slice_total_frames(lengths, n_utt, kIn);
    t_last_slices = 0;
    for (int u = 0; u < n_utt; ++u) {
        n_feat[u] = 0;
        if (lengths[u] / kIn == 0) { /* in no slice: DoVADFlush on the initial state */
            memset(feats[u], 0, 6 * 15 * sizeof(float));
            n_feat[u] = 6;
        }
    }
    if (total_fr == 0) return 0;
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    /* "small list -> one slice" in FRAMES at both rates: a frame costs the 8 kHz chain what it costs the wideband one (the frame
     * loop and the tile are the same), so the list too small to cut is one of 2 MB / 320 B = 6553 frames */
    const bool small = total_fr * SEA_WB_HOP * 2 < (2 << 20) || pool.size() <= 1;
    SlicePlan p;
    plan_call(p, lengths, n_utt, kIn, small);
    if (p.max_fr > 0x7fffffffLL - 8) return fail("%s: utterance %d is too long", who, p.idx[0]);
    const int K = t_last_slices = p.K;

    /* meta: the slices' offsets | lengths rows, then per slice the two prefix sums (nact + 1 each); ints: per piece the count,
     * then first_out and onset per utterance; feat: the block of the slice whose first piece is number i0 starts at row
     * foff[k] + 6 * i0 */
    const long long max_slice_fr = slice_max_frames(p);
    const size_t n_act = p.mbase[K] / 2;
    auto cum_base = [&](int k) { return p.mbase[K] + p.mbase[k] + 2 * (size_t)k; };
    HIP_TRY(w.in.ensure((size_t)(total_fr * kIn)));
    HIP_TRY(w.out.ensure((size_t)(total_fr * kOut)));
    HIP_TRY(w.meta.ensure(cum_base(K)));
    HIP_TRY(w.ints.ensure(n_act + 2 * (size_t)n_utt));
    HIP_TRY(w.fin.ensure(n_act));
    HIP_TRY(w.feat.ensure(((size_t)total_fr + 6 * n_act) * 15));
    HIP_TRY(w.f32.ensure_device((size_t)(max_slice_fr * kOut)));
    HIP_TRY(w.flag_rows.ensure_device(WB ? (size_t)max_slice_fr + 1 : (size_t)max_slice_fr * 10 + 1));
    HIP_TRY(w.ceps.ensure_device((size_t)max_slice_fr * SEA_CC_NCEP));
    HIP_TRY(w.ensure_state((size_t)n_utt * (WB ? sea::kWbSliceStateFloats : sea::kNsPipeStateFloats)));
    HIP_TRY(w.afe_state.ensure_device((size_t)n_utt * (WB ? sea::kWbAfeStateFloats : sea::kAfeStateFloats)));
    if (WB) {
        HIP_TRY(w.wb_rows.ensure_device(12 * ((size_t)max_slice_fr + 1)));
        HIP_TRY(w.ensure_inter((size_t)sea_wb_scratch_bytes(max_slice_fr * kIn, n_utt)));
    }
    for (int k = 0; k < K; ++k) {
        const int n = p.nact[k];
        long long *cc = w.meta.h + cum_base(k), *fc = cc + n + 1, c = 0;
        unsigned char *fin = w.fin.h + p.mbase[k] / 2;
        for (int j = 0; j < n; ++j) {
            cc[j] = c;
            fc[j] = c + 6 * (long long)j;
            fin[j] = p.nfr[j] <= p.B[k + 1];
            c += slice_piece_frames(p, k, j);
        }
        cc[n] = c;
        fc[n] = c + 6 * (long long)n;
    }
    short *h_out = w.out.h;
    float *h_feat = w.feat.h;
    const int *h_cnt = w.ints.h;
    int *d_first = w.ints.d + n_act, *d_onset = d_first + n_utt;
    float *d_hp = WB ? w.wb_rows.d : nullptr, *d_code = WB ? w.wb_rows.d + 3 * ((size_t)max_slice_fr + 1) : nullptr;
    HIP_TRY(hipMemcpyAsync(w.fin.d, w.fin.h, n_act, hipMemcpyHostToDevice, w.stream[0])); /* the upload stream, before every slice */

    return run_slices(
        w, pool, p, WB ? "wideband feature slice" : "feature slice", in, kIn, kOut, out != nullptr, false, small, cum_base(K), h_cnt,
        n_feat,
        [&](const SliceView &v) {
            const long long *d_rows = v.d_rows, *d_cc = w.meta.d + cum_base(v.k);
            const int n = v.n;
            const short *d_in = w.in.d + kIn * v.f0;
            short *d_out = w.out.d + kOut * v.f0;
            float *d_blk = w.feat.d + 15 * (v.f0 + 6 * (long long)v.i0);
            if constexpr (WB) {
                if (sea_wb_denoise_batch_slice_fd(d_in, d_out, w.f32.d, d_rows, d_rows + n, nullptr, d_first, d_onset, w.flag_rows.d,
                                                  d_hp, d_code, (float *)w.inter.d, v.fr * kIn, w.state.d, n, v.frame_base, v.resume,
                                                  v.sKern))
                    return 1;
                return sea_wb_afe_features_batch_slice(w.f32.d, w.flag_rows.d, d_hp, d_code, d_rows, d_rows + n, d_first, d_onset,
                                                       w.fin.d + v.i0, d_cc, v.fr, w.ceps.d, nullptr, d_cc + n + 1, d_blk,
                                                       w.ints.d + v.i0, nullptr, w.afe_state.d, n, v.frame_base, v.resume, v.sKern);
            } else {
                if (sea_ns_denoise_batch_slice_fd(d_in, d_out, w.f32.d, d_rows, d_rows + n, nullptr, d_first, w.flag_rows.d, d_onset,
                                                  w.state.d, n, v.frame_base, v.resume, v.sKern))
                    return 1;
                return sea_afe_features_batch_slice(w.f32.d, w.flag_rows.d, d_rows, d_rows + n, d_first, d_onset, w.fin.d + v.i0, d_cc,
                                                    v.fr, w.ceps.d, nullptr, d_cc + n + 1, d_blk, w.ints.d + v.i0, nullptr,
                                                    w.afe_state.d, n, v.frame_base, v.resume, v.sKern);
            }
        },
        [&](const SliceView &v) {
            const long long r0 = v.f0 + 6 * (long long)v.i0, nr = v.fr + 6 * (long long)v.n;
            HIP_TRY(hipMemcpyAsync(h_feat + 15 * r0, w.feat.d + 15 * r0, (size_t)nr * 15 * sizeof(float), hipMemcpyDeviceToHost, v.sDown));
            HIP_TRY(hipMemcpyAsync(w.ints.h + v.i0, w.ints.d + v.i0, (size_t)v.n * sizeof(int), hipMemcpyDeviceToHost, v.sDown));
            return 0;
        },
        [=](const SlicePiece &c) {
            if (out && out[c.u]) /* whole frames only: the trailing partial frame stays untouched, as with etsi_denoise */
                copy_stream(out[c.u] + kOut * c.b, h_out + kOut * c.f0, (size_t)(c.n * kOut) * sizeof(short));
            if (h_cnt[c.i] > 0)
                copy_stream(feats[c.u] + 15 * c.start, h_feat + 15 * (c.f0 + 6 * (long long)c.i), (size_t)h_cnt[c.i] * 15 * sizeof(float));
        });
}

} // namespace

extern "C" {

/* Test hook: from the nth event query of this process on (1-based; 0 switches the hook off) every query reports a device
 * fault instead of asking the runtime.  tests/test_gpu_parity.py::test_host_pipeline_returns_fault_on_event_error checks
 * that the time-slice driver (through three of its entry points) and both chunk pipelines then return 1 with their streams
 * drained and work again afterwards. */
static std::atomic<long long> g_fault_after{0}, g_queries{0};
static hipError_t faulty_query(hipEvent_t e)
{
    const long long n = g_fault_after.load();
    if (n > 0 && ++g_queries >= n) return hipErrorLaunchFailure;
    return hipEventQuery(e);
}
int sea_selftest_hostpipe_fault(long long nth_query)
{
    g_queries = 0;
    g_fault_after = nth_query;
    g_event_query = nth_query > 0 ? faulty_query : hipEventQuery;
    return 0;
}

int sea_host_threads(void)
{ /* of the calling thread's current device */
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return Pool::get(dev).size();
}

/* ---------------------------------------------------------------------------------------------------- */
static int denoise_utterances_slices(const short *const *in, short *const *out, const long *lengths, int n_utt);

/* SEA_HOST_MODE=chunks: the list cut into chunks of whole utterances, one launch per chunk on its own stream (round 3's
 * first pipeline, kept for A/B).  Default: time slices (denoise_utterances_slices below). */
static int denoise_utterances_chunks(const short *const *in, short *const *out, const long *lengths, int n_utt)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    for (int u = 0; u < n_utt; ++u)
        if (lengths[u] < 0) return fail("negative length for utterance %d", u);
    /* launch order: longest first */
    std::vector<int> idx(n_utt);
    for (int i = 0; i < n_utt; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lengths[a] > lengths[b]; });
    std::vector<long long> pre(n_utt + 1, 0); /* packed offset of sorted position j, in samples */
    for (int j = 0; j < n_utt; ++j) pre[j + 1] = pre[j] + align8(lengths[idx[j]]);
    const long long total = pre[n_utt];
    if (total == 0) return 0;

    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    HIP_TRY(w.in.ensure((size_t)total));
    HIP_TRY(w.out.ensure((size_t)total));
    HIP_TRY(w.meta.ensure(2 * (size_t)n_utt));
    long long *offs = w.meta.h, *lens = w.meta.h + n_utt;
    for (int j = 0; j < n_utt; ++j) {
        offs[j] = pre[j];
        lens[j] = lengths[idx[j]];
    }
    /* Chunks (small lists: one chunk, packed by the calling thread), issued longest first.  Default: a third of the list
     * each -- measured on the 1024-utterance bench corpus: kernels launched on different streams do overlap, but a launch
     * runs as long as its longest utterance's chain of frames whatever its size and several small launches side by side
     * fill the chip worse than one large one, so few large chunks win (3 chunks 6.3 ms, 6 chunks 7.4 ms, 16 chunks 16.5 ms;
     * one chunk = no overlap 10.4 ms).  SEA_HOST_CHUNK_MB sets the chunk size in MB of int16.
     * Measured with switches that were removed afterwards: issuing the shortest chunk first, or long and short
     * in turn, is within 5 % of longest first and no better; kernel stores straight to the pinned output staging instead of
     * a D2H copy reach ~24 GB/s against the copy's 52 GB/s and slow the kernel down by as much as the copy they save. */
    const long long chunk_samples = getenv("SEA_HOST_CHUNK_MB") ? env_mb("SEA_HOST_CHUNK_MB", 24) * (1 << 20) / 2
                                                                : std::max<long long>((total + 2) / 3, 1 << 20);
    const bool small = total * 2 < (2 << 20) || n_utt == 1 || pool.size() <= 1;
    const std::vector<int> cuts = small ? std::vector<int>{0, n_utt} : cut_chunks(pre, n_utt, chunk_samples, kMaxChunks);
    const int nchunk = (int)cuts.size() - 1;
    const int form = ns_pick_form(n_utt, dc->n_cu);

    std::vector<Latch> packed(nchunk);
    Scope scope(&w);
    short *h_in = w.in.h, *h_out = w.out.h;
    std::vector<long long> bytes_pre(pre); /* task sizing */
    for (auto &b : bytes_pre) b *= 2;
    const long long *bp = bytes_pre.data();
    const int *ix = idx.data();
    for (int k = 0; k < nchunk; ++k)
        run_copies(pool, cuts[k], cuts[k + 1], bp, &packed[k], &scope.all, small, [=](int j) {
            const long long L = lens[j];
            copy_stream(h_in + offs[j], in[ix[j]], (size_t)L * sizeof(short));
            const long long pad = align8(L) - L;
            if (pad) memset(h_in + offs[j] + L, 0, (size_t)pad * sizeof(short));
        });
    HIP_TRY(hipMemcpyAsync(w.meta.d, w.meta.h, 2 * (size_t)n_utt * sizeof(long long), hipMemcpyHostToDevice, w.stream[0]));
    HIP_TRY(hipEventRecord(w.ev_meta, w.stream[0]));

    return run_pipeline(
        w, scope, packed, "chunk", true,
        [&](int k) {
            hipStream_t s = w.stream[k % kStreams];
            const int u0 = cuts[k], n = cuts[k + 1] - cuts[k];
            const long long o0 = pre[u0], cnt = pre[cuts[k + 1]] - o0;
            if (k > 0 && k < kStreams) HIP_TRY(hipStreamWaitEvent(s, w.ev_meta, 0));
            HIP_TRY(hipMemcpyAsync(w.in.d + o0, h_in + o0, (size_t)cnt * sizeof(short), hipMemcpyHostToDevice, s));
            HIP_TRY(hipEventRecord(w.ev_h2d[k], s));
            sea::NsBatchArgs a = {};
            a.in = w.in.d;
            a.out = w.out.d;
            a.offsets = w.meta.d + u0;
            a.lengths = w.meta.d + n_utt + u0;
            a.tables = dc->ns;
            a.n_utt = n;
            if (form == 2 && n_utt > dc->n_cu) { /* issue priority by rows of the whole list, as the one-launch form has it */
                a.prio_row = dc->n_cu;
                a.prio_base = u0 / dc->n_cu;
            }
            if (ns_launch(a, form, s)) return 1;
            HIP_TRY(hipEventRecord(w.ev_kernel[k], s));
            return 0;
        },
        [&](int k) {
            hipStream_t s = w.stream[k % kStreams];
            const long long o0 = pre[cuts[k]], cnt = pre[cuts[k + 1]] - o0;
            HIP_TRY(hipMemcpyAsync(h_out + o0, w.out.d + o0, (size_t)cnt * sizeof(short), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(w.ev_done[k], s));
            return 0;
        },
        [&](int k) {
            run_copies(pool, cuts[k], cuts[k + 1], bp, nullptr, &scope.all, small, [=](int j) {
                /* the trailing partial frame stays untouched */
                copy_stream(out[ix[j]], h_out + offs[j], (size_t)(lens[j] / 80 * 80) * sizeof(short));
            });
        });
}

int sea_denoise_utterances(const short *const *in, short *const *out, const long *lengths, int n_utt)
{
    const char *m = getenv("SEA_HOST_MODE");
    if ((m && !strcmp(m, "chunks")) || kStreams < 3) return denoise_utterances_chunks(in, out, lengths, n_utt);
    return denoise_utterances_slices(in, out, lengths, n_utt);
}

/* NoiseSup in time slices (run_slices above), sea_ns_denoise_batch_slice per slice.  The slices lie one after the other in the
 * staging, offsets absolute: the device sees ONE in and ONE out buffer.  A list that is not cut needs no state blob and runs
 * as sea_ns_denoise_batch would (ns_launch_slice). */
static int denoise_utterances_slices(const short *const *in, short *const *out, const long *lengths, int n_utt)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    for (int u = 0; u < n_utt; ++u)
        if (lengths[u] < 0) return fail("negative length for utterance %d", u);
    constexpr long long kHop = SEA_HOP;
    const long long total = slice_total_frames(lengths, n_utt, kHop) * kHop;
    if (total == 0) return 0;
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    const bool small = total * 2 < (2 << 20) || pool.size() <= 1;
    SlicePlan p;
    plan_call(p, lengths, n_utt, kHop, small);
    const int K = t_last_slices = p.K;
    HIP_TRY(w.in.ensure((size_t)total));
    HIP_TRY(w.out.ensure((size_t)total));
    HIP_TRY(w.meta.ensure(p.mbase[K]));
    if (K > 1) HIP_TRY(w.ensure_state((size_t)n_utt * sea::kNsPipeStateFloats));
    short *h_out = w.out.h;
    return run_slices(
        w, pool, p, "slice", in, kHop, kHop, true, true, small, p.mbase[K], nullptr, nullptr,
        [&](const SliceView &v) { return ns_launch_slice(w, dc, v.d_rows, v.n, K, v.k, v.frame_base, v.sKern); },
        [](const SliceView &) { return 0; },
        [=](const SlicePiece &c) { copy_stream(out[c.u] + kHop * c.b, h_out + kHop * c.f0, (size_t)(c.n * kHop) * sizeof(short)); });
}

/* ---------------------------------------------------------------------------------------------------- */
/* The wideband (16 kHz) mode from host buffers: the same cut (frames of 160 input samples here), streams and loop as
 * sea_denoise_utterances, for sea_wb_denoise_batch_slice.  What differs is what travels: 160 int16 up and 80 int16 down per
 * frame, and, where the caller asks for them, 3 + 9 floats of high-band rows down.  Slice k is a batch of its own on the
 * device: its offsets count from the slice's start, so the QMF scratch (two floats per input sample) is one slice's, reused by
 * the next -- the slices' kernels run in order on one stream.  Rows of frames without an output are not written by the
 * kernels and reach the caller as zeros: the slice's rows are cleared on the kernels' stream first.
 * The state is used even for a list that is not cut: there is one wideband path here, the slice kernels'. */
int sea_wb_denoise_utterances(const short *const *in, short *const *out_lp, float *const *hp_rows, float *const *code_rows,
                              const long *lengths, int n_utt)
{
    if (n_utt <= 0) return 0;
    if (!in || !out_lp || !lengths) return fail("sea_wb_denoise_utterances: in, out_lp and lengths are required");
    if ((hp_rows == nullptr) != (code_rows == nullptr)) return fail("sea_wb_denoise_utterances: hp_rows and code_rows come together");
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0) return fail("negative length for utterance %d", u);
        if (hp_rows && (hp_rows[u] == nullptr) != (code_rows[u] == nullptr))
            return fail("sea_wb_denoise_utterances: hp_rows[%d] and code_rows[%d] come together", u, u);
    }
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    const bool rows = hp_rows != nullptr;
    constexpr long long kIn = SEA_WB_HOP, kOut = SEA_HOP; /* samples per frame up / down */
    const long long total_fr = slice_total_frames(lengths, n_utt, kIn);
    t_last_slices = 0;
    if (total_fr == 0) return 0;
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    const bool small = total_fr * kIn * 2 < (2 << 20) || pool.size() <= 1;
    SlicePlan p;
    plan_call(p, lengths, n_utt, kIn, small);
    if (p.max_fr > 0x7fffffffLL - 8) return fail("sea_wb_denoise_utterances: utterance %d is too long", p.idx[0]);
    const int K = t_last_slices = p.K;

    /* slice k starts at frame foff[k] of every staging buffer: x 160 in the input, x 80 in the output, x 3 and x 9 in the rows */
    const size_t n_rows = (size_t)total_fr + 1; /* a slice writes rows [0, its frames): sea_wb_rows' spare row is never touched */
    HIP_TRY(w.in.ensure((size_t)(total_fr * kIn)));
    HIP_TRY(w.out.ensure((size_t)(total_fr * kOut)));
    HIP_TRY(w.meta.ensure(p.mbase[K]));
    if (rows) HIP_TRY(w.wb_rows.ensure(12 * n_rows));
    HIP_TRY(w.ensure_state((size_t)n_utt * sea::kWbSliceStateFloats));
    HIP_TRY(w.ensure_inter((size_t)sea_wb_scratch_bytes(slice_max_frames(p) * kIn, n_utt)));
    short *h_out = w.out.h;
    float *h_hp = rows ? w.wb_rows.h : nullptr, *h_code = rows ? w.wb_rows.h + 3 * n_rows : nullptr;
    float *d_hp = rows ? w.wb_rows.d : nullptr, *d_code = rows ? w.wb_rows.d + 3 * n_rows : nullptr;

    return run_slices(
        w, pool, p, "wideband slice", in, kIn, kOut, true, false, small, p.mbase[K], nullptr, nullptr,
        [&](const SliceView &v) {
            if (rows) {
                HIP_TRY(hipMemsetAsync(d_hp + 3 * v.f0, 0, (size_t)v.fr * 3 * sizeof(float), v.sKern));
                HIP_TRY(hipMemsetAsync(d_code + 9 * v.f0, 0, (size_t)v.fr * 9 * sizeof(float), v.sKern));
            }
            return sea_wb_denoise_batch_slice(w.in.d + kIn * v.f0, w.out.d + kOut * v.f0, nullptr, v.d_rows, v.d_rows + v.n, nullptr,
                                              nullptr, nullptr, rows ? d_hp + 3 * v.f0 : nullptr, rows ? d_code + 9 * v.f0 : nullptr,
                                              (float *)w.inter.d, v.fr * kIn, w.state.d, v.n, v.frame_base, v.resume, v.sKern);
        },
        [&](const SliceView &v) {
            if (rows) {
                HIP_TRY(hipMemcpyAsync(h_hp + 3 * v.f0, d_hp + 3 * v.f0, (size_t)v.fr * 3 * sizeof(float), hipMemcpyDeviceToHost, v.sDown));
                HIP_TRY(hipMemcpyAsync(h_code + 9 * v.f0, d_code + 9 * v.f0, (size_t)v.fr * 9 * sizeof(float), hipMemcpyDeviceToHost, v.sDown));
            }
            return 0;
        },
        [=](const SlicePiece &c) {
            copy_stream(out_lp[c.u] + kOut * c.b, h_out + kOut * c.f0, (size_t)(c.n * kOut) * sizeof(short));
            if (rows && hp_rows[c.u]) {
                copy_stream(hp_rows[c.u] + 3 * c.b, h_hp + 3 * c.f0, (size_t)c.n * 3 * sizeof(float));
                copy_stream(code_rows[c.u] + 9 * c.b, h_code + 9 * c.f0, (size_t)c.n * 9 * sizeof(float));
            }
        });
}

/* ---------------------------------------------------------------------------------------------------- */
/* The feature chains from host buffers (features_slices above): rows of 15 floats, n_feat[u] of them. */
int sea_wb_features_utterances(const short *const *in, short *const *out_lp, float *const *feats, int *n_feat,
                               const long *lengths, int n_utt)
{
    return features_slices<true>("sea_wb_features_utterances", in, out_lp, feats, n_feat, lengths, n_utt);
}

int sea_features_utterances(const short *const *in, short *const *out, float *const *feats, int *n_feat, const long *lengths,
                            int n_utt)
{
    return features_slices<false>("sea_features_utterances", in, out, feats, n_feat, lengths, n_utt);
}

/* launches the calling thread's last time-slice pipeline call (sea_denoise_utterances in the time-slice mode,
 * sea_wb_denoise_utterances, sea_wb_features_utterances, sea_features_utterances, sea_denoise_ceps_utterances,
 * sea_wb_denoise_ceps_utterances) was cut into */
int sea_host_last_slices(void) { return t_last_slices; }

/* ---------------------------------------------------------------------------------------------------- */
/* sea_packed_*: NoiseSup from PINNED staging the CALLER fills and reads (VERDICT r03 #5 ii).
 *
 * sea_denoise_utterances takes the caller's pageable buffers, so every sample is copied twice more than the PCIe transfer
 * needs (pack into pinned staging, unpack out of it): 2 x 131 MB per 1024 utterances, and with the copies the DMA engines do
 * that is ~790 MB of DRAM traffic per call -- the packing threads' aggregate rate (~58 GB/s on the 1-GPU box, no better with
 * more threads) is what paces that entry point at ~4.5 ms per call (profiles/r04_host_pipeline.txt).  A caller that PRODUCES
 * its samples (a file reader) can write them where the copy engine reads them, and read the results where it writes them:
 *
 *   p = sea_packed_create();                       once per reusable staging set (any thread)
 *   sea_packed_plan(p, lengths, n);                lays the list out: the time slices of slice_plan.h, one after the other
 *   k = sea_packed_segments(p, u, in, out, cnt, max);   utterance u = k pieces in time order: fill in[i][0 .. cnt[i])
 *   sea_packed_denoise(p);                         on a device thread: uploads, launches, downloads, pipelined over the slices
 *   ... read out[i][0 .. cnt[i]) ...               etsi_denoise's result for every whole frame (the trailing lengths[u] % 80
 *                                                  samples are not part of any piece: the caller's, as with etsi_denoise)
 * The pinned staging is portable (any device may run sea_packed_denoise on it); the device side (buffers, streams, the
 * per-utterance state blob) is the calling thread's workspace, as for sea_denoise_utterances. */
} /* extern "C": the staging set's type and its allocator are C++ */
struct sea_packed {
    Grow<short> in, out;  /* the pinned halves only: portable, the slices one after the other */
    Grow<long long> meta; /* the same: per slice the offsets | lengths rows, offsets absolute, as the kernel reads them */
    SlicePlan plan;       /* frames of 80 samples */
    int n_utt = 0;
};

extern "C" {

sea_packed *sea_packed_create(void) { return new (std::nothrow) sea_packed(); }

void sea_packed_destroy(sea_packed *p) { delete p; }

int sea_packed_plan(sea_packed *p, const long *lengths, int n_utt)
{
    if (!p || n_utt < 0) return fail("sea_packed_plan: bad argument");
    p->n_utt = n_utt;
    p->plan.K = 0;
    for (int u = 0; u < n_utt; ++u)
        if (lengths[u] < 0) return fail("negative length for utterance %d", u);
    const long long total = slice_total_frames(lengths, n_utt, SEA_HOP) * SEA_HOP;
    /* slices: SEA_HOST_SLICES, default 10 (tools/host_packed.py on the configs[1] corpus, one box: 4: 4.22 ms, 6: 3.98, 8: 3.84,
     * 10: 3.74, 12: 3.73, 16: 3.82, 24: 3.94 -- without packing to overlap, the optimum is a little finer than the pointer-array
     * entry point's eight) */
    SlicePlan &plan = p->plan;
    slice_plan(plan, lengths, n_utt, SEA_HOP, (total * 2 < (2 << 20)) ? 1 : (int)env_mb("SEA_HOST_SLICES", 10));
    if (plan.K == 0) return 0;
    HIP_TRY(p->in.ensure_host((size_t)total, hipHostMallocPortable));
    HIP_TRY(p->out.ensure_host((size_t)total, hipHostMallocPortable));
    HIP_TRY(p->meta.ensure_host(plan.mbase[plan.K], hipHostMallocPortable));
    for (int k = 0; k < plan.K; ++k) slice_rows(plan, k, SEA_HOP, true, p->meta.h + plan.mbase[k], nullptr);
    return 0;
}

int sea_packed_slices(const sea_packed *p) { return p ? p->plan.K : 0; }

int sea_packed_segments(const sea_packed *p, int u, short **in_seg, short **out_seg, long *count, int max_seg)
{
    if (!p || u < 0 || u >= p->n_utt) return 0;
    const SlicePlan &plan = p->plan;
    const int j = plan.inv[u];
    int n = 0;
    for (int k = 0; k < plan.K && n < max_seg; ++k) {
        if (j >= plan.nact[k]) break; /* the list is sorted by length: no later slice holds this utterance either */
        const long long *offs = p->meta.h + plan.mbase[k], *lens = offs + plan.nact[k];
        if (in_seg) in_seg[n] = p->in.h + offs[j];
        if (out_seg) out_seg[n] = p->out.h + offs[j];
        if (count) count[n] = (long)lens[j];
        ++n;
    }
    return n;
}

int sea_packed_denoise(sea_packed *p)
{
    if (!p) return fail("sea_packed_denoise: NULL");
    const SlicePlan &plan = p->plan;
    const int K = plan.K;
    if (p->n_utt == 0 || K == 0) return 0;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    HIP_TRY(w.in.ensure_device((size_t)(plan.total_fr * SEA_HOP))); /* the pinned halves are the handle's */
    HIP_TRY(w.out.ensure_device((size_t)(plan.total_fr * SEA_HOP)));
    HIP_TRY(w.meta.ensure_device(plan.mbase[K]));
    if (K > 1) HIP_TRY(w.ensure_state((size_t)p->n_utt * sea::kNsPipeStateFloats));
    Scope scope(&w);
    hipStream_t sUp = w.stream[0], sKern = w.stream[1], sDown = w.stream[2];
    HIP_TRY(hipMemcpyAsync(w.meta.d, p->meta.h, plan.mbase[K] * sizeof(long long), hipMemcpyHostToDevice, sUp));
    /* Nothing to pack or unpack, so everything is issued up front: uploads in order on one stream, kernels in order on
     * another (slice k needs slice k - 1's state).  What is left of the pipelines' loop is its rule for downloads: each is
     * handed to the runtime when its kernel HAS finished (the copy engines' queues are in order: a download queued behind
     * its still-running kernel would hold up the next upload). */
    auto soff = [&](int k) { return (long long)SEA_HOP * plan.foff[k]; };
    for (int k = 0; k < K; ++k) {
        HIP_TRY(hipMemcpyAsync(w.in.d + soff(k), p->in.h + soff(k), (size_t)(soff(k + 1) - soff(k)) * sizeof(short), hipMemcpyHostToDevice, sUp));
        HIP_TRY(hipEventRecord(w.ev_h2d[k], sUp));
        HIP_TRY(hipStreamWaitEvent(sKern, w.ev_h2d[k], 0));
        if (ns_launch_slice(w, dc, w.meta.d + plan.mbase[k], plan.nact[k], K, k, (int)plan.B[k], sKern)) return 1;
        HIP_TRY(hipEventRecord(w.ev_kernel[k], sKern));
    }
    int next = 0;
    while (next < K) {
        const int r = evq(w.ev_kernel[next], "sea_packed_denoise: kernel event");
        if (r < 0) return 1;
        if (r == 0) {
            std::this_thread::sleep_for(std::chrono::microseconds(20));
            continue;
        }
        HIP_TRY(hipMemcpyAsync(p->out.h + soff(next), w.out.d + soff(next), (size_t)(soff(next + 1) - soff(next)) * sizeof(short),
                               hipMemcpyDeviceToHost, sDown));
        ++next;
    }
    HIP_TRY(hipStreamSynchronize(sDown));
    scope.ok = true;
    return 0;
}

/* ---------------------------------------------------------------------------------------------------- */
/* NoiseSup + the plain CompCeps from host buffers as a pipeline over TIME SLICES, both rates: features_slices' cut, streams
 * and loop (run_slices), per slice sea_ns_denoise_batch_slice + sea_compceps_batch_slice (WB: sea_wb_denoise_batch_slice +
 * sea_wb_compceps_batch_slice) on the kernel stream.  Slice k is a batch of its own on the device (offsets from the slice's
 * start), so the float stream -- and the wideband mode's QMF scratch, high-band rows and code rows -- live in device buffers of
 * one slice's size, reused by the next slice and never downloaded.  What travels back is the int16 audio, a slice's block of
 * cepstral rows (its frames) and the counts.
 * one_piece_elsewhere: return -1 before any work where the plan gives one slice (the 8 kHz call keeps its one launch there). */
} /* extern "C": a template */
template <bool WB>
static int denoise_ceps_slices(const char *who, const short *const *in, short *const *out, float *const *ceps, int *n_ceps,
                               const long *lengths, int n_utt, bool one_piece_elsewhere)
{
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    constexpr long long kIn = WB ? SEA_WB_HOP : SEA_HOP, kOut = SEA_HOP; /* samples per frame up / down */
    const long long total_fr = slice_total_frames(lengths, n_utt, kIn);
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    /* "small list -> one slice" is features_slices' rule, in FRAMES: the frame loop and the tile cost the same at both rates */
    const bool small = total_fr * SEA_WB_HOP * 2 < (2 << 20) || pool.size() <= 1;
    SlicePlan p;
    plan_call(p, lengths, n_utt, kIn, small);
    if (one_piece_elsewhere && p.K <= 1) return -1;
    for (int u = 0; u < n_utt; ++u) n_ceps[u] = 0;
    t_last_slices = 0;
    if (total_fr == 0) return 0;
    if (p.max_fr > 0x7fffffffLL - 8) return fail("%s: utterance %d is too long", who, p.idx[0]);
    const int K = t_last_slices = p.K;

    /* meta: the slices' offsets | lengths rows, then per slice the prefix sums of the capacities (nact + 1); ints: per piece the
     * count, then first_out per utterance; ceps: slice k's block starts at row foff[k] */
    const long long max_slice_fr = slice_max_frames(p);
    const size_t n_act = p.mbase[K] / 2;
    auto cum_base = [&](int k) { return p.mbase[K] + p.mbase[k] / 2 + (size_t)k; };
    HIP_TRY(w.in.ensure((size_t)(total_fr * kIn)));
    HIP_TRY(w.out.ensure((size_t)(total_fr * kOut)));
    HIP_TRY(w.meta.ensure(cum_base(K)));
    HIP_TRY(w.ints.ensure(n_act + (size_t)n_utt));
    HIP_TRY(w.ceps.ensure((size_t)total_fr * SEA_CC_NCEP));
    HIP_TRY(w.f32.ensure_device((size_t)(max_slice_fr * kOut)));
    HIP_TRY(w.ensure_state((size_t)n_utt * (WB ? sea::kWbSliceStateFloats : sea::kNsPipeStateFloats)));
    HIP_TRY(w.afe_state.ensure_device((size_t)n_utt * (WB ? sea::kWbCcStateFloats : sea::kCcStateFloats)));
    if (WB) {
        HIP_TRY(w.wb_rows.ensure_device(12 * ((size_t)max_slice_fr + 1)));
        HIP_TRY(w.ensure_inter((size_t)sea_wb_scratch_bytes(max_slice_fr * kIn, n_utt)));
    }
    for (int k = 0; k < K; ++k) {
        long long *cc = w.meta.h + cum_base(k);
        cc[0] = 0;
        for (int j = 0; j < p.nact[k]; ++j) cc[j + 1] = cc[j] + slice_piece_frames(p, k, j);
    }
    short *h_out = w.out.h;
    float *h_ceps = w.ceps.h;
    const int *h_cnt = w.ints.h;
    int *d_first = w.ints.d + n_act;
    float *d_hp = WB ? w.wb_rows.d : nullptr, *d_code = WB ? w.wb_rows.d + 3 * ((size_t)max_slice_fr + 1) : nullptr;

    return run_slices(
        w, pool, p, WB ? "wideband cepstrum slice" : "cepstrum slice", in, kIn, kOut, out != nullptr, false, small, cum_base(K), h_cnt,
        n_ceps,
        [&](const SliceView &v) {
            const long long *d_rows = v.d_rows, *d_cc = w.meta.d + cum_base(v.k);
            const int n = v.n;
            const short *d_in = w.in.d + kIn * v.f0;
            short *d_out = w.out.d + kOut * v.f0;
            float *d_blk = w.ceps.d + SEA_CC_NCEP * v.f0;
            int *d_cnt = w.ints.d + v.i0;
            if constexpr (WB) {
                if (sea_wb_denoise_batch_slice(d_in, d_out, w.f32.d, d_rows, d_rows + n, nullptr, d_first, nullptr, d_hp, d_code,
                                               (float *)w.inter.d, v.fr * kIn, w.state.d, n, v.frame_base, v.resume, v.sKern))
                    return 1;
                return sea_wb_compceps_batch_slice(w.f32.d, d_rows, d_rows + n, d_first, d_hp, d_code, d_cc, v.fr, d_blk, d_cnt,
                                                   w.afe_state.d, n, v.frame_base, v.resume, v.sKern);
            } else {
                if (sea_ns_denoise_batch_slice(d_in, d_out, w.f32.d, d_rows, d_rows + n, nullptr, d_first, w.state.d, n, v.frame_base,
                                               v.resume, v.sKern))
                    return 1;
                return sea_compceps_batch_slice(w.f32.d, d_rows, d_rows + n, d_first, d_cc, v.fr, d_blk, d_cnt, w.afe_state.d, n,
                                                v.frame_base, v.resume, v.sKern);
            }
        },
        [&](const SliceView &v) {
            HIP_TRY(hipMemcpyAsync(h_ceps + SEA_CC_NCEP * v.f0, w.ceps.d + SEA_CC_NCEP * v.f0, (size_t)v.fr * SEA_CC_NCEP * sizeof(float),
                                   hipMemcpyDeviceToHost, v.sDown));
            HIP_TRY(hipMemcpyAsync(w.ints.h + v.i0, w.ints.d + v.i0, (size_t)v.n * sizeof(int), hipMemcpyDeviceToHost, v.sDown));
            return 0;
        },
        [=](const SlicePiece &c) {
            if (out && out[c.u]) /* whole frames only: the trailing partial frame stays untouched, as with etsi_denoise */
                copy_stream(out[c.u] + kOut * c.b, h_out + kOut * c.f0, (size_t)(c.n * kOut) * sizeof(short));
            if (h_cnt[c.i] > 0)
                copy_stream(ceps[c.u] + SEA_CC_NCEP * c.start, h_ceps + SEA_CC_NCEP * c.f0, (size_t)h_cnt[c.i] * SEA_CC_NCEP * sizeof(float));
        });
}
extern "C" {

/* NoiseSup + CompCeps from host buffers: the explicit chain SURVEY 8(c) describes for the reference (DoNoiseSup into
 * the denoised-sample shift register, DoCompCeps on its last 201 samples from the third output on,
 * etsi/cpp/ParmInterface.c:275-293).  ceps[u] receives n_ceps[u] rows of 14 floats (c1..c12, c0, logE); its capacity
 * must be max(lengths[u]/80 - 6, 0) rows.  One launch each, no chunking: the path of a list the slice plan leaves in one piece
 * (sea_denoise_ceps_utterances below). */
static int denoise_ceps_one_launch(const short *const *in, short *const *out, float *const *ceps, int *n_ceps,
                                   const long *lengths, int n_utt)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    std::vector<long long> pre(n_utt + 1, 0), cum(n_utt + 1, 0);
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0) return fail("negative length for utterance %d", u);
        pre[u + 1] = pre[u] + align8(lengths[u]);
        cum[u + 1] = cum[u] + std::max<long long>(lengths[u] / 80 - 6, 0);
    }
    const long long total = pre[n_utt], total_ceps = cum[n_utt];
    for (int u = 0; u < n_utt; ++u) n_ceps[u] = 0;
    if (total == 0) return 0;
    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    HIP_TRY(w.in.ensure((size_t)total));
    HIP_TRY(w.out.ensure((size_t)total));
    HIP_TRY(w.meta.ensure(3 * (size_t)n_utt + 1));
    long long *offs = w.meta.h, *lens = w.meta.h + n_utt, *ccum = w.meta.h + 2 * n_utt;
    for (int u = 0; u < n_utt; ++u) {
        offs[u] = pre[u];
        lens[u] = lengths[u];
        memcpy(w.in.h + pre[u], in[u], (size_t)lengths[u] * sizeof(short));
        const long long pad = align8(lengths[u]) - lengths[u];
        if (pad) memset(w.in.h + pre[u] + lengths[u], 0, (size_t)pad * sizeof(short));
    }
    for (int u = 0; u <= n_utt; ++u) ccum[u] = cum[u];
    /* grow-only members of the workspace (round 3 allocated and freed five device buffers per call: an implicit device
     * synchronisation for every other host thread of the process, and the file driver calls this per chunk) */
    const size_t nceps_f = (size_t)std::max<long long>(total_ceps, 1) * 14;
    HIP_TRY(w.f32.ensure((size_t)total));
    HIP_TRY(w.ceps.ensure(nceps_f));
    HIP_TRY(w.ints.ensure(3 * (size_t)n_utt));
    int *d_first = w.ints.d, *d_nceps = w.ints.d + n_utt, *d_order = w.ints.d + 2 * n_utt;
    int *h_nceps = w.ints.h + n_utt, *h_order = w.ints.h + 2 * n_utt;
    launch_order(lens, n_utt, dc->n_cu, h_order);
    hipStream_t s = w.stream[0];
    /* from the first asynchronous call on every exit path drains the stream (Scope: ok stays false on a fault), so no copy
     * into w's pinned staging or kernel over w's device buffers is still in flight when the caller gets its fault code */
    Scope scope(&w);
    HIP_TRY(hipMemcpyAsync(w.in.d, w.in.h, (size_t)total * sizeof(short), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.meta.d, w.meta.h, (3 * (size_t)n_utt + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_order, h_order, (size_t)n_utt * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_nceps, 0, (size_t)n_utt * sizeof(int), s));
    if (sea_ns_denoise_batch(w.in.d, w.out.d, w.f32.d, w.meta.d, w.meta.d + n_utt, n_utt > 1 ? d_order : nullptr, d_first,
                             n_utt, s))
        return 1;
    if (total_ceps > 0 && sea_compceps_batch(w.f32.d, w.meta.d, w.meta.d + n_utt, d_first, w.meta.d + 2 * n_utt, total_ceps,
                                             w.ceps.d, d_nceps, n_utt, s))
        return 1;
    HIP_TRY(hipMemcpyAsync(w.out.h, w.out.d, (size_t)total * sizeof(short), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(w.ceps.h, w.ceps.d, nceps_f * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_nceps, d_nceps, (size_t)n_utt * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    scope.ok = true;
    for (int u = 0; u < n_utt; ++u) {
        n_ceps[u] = h_nceps[u];
        memcpy(out[u], w.out.h + pre[u], (size_t)(lengths[u] / 80 * 80) * sizeof(short));
        if (n_ceps[u] > 0) memcpy(ceps[u], w.ceps.h + (size_t)cum[u] * 14, (size_t)n_ceps[u] * 14 * sizeof(float));
    }
    return 0;
}

/* the lists the slice plan cuts go through the pipeline unless SEA_HOST_CEPS_PIPELINE=0 */
static bool ceps_pipeline_on()
{
    const char *e = getenv("SEA_HOST_CEPS_PIPELINE");
    return !(e && e[0] == '0');
}

static int ceps_args_ok(const char *who, const void *in, const void *out, bool out_required, float *const *ceps, const int *n_ceps,
                        const long *lengths, int n_utt)
{
    if (!in || (out_required && !out) || !ceps || !n_ceps || !lengths)
        return fail(out_required ? "%s: in, out, ceps, n_ceps and lengths are required" : "%s: in, ceps, n_ceps and lengths are required", who);
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < 0) return fail("%s: negative length for utterance %d", who, u);
        if (!ceps[u]) return fail("%s: ceps[%d] is NULL", who, u);
    }
    return 0;
}

/* NoiseSup + CompCeps from host buffers (include/sea_mi355x.h).  A list the slice plan cuts runs the pipeline above; a list in
 * one piece -- small lists -- keeps the one launch each. */
int sea_denoise_ceps_utterances(const short *const *in, short *const *out, float *const *ceps, int *n_ceps,
                                const long *lengths, int n_utt)
{
    const char *who = "sea_denoise_ceps_utterances";
    if (n_utt <= 0) return 0;
    if (ceps_args_ok(who, in, out, true, ceps, n_ceps, lengths, n_utt)) return 1;
    if (ceps_pipeline_on()) {
        const int rc = denoise_ceps_slices<false>(who, in, out, ceps, n_ceps, lengths, n_utt, true);
        if (rc >= 0) return rc;
    }
    t_last_slices = 0;
    const int rc = denoise_ceps_one_launch(in, out, ceps, n_ceps, lengths, n_utt);
    if (!rc && slice_total_frames(lengths, n_utt, SEA_HOP) > 0) t_last_slices = 1;
    return rc;
}

/* The wideband mode's: one path, the slice kernels', also for a list that is not cut (as sea_wb_features_utterances). */
int sea_wb_denoise_ceps_utterances(const short *const *in, short *const *out_lp, float *const *ceps, int *n_ceps,
                                   const long *lengths, int n_utt)
{
    const char *who = "sea_wb_denoise_ceps_utterances";
    if (n_utt <= 0) return 0;
    if (ceps_args_ok(who, in, out_lp, false, ceps, n_ceps, lengths, n_utt)) return 1;
    return denoise_ceps_slices<true>(who, in, out_lp, ceps, n_ceps, lengths, n_utt, false);
}

/* ---------------------------------------------------------------------------------------------------- */
/* The [time][64] float intermediate costs 256 B of HBM per sample (~16 MB per 4-s utterance).  The chunks of the
 * pipeline run on kStreams streams, each with a scratch region of its own, sized so that all regions together fit
 * in 60 % of the HBM that is free right now (SEA_RESYNTH_SCRATCH_MB overrides the budget); a chunk is at most what
 * one region holds.  The reference processes one utterance at a time (resyth_64sub_ori/cpp/main.cpp:84-145);
 * results do not depend on the cut. */
int sea_resynth_utterances(const short *const *in, const long *lengths, const float *const *masks, int binary,
                           short *const *out, int n_utt)
{
    if (n_utt <= 0) return 0;
    DeviceCtx *dc;
    if (ctx(&dc)) return 1;
    auto nrows = [&](long L) -> long long { return (binary & 2) ? L / 160 : (L - 320) / 160 + 1; };
    long long largest = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (lengths[u] < ((binary & 2) ? 160 : 320))
            return fail("resynth: utterance %d has %ld samples (too short for one mask frame)", u, lengths[u]);
        largest = std::max(largest, sea_resynth_scratch_bytes(align8(lengths[u]), 1));
    }
    std::vector<int> idx(n_utt);
    for (int i = 0; i < n_utt; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lengths[a] > lengths[b]; });
    std::vector<long long> pre(n_utt + 1, 0), rpre(n_utt + 1, 0);
    for (int j = 0; j < n_utt; ++j) {
        pre[j + 1] = pre[j] + align8(lengths[idx[j]]);
        rpre[j + 1] = rpre[j] + nrows(lengths[idx[j]]);
    }
    const long long total = pre[n_utt], rows = rpre[n_utt];

    PipeWs &w = t_ws;
    HIP_TRY(w.bind());
    Pool &pool = Pool::get(w.device);
    long long budget;
    if (scratch_budget("SEA_RESYNTH_SCRATCH_MB", &budget, w.inter.dcap)) return 1;
    /* regions: as many streams as there will be chunks, each at least one utterance */
    long long region = std::max(largest, budget / kStreams);
    /* chunk = at most a region's worth of scratch and about SEA_HOST_CHUNK_MB of (int16 + mask) input */
    std::vector<int> cuts(1, 0);
    {
        /* default: about a quarter of the list per chunk (few large launches fill the chip better than many small ones) */
        const long long in_target = getenv("SEA_HOST_CHUNK_MB") ? env_mb("SEA_HOST_CHUNK_MB", 24) * (1 << 20)
                                                                : std::max<long long>((total * 4 + rows * 256 + 3) / 4, 1 << 20);
        long long run = 0, run_bytes = 0;
        int run_n = 0;
        for (int j = 0; j < n_utt; ++j) {
            const long long Lp = align8(lengths[idx[j]]);
            const long long b = Lp * 4 + nrows(lengths[idx[j]]) * 256;
            const bool over = sea_resynth_scratch_bytes(run + Lp, run_n + 1) > region || run_bytes + b > in_target ||
                              run_n >= 4 * dc->n_cu;
            if (run_n > 0 && over && (int)cuts.size() < kMaxChunks) {
                cuts.push_back(j);
                run = run_bytes = 0;
                run_n = 0;
            }
            run += Lp;
            run_bytes += b;
            run_n++;
        }
        cuts.push_back(n_utt);
    }
    const int nchunk = (int)cuts.size() - 1;
    /* a region is as large as the largest chunk (the last one can exceed the budget share when kMaxChunks is reached:
     * hipMalloc then reports what does not fit) */
    region = 0;
    for (int k = 0; k < nchunk; ++k)
        region = std::max(region, sea_resynth_scratch_bytes(pre[cuts[k + 1]] - pre[cuts[k]], cuts[k + 1] - cuts[k]));
    const int nregion = std::min(nchunk, kStreams);
    HIP_TRY(w.ensure_inter((size_t)region * nregion));
    HIP_TRY(w.in.ensure((size_t)total));
    HIP_TRY(w.out.ensure((size_t)total));
    HIP_TRY(w.mask.ensure((size_t)rows * 64));
    HIP_TRY(w.meta.ensure(3 * (size_t)n_utt));
    long long *offs = w.meta.h, *lens = w.meta.h + n_utt, *moffs = w.meta.h + 2 * n_utt;
    for (int k = 0; k < nchunk; ++k)
        for (int j = cuts[k]; j < cuts[k + 1]; ++j) {
            /* sample offsets are relative to the chunk (the scratch region is indexed by them), buffers are sliced */
            offs[j] = pre[j] - pre[cuts[k]];
            lens[j] = lengths[idx[j]];
            moffs[j] = rpre[j] - rpre[cuts[k]];
        }
    const bool small = (total * 4 + rows * 256) < (2 << 20) || n_utt == 1 || pool.size() <= 1;

    std::vector<Latch> packed(nchunk);
    Scope scope(&w);
    short *h_in = w.in.h, *h_out = w.out.h;
    float *h_mask = w.mask.h;
    std::vector<long long> bytes_pre(n_utt + 1);
    for (int j = 0; j <= n_utt; ++j) bytes_pre[j] = pre[j] * 2 + rpre[j] * 256;
    const long long *bp = bytes_pre.data(), *prep = pre.data(), *rprep = rpre.data();
    const int *ix = idx.data();
    for (int k = 0; k < nchunk; ++k)
        run_copies(pool, cuts[k], cuts[k + 1], bp, &packed[k], &scope.all, small, [=](int j) {
            const long long L = lens[j];
            copy_stream(h_in + prep[j], in[ix[j]], (size_t)L * sizeof(short));
            const long long pad = align8(L) - L;
            if (pad) memset(h_in + prep[j] + L, 0, (size_t)pad * sizeof(short));
            copy_stream(h_mask + rprep[j] * 64, masks[ix[j]], (size_t)(rprep[j + 1] - rprep[j]) * 64 * sizeof(float));
        });
    HIP_TRY(hipMemcpyAsync(w.meta.d, w.meta.h, 3 * (size_t)n_utt * sizeof(long long), hipMemcpyHostToDevice, w.stream[0]));
    HIP_TRY(hipEventRecord(w.ev_meta, w.stream[0]));

    /* a chunk reuses the scratch region and the stream of chunk k - nregion: stream order protects the region.  Uploads do
     * not wait for each other: the kernel is six times the copies */
    return run_pipeline(
        w, scope, packed, "resynthesis chunk", false,
        [&](int k) {
            const int r = k % nregion;
            hipStream_t s = w.stream[r];
            const int u0 = cuts[k], n = cuts[k + 1] - cuts[k];
            const long long o0 = pre[u0], cnt = pre[cuts[k + 1]] - o0, r0 = rpre[u0], rcnt = rpre[cuts[k + 1]] - r0;
            if (k > 0 && k < nregion) HIP_TRY(hipStreamWaitEvent(s, w.ev_meta, 0));
            HIP_TRY(hipMemcpyAsync(w.in.d + o0, h_in + o0, (size_t)cnt * sizeof(short), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(w.mask.d + r0 * 64, h_mask + r0 * 64, (size_t)rcnt * 64 * sizeof(float), hipMemcpyHostToDevice, s));
            if (sea_resynth64_batch(w.in.d + o0, w.out.d + o0, w.meta.d + u0, w.meta.d + n_utt + u0, w.mask.d + r0 * 64,
                                    w.meta.d + 2 * n_utt + u0, (float *)(w.inter.d + (size_t)r * region), nullptr, n, binary, s))
                return 1;
            HIP_TRY(hipEventRecord(w.ev_kernel[k], s));
            return 0;
        },
        [&](int k) {
            const long long o0 = pre[cuts[k]], cnt = pre[cuts[k + 1]] - o0;
            hipStream_t s = w.stream[k % nregion];
            HIP_TRY(hipMemcpyAsync(h_out + o0, w.out.d + o0, (size_t)cnt * sizeof(short), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(w.ev_done[k], s));
            return 0;
        },
        [&](int k) {
            run_copies(pool, cuts[k], cuts[k + 1], bp, nullptr, &scope.all, small,
                       [=](int j) { copy_stream(out[ix[j]], h_out + prep[j], (size_t)lens[j] * sizeof(short)); });
        });
}

} // extern "C"
