/*
 * slice_plan.h -- how the host pipelines cut a list of utterances along the TIME axis (hostpipe.hip: run_slices and
 * sea_packed_plan), and where the rows a slice emits go in the caller's arrays (RowOrder).  Integer arithmetic only, no HIP:
 * tests/slice_plan_driver.cpp runs it on a CPU.
 *
 * The utterances are sorted longest first (stable), utterance idx[j] at position j with nfr[j] = length / hop whole frames.
 * Slice k holds the frames [B[k], B[k+1]) of every utterance that has them: the first nact[k] positions.  The boundaries give
 * the slices equal shares of the frames: B[k] is the smallest f > B[k-1] with sum_j min(nfr[j], f) >= total_fr * k / want,
 * boundaries stop at the first such f >= max_fr, and the last one is max_fr.
 */
#pragma once
#include <algorithm>
#include <vector>

namespace sea_capi {

constexpr int kMaxSlices = 64;

struct SlicePlan {
    std::vector<int> idx, inv;   /* idx[j]: the utterance at sorted position j; inv[idx[j]] == j */
    std::vector<long long> nfr;  /* whole frames, by sorted position */
    std::vector<long long> B;    /* K + 1 boundaries in frames, 0 .. max_fr */
    std::vector<int> nact;       /* utterances that reach slice k */
    std::vector<long long> foff; /* K + 1: where slice k starts in a staging that holds the slices one after the other, in frames */
    std::vector<size_t> mbase;   /* K + 1: where slice k's offsets | lengths rows start in the meta array */
    int K = 0;                   /* slices; 0 for a list without a whole frame */
    long long total_fr = 0, max_fr = 0;
};

/* whole frames of the list: what a caller's "too small to cut" test needs before it asks for a plan */
inline long long slice_total_frames(const long *lengths, int n_utt, long long hop)
{
    long long s = 0;
    for (int u = 0; u < n_utt; ++u) s += lengths[u] / hop;
    return s;
}

/* at most min(want, kMaxSlices, max(1, max_fr / 8)) slices */
inline void slice_plan(SlicePlan &p, const long *lengths, int n_utt, long long hop, int want)
{
    p.idx.resize(n_utt);
    p.inv.resize(n_utt);
    p.nfr.resize(n_utt);
    for (int i = 0; i < n_utt; ++i) p.idx[i] = i;
    std::stable_sort(p.idx.begin(), p.idx.end(), [&](int a, int b) { return lengths[a] > lengths[b]; });
    p.total_fr = 0;
    for (int j = 0; j < n_utt; ++j) {
        p.inv[p.idx[j]] = j;
        p.total_fr += (p.nfr[j] = lengths[p.idx[j]] / hop);
    }
    p.max_fr = n_utt > 0 ? p.nfr[0] : 0;
    p.K = 0;
    p.B.assign(1, 0);
    p.nact.clear();
    p.foff.assign(1, 0);
    p.mbase.assign(1, 0);
    if (p.total_fr == 0) return;
    want = (int)std::min<long long>(std::min(want, kMaxSlices), std::max<long long>(1, p.max_fr / 8));
    auto frames_below = [&](long long f) {
        long long s = 0;
        for (int j = 0; j < n_utt; ++j) s += std::min(p.nfr[j], f);
        return s;
    };
    for (int k = 1; k < want; ++k) {
        long long lo = p.B.back() + 1, hi = p.max_fr; /* smallest f with frames_below(f) >= share */
        const long long share = p.total_fr * k / want;
        while (lo < hi) {
            const long long mid = (lo + hi) / 2;
            if (frames_below(mid) >= share) hi = mid; else lo = mid + 1;
        }
        if (lo >= p.max_fr) break;
        p.B.push_back(lo);
    }
    p.B.push_back(p.max_fr);
    p.K = (int)p.B.size() - 1;
    for (int k = 0; k < p.K; ++k) {
        int n = 0;
        long long fr = 0;
        for (; n < n_utt && p.nfr[n] > p.B[k]; ++n) fr += std::min(p.nfr[n], p.B[k + 1]) - p.B[k];
        p.nact.push_back(n);
        p.foff.push_back(p.foff[k] + fr);
        p.mbase.push_back(p.mbase[k] + 2 * (size_t)n);
    }
}

/* frames of sorted position j in slice k (j < nact[k]) */
inline long long slice_piece_frames(const SlicePlan &p, int k, int j) { return std::min(p.nfr[j], p.B[k + 1]) - p.B[k]; }

/* frames of the largest slice: what a device buffer that holds one slice at a time is sized for */
inline long long slice_max_frames(const SlicePlan &p)
{
    long long m = 0;
    for (int k = 0; k < p.K; ++k) m = std::max(m, p.foff[k + 1] - p.foff[k]);
    return m;
}

/* Slice k as the kernels read it: rows[0 .. nact) the pieces' offsets, rows[nact .. 2 nact) their lengths, both in samples of
 * `hop` per frame.  Offsets count from the start of the staging (absolute: one batch, launched slice by slice) or from the
 * start of the slice (a batch of its own).  bytes_prefix, where given, receives nact + 1 running sums of the pieces' int16
 * bytes, for cutting the copies into tasks. */
inline void slice_rows(const SlicePlan &p, int k, long long hop, bool absolute, long long *rows, long long *bytes_prefix)
{
    const int n = p.nact[k];
    long long o = absolute ? hop * p.foff[k] : 0;
    if (bytes_prefix) bytes_prefix[0] = 0;
    for (int j = 0; j < n; ++j) {
        const long long L = hop * slice_piece_frames(p, k, j);
        rows[j] = o;
        rows[n + j] = L;
        o += L;
        if (bytes_prefix) bytes_prefix[j + 1] = bytes_prefix[j] + 2 * L;
    }
}

/* Where the rows that the slices emit go in the caller's per-utterance arrays.  A pipeline whose slices emit a number of rows
 * per utterance that only the device knows (feature rows, cepstral rows) places an utterance's rows of slice k behind those of
 * its earlier slices, so where they go is known once the counts of slices 0 .. k - 1 are on the host.  The event loop that
 * brings them there (hostpipe.hip: run_pipeline) promises no order among the slices: one pass of it may find slice k's kernel
 * or download event "not ready" and slice k + 1's done, so both the download and the unpacking of slice k + 1 may come before
 * slice k's.  arrive (k) therefore only notes that slice k is on the host; the slices are CUT -- their start rows fixed, their
 * copy tasks handed out -- strictly in slice order, each as soon as it and every slice before it have arrived, from a running
 * sum that by then holds exactly the earlier slices' counts.  The copy tasks need no order among themselves.
 * start[k] is what those tasks read: it is written once, when slice k is cut, and must outlive them. */
struct RowOrder {
    std::vector<long long> pos;                /* rows of sorted position j in the slices before next_cut */
    std::vector<std::vector<long long>> start; /* per cut slice: where each of its utterances' rows go */
    std::vector<char> arrived;                 /* slice k's rows and counts are on the host */
    int next_cut = 0;                          /* the first slice that is not cut yet */

    RowOrder(int K, int n_utt) : pos(n_utt, 0), start(K), arrived(K, 0) {}

    /* Slice arrived_k is on the host; counts holds the rows every piece emitted, slice k's nact[k] at counts + mbase[k] / 2.
     * Calls cut(k, start[k].data()) for every slice that can be cut now, in slice order.  Once every slice has arrived, pos[j]
     * is the total of sorted position j. */
    template <class Cut>
    void arrive(const SlicePlan &p, int arrived_k, const int *counts, Cut cut)
    {
        arrived[arrived_k] = 1;
        for (; next_cut < p.K && arrived[next_cut]; ++next_cut) {
            const int k = next_cut, n = p.nact[k];
            const int *cnt = counts + p.mbase[k] / 2;
            start[k].resize(n);
            for (int j = 0; j < n; ++j) { /* pos: the counts of slices 0 .. k - 1, all arrived */
                start[k][j] = pos[j];
                pos[j] += cnt[j];
            }
            cut(k, start[k].data());
        }
    }
};

} // namespace sea_capi
