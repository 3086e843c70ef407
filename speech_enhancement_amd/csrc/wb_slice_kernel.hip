/*
 * wb_slice_kernel.hip -- the wideband (16 kHz) mode over one TIME SLICE of every utterance (include/sea_mi355x.h,
 * sea_wb_denoise_batch_slice; the state's layout: sea_kernels.h, kWbSliceStateFloats).
 *
 * wb_kernel.hip's three kernels each have a form here that takes what lies before the slice from a per-utterance state
 * instead of from the same launch's buffers, and the low-band frame loop has its own (ns_pipe_kernel.hip,
 * ns_denoise_pipe_wb_slice_kernel).  The arithmetic of a frame -- the QMF sums, the dual transform with the band sums and the
 * code, one step of DoSpecSub16k -- is restated here statement for statement as three inline functions; the whole-utterance
 * kernels keep their own text, because calling shared functions from them changed their register allocation, and they are to
 * come out of the compiler as they were.  tests/test_gpu_wb_slices.py holds the two texts together: the slices of an
 * utterance must give the bits of the one launch.
 *
 * What is carried, and who stores it.  wb_qmf_slice_kernel and wb_hb_slice_kernel stride over a slice's frames with many
 * workgroups per utterance, so they only READ the state; the slice's last launch, wb_slice_end_kernel (one workgroup per
 * utterance), runs the spectral subtraction's tracker over the slice's rows and then writes every wideband part of the state.
 */
#include "ns_core.h"

namespace sea {

/* output k of one frame's two bands from the staged window x[0 .. 276] (x[117] is the frame's first sample) */
__device__ __forceinline__ void wb_qmf_filter(const float *x, const float *tap, int k, float *lp, float *hp)
{
    const float *w = x + 2 * k;
    float aux1 = 0.0f, aux2 = 0.0f;
#pragma unroll 2
    for (int j = 0; j < SEA_WB_QMF; j += 2) {
        const float p0 = w[j] * tap[j], p1 = w[j + 1] * tap[j + 1];
        aux1 += p0;
        aux2 += -p0; /* high-pass tap j even: -low-pass */
        aux1 += p1;
        aux2 += p1;  /* j odd: +low-pass */
    }
    lp[k] = aux1;
    hp[k] = (k & 1) ? -aux2 : aux2;
}

/* one output frame from its two staged windows (bufA / bufB [60 .. 259]): the raw band energies into its row of hp_rows, the
 * nine code values into its row of code_rows */
__device__ __forceinline__ void wb_hb_output(float *bufA, float *bufB, float *work, float *psdA, float *psdB, float *logs,
                                             const Fft2Regs &fft, const float (&win8)[8], const sea_wb_tables *wb, float floorSpec,
                                             float *hp_rows, float *code_rows, long long row, int lane)
{
    wave_sync();
    ns_front_dual<false>(bufA, true, psdA, bufB, true, psdB, work, fft, win8, lane);
    float v = 0.0f;
    if (lane < 3) { /* GetBandsForCoding16k, 16kHzProcessing.c:497-510 */
        const int b0 = lane == 0 ? 33 : (lane == 1 ? 39 : 49), b1 = lane == 0 ? 39 : (lane == 1 ? 49 : 65);
        for (int i = b0; i < b1; ++i) v += psdA[i];
    } else if (lane < 6) { /* DoMelFB, MelProc.c:82-104 */
        const int b = lane - 3, st = wb->hpMelStart[b], n = wb->hpMelLen[b];
        for (int i = 0; i < n; ++i) v += psdB[st + i] * wb->hpMelW[b][i];
        hp_rows[row * 3 + b] = v;
    }
    if (lane < 6) logs[lane] = (v > floorSpec) ? ns_logf(v) : -10.0f; /* NoiseSup.c:1230-1233, :1320-1323 */
    wave_sync();
    if (lane < 9) code_rows[row * 9 + lane] = logs[lane % 3] - logs[3 + lane / 3]; /* code[3 i + j] = lpBands[j] - fb16k[i] */
    wave_sync();
}

/* DoSpecSub16k's state between two output frames, and one frame of it on a row of raw band energies (in place) */
struct WbSubState {
    float noise[3] = {0.0f, 0.0f, 0.0f}, meanEn = 0.0f;
    int nbSpeech = 0, hangOver = 0;
};
__device__ __forceinline__ void wb_specsub_step(WbSubState &s, int nbFrame, float *row, float eps, float logMin)
{
    const float lambdaNSE = nbFrame < 100 ? (float)(1.0 - 1.0 / (double)(float)nbFrame) : (float)0.99;
    float in[3] = {row[0], row[1], row[2]};
    float frameEn = 0.0f;
    for (int i = 0; i < 3; ++i) frameEn += in[i];
    frameEn = ((double)frameEn > 0.001) ? ns_logf(frameEn) : logMin;
    if (((double)(frameEn - s.meanEn) < 1.2) || nbFrame < 10) {
        if (nbFrame < 10) s.meanEn += (1 - lambdaNSE) * (frameEn - s.meanEn);
        else if (frameEn < s.meanEn) s.meanEn = (float)((double)s.meanEn + (1 - 0.98) * (double)(frameEn - s.meanEn));
        else s.meanEn = (float)((double)s.meanEn + (1 - 0.995) * (double)(frameEn - s.meanEn));
    }
    int flagVAD;
    if ((double)(frameEn - s.meanEn) > 2.2) {
        flagVAD = 1;
        s.nbSpeech++;
    } else {
        if (s.nbSpeech > 4) s.hangOver = 15;
        s.nbSpeech = 0;
        if (s.hangOver != 0) {
            s.hangOver--;
            flagVAD = 1;
        } else
            flagVAD = 0;
    }
    if (flagVAD == 0) {
        for (int i = 0; i < 3; ++i) {
            if (nbFrame < 10 || in[i] < s.noise[i]) s.noise[i] = lambdaNSE * s.noise[i] + (1 - lambdaNSE) * in[i];
            else s.noise[i] = (float)(0.995 * (double)s.noise[i] + (1 - 0.995) * (double)in[i]);
            if (s.noise[i] < eps) s.noise[i] = eps;
        }
    }
    for (int i = 0; i < 3; ++i) {
        const float floor = (float)(0.1 * (double)in[i]);
        const float diff = (float)((double)in[i] - 1.5 * (double)s.noise[i]);
        row[i] = diff > floor ? diff : floor;
    }
}

/* the first non-zero frame so far, absolute: the smaller of what the earlier slices left and what this slice's QMF found */
__device__ __forceinline__ int wb_slice_onset(const WbSliceArgs &a, const float *st, int u)
{
    int onset = a.q.onset[u];
    if (a.resume) {
        const int before = __float_as_int(st[kWbStOnset]);
        if (before < onset) onset = before;
    }
    return onset;
}

/* wb_qmf_kernel with the delay line of the slice's first frame taken from the state (zeros in a first slice) and the onset
 * as an absolute frame index */
__global__ __launch_bounds__(kWbQmfThreads) void wb_qmf_slice_kernel(WbSliceArgs a)
{
    constexpr int kHist = SEA_WB_QMF - 1;
    constexpr int kWin = SEA_WB_HOP + kHist;
    __shared__ float x[kWin + 3];
    __shared__ float tap[SEA_WB_QMF + 2];
    const int u = blockIdx.x;
    const long long off = a.q.offsets[u];
    const long long nfr = a.q.lengths[u] / SEA_WB_HOP;
    const int16_t *in = a.q.in + off;
    const float *hist = a.state + (size_t)u * kWbSliceStateFloats + kWbStQmf;
    const bool resume = a.resume != 0;
    float *lp = a.q.lp + off / 2, *hp = a.q.hp + off / 2;
    for (int j = threadIdx.x; j < SEA_WB_QMF; j += kWbQmfThreads) tap[j] = a.q.tables->qmfLp[j];
    for (long long f = blockIdx.y; f < nfr; f += gridDim.y) {
        const long long base = f * SEA_WB_HOP - kHist;
        int nonzero = 0;
        for (int i = threadIdx.x; i < kWin; i += kWbQmfThreads) {
            const long long p = base + i; /* -117 <= p < 160 (f + 1) <= lengths[u] */
            const int16_t s = p >= 0 ? in[p] : (int16_t)0;
            x[i] = p >= 0 ? (float)s : (resume ? hist[kHist + p] : 0.0f);
            nonzero |= (i >= kHist && s != 0) ? 1 : 0;
        }
        if (__syncthreads_or(nonzero) && threadIdx.x == 0) atomicMin(a.q.onset + u, a.frame_base + (int)f);
        if (threadIdx.x < SEA_HOP) wb_qmf_filter(x, tap, threadIdx.x, lp + f * SEA_HOP, hp + f * SEA_HOP);
        __syncthreads();
    }
}

/* wb_hb_kernel over the slice's frames that have an output, F = frame_base + local frame >= onset + 4.  Its windows start at
 * sample 60 of low-band frame F - 5 and at high-band frame F - 4, absolute: what lies before the slice comes from the five
 * frames the state keeps of either stream (zeros in a first slice), what lies before the onset is zero as in the one launch. */
__global__ __launch_bounds__(64) void wb_hb_slice_kernel(WbSliceArgs a)
{
    __shared__ __attribute__((aligned(16))) float bufA[320], bufB[320], work[512], psdA[68], psdB[68], logs[8];
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const long long off2 = a.q.offsets[u] / 2;
    const long long nfr = a.q.lengths[u] / SEA_WB_HOP;
    const float *st = a.state + (size_t)u * kWbSliceStateFloats;
    const bool resume = a.resume != 0;
    const long long onset = wb_slice_onset(a, st, u);
    const long long fb = a.frame_base, fEnd = fb + nfr;
    const long long fFirst = onset + 4 > fb ? onset + 4 : fb; /* no onset yet: beyond fEnd */
    if (fFirst >= fEnd) return;
    const long long row0 = (a.q.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP - fb; /* + F: the row of frame F */
    Fft2Regs fft;
    load_fft2_regs<false>(fft, &a.ns->fft, lane, nullptr);
    float win8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) win8[k] = a.ns->win8[k][lane];
    const float *lp = a.q.lp + off2, *hp = a.q.hp + off2;
    const float floorSpec = a.q.tables->floorSpec;
    /* sample s (absolute, 8 kHz rate) of a stream: the slice's own at s - 80 fb, the state's 400 end at 80 fb */
    auto fetch = [&](const float *cur, int part, long long s) {
        const long long loc = s - fb * SEA_HOP; /* -340 <= loc < 80 nfr */
        return loc >= 0 ? cur[loc] : (resume ? st[part + 5 * SEA_HOP + loc] : 0.0f);
    };
    for (long long F = fFirst + blockIdx.y; F < fEnd; F += gridDim.y) {
        for (int j = lane; j < 320; j += kLanes) { /* the transforms read buf[60 .. 259] */
            const int i = j - 60;
            const long long ia = (F - 5) * SEA_HOP + j, ib = (F - 4) * SEA_HOP + i; /* < 80 (F - 1) < 80 fEnd */
            const bool in = i >= 0 && i < SEA_WIN;
            bufA[j] = (in && ia >= onset * SEA_HOP) ? fetch(lp, kWbStLp, ia) : 0.0f;
            bufB[j] = in ? fetch(hp, kWbStHp, ib) : 0.0f;
        }
        wb_hb_output(bufA, bufB, work, psdA, psdB, logs, fft, win8, a.q.tables, floorSpec, a.hp_rows, a.code_rows, row0 + F, lane);
    }
}

/* The slice's last launch, one workgroup per utterance.  Thread 0 runs DoSpecSub16k over the rows of the slice's outputs from
 * where the previous slice left the tracker (nbFrame is the output's absolute number).  Then every part of the state beyond
 * the frame loop's blob is written for the next slice: the delay line and the two five-frame histories are what they were,
 * shifted by the slice's frames, with the slice's own samples behind them -- read first, stored after a barrier. */
__global__ __launch_bounds__(128) void wb_slice_end_kernel(WbSliceArgs a)
{
    constexpr int kHist = SEA_WB_QMF - 1, kKeep = 5 * SEA_HOP, kPer = (kKeep + 127) / 128;
    const int t = threadIdx.x;
    const int u = blockIdx.x;
    const long long off = a.q.offsets[u];
    const long long nfr = a.q.lengths[u] / SEA_WB_HOP;
    float *st = a.state + (size_t)u * kWbSliceStateFloats;
    const bool resume = a.resume != 0;
    const int onset = wb_slice_onset(a, st, u);
    const long long fb = a.frame_base;
    if (t == 0) {
        WbSubState s;
        long long count = 0;
        if (resume) {
            s.noise[0] = st[kWbStSub + 0]; s.noise[1] = st[kWbStSub + 1]; s.noise[2] = st[kWbStSub + 2];
            s.meanEn = st[kWbStSub + 3];
            s.nbSpeech = __float_as_int(st[kWbStSub + 4]);
            s.hangOver = __float_as_int(st[kWbStSub + 5]);
            count = __float_as_int(st[kWbStSub + 6]);
        }
        const long long kEnd = fb + nfr - onset - 4; /* outputs so far, this slice included */
        if (a.hp_rows && onset != kWbNoOnset && kEnd > 0) {
            const float eps = a.q.tables->floorSpec, logMin = a.q.tables->logMin16k;
            long long k = fb - onset - 4; /* the first output whose frame lies in this slice ... */
            if (k < count) k = count;     /* ... which is where the tracker stands */
            float *row = a.hp_rows + ((off + SEA_WB_HOP - 1) / SEA_WB_HOP + (onset + 4 + k - fb)) * 3;
            for (; k < kEnd; ++k, row += 3)
                wb_specsub_step(s, k + 1 < 2147483647LL ? (int)(k + 1) : 2147483647, row, eps, logMin);
            if (count < kEnd) count = kEnd;
        }
        st[kWbStSub + 0] = s.noise[0]; st[kWbStSub + 1] = s.noise[1]; st[kWbStSub + 2] = s.noise[2];
        st[kWbStSub + 3] = s.meanEn;
        st[kWbStSub + 4] = __int_as_float(s.nbSpeech);
        st[kWbStSub + 5] = __int_as_float(s.hangOver);
        st[kWbStSub + 6] = __int_as_float((int)count);
        st[kWbStSub + 7] = 0.0f;
    }
    /* element i of a history of n is element i + m of (old history, the slice's m new samples) */
    const long long m16 = nfr * SEA_WB_HOP, m8 = nfr * SEA_HOP;
    const int16_t *in = a.q.in + off;
    const float *lp = a.q.lp + off / 2, *hp = a.q.hp + off / 2;
    float q = 0.0f, vl[kPer], vh[kPer];
    if (t < kHist) {
        const long long j = t + m16;
        q = j >= kHist ? (float)in[j - kHist] : (resume ? st[kWbStQmf + j] : 0.0f);
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int i = t + 128 * r;
        const long long j = i + m8;
        vl[r] = vh[r] = 0.0f;
        if (i < kKeep) {
            vl[r] = j >= kKeep ? lp[j - kKeep] : (resume ? st[kWbStLp + j] : 0.0f);
            vh[r] = j >= kKeep ? hp[j - kKeep] : (resume ? st[kWbStHp + j] : 0.0f);
        }
    }
    __syncthreads();
    if (t < kHist) st[kWbStQmf + t] = q;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int i = t + 128 * r;
        if (i < kKeep) {
            st[kWbStLp + i] = vl[r];
            st[kWbStHp + i] = vh[r];
        }
    }
    if (t == 0) {
        st[kWbStOnset] = __int_as_float(onset);
        st[kWbStOnset + 1] = st[kWbStOnset + 2] = 0.0f;
    }
}

} // namespace sea
