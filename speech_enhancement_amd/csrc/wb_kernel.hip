/*
 * wb_kernel.hip -- the ETSI wideband (16 kHz) mode: the QMF split and the high band's features.
 *
 * ES 202 050's 16 kHz mode (AdvProcessAlloc (16000), etsi/cpp/ParmInterface.c:100-108) reads frames of 160 samples and
 * splits each with a 118-tap QMF pair, computing every second output, into 80 low-band samples (0-4 kHz) and 80
 * high-band samples shifted down to 0-4 kHz by (-1)^k (Do16kProcessing, etsi/cpp/16kHzProcessing.c:711-774).  The filter's
 * delay line holds the last 117 input samples and starts as zeros; frames before the first non-zero one do not reach it
 * (ParmInterface.c:250-260), and being all zeros they would not change it: the split is a plain FIR over the raw input
 * with zero history, every frame independent of every other.  One workgroup takes one frame at a time:
 *
 *   stage   the 277 samples x[160 f - 117 .. 160 f + 159] as floats in LDS (zeros before the utterance's start); the same
 *           pass finds whether the frame's own 160 samples hold a non-zero one (the zero-frame gate's test,
 *           ParmInterface.c:244-250: a sum of squares that is zero only for an all-zero frame) -> atomicMin into onset
 *   filter  lane k < 80 adds the 118 products x[2k + j] * tap[j] in the reference's order j = 0..117, multiply then
 *           add (no contraction: the unit is built with -ffp-contract=off), starting from 0.0f as the reference does.
 *           The high-pass tap j is the low-pass tap j with the sign (-1)^(j+1) (sea_tables.c), and x * (-t) = -(x * t)
 *           exactly, so one product feeds both sums.  The down-shift sign restarts at every frame (hpSign = 1, :740).
 *
 * The low band then runs through the NoiseSup frame loop with a float intake (ns_pipe_kernel.hip, ns_denoise_pipe_wb_kernel).
 * Nothing of the high band feeds back into it, and the high band takes only two things from it: the RAW first-stage PSD of
 * the low-band window (nSigSE before PSDMean, NoiseSup.c:1211-1235) and the count of second-stage frames.  So per output
 * frame everything but a three-band noise tracker is free of recursion (wb_hb_kernel), and the tracker is a few dozen
 * operations per frame (wb_specsub_kernel).
 */
#include "ns_core.h"

namespace sea {

__global__ __launch_bounds__(kWbQmfThreads) void wb_qmf_kernel(WbQmfArgs a)
{
    constexpr int kHist = SEA_WB_QMF - 1;        /* 117 samples of history */
    constexpr int kWin = SEA_WB_HOP + kHist;     /* 277 */
    __shared__ float x[kWin + 3];
    __shared__ float tap[SEA_WB_QMF + 2]; /* (the taps as scalar operands from the table, one 8-byte LDS read per two products: 1.67 ms against 1.26) */
    const int u = blockIdx.x;
    const long long off = a.offsets[u];
    const long long nfr = a.lengths[u] / SEA_WB_HOP;
    const int16_t *in = a.in + off;
    float *lp = a.lp + off / 2, *hp = a.hp + off / 2;
    for (int j = threadIdx.x; j < SEA_WB_QMF; j += kWbQmfThreads) tap[j] = a.tables->qmfLp[j];
    for (long long f = blockIdx.y; f < nfr; f += gridDim.y) {
        const long long base = f * SEA_WB_HOP - kHist;
        int nonzero = 0;
        for (int i = threadIdx.x; i < kWin; i += kWbQmfThreads) {
            const long long p = base + i; /* p < 160 (f + 1) <= lengths[u] */
            const int16_t s = p >= 0 ? in[p] : (int16_t)0;
            x[i] = (float)s;
            nonzero |= (i >= kHist && s != 0) ? 1 : 0;
        }
        if (__syncthreads_or(nonzero) && threadIdx.x == 0) atomicMin(a.onset + u, (int)f);
        if (threadIdx.x < SEA_HOP) {
            const int k = threadIdx.x;
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
            lp[f * SEA_HOP + k] = aux1;
            hp[f * SEA_HOP + k] = (k & 1) ? -aux2 : aux2;
        }
        __syncthreads();
    }
}

/* The high band of one output frame.  Tick t = 1 is the first non-zero frame; NoiseSup's second stage, and with it the high
 * band (NoiseSup.c:1307-1327), runs from tick 5 on: output k = 0, 1, .. belongs to tick k + 5, frame onset + 4 + k.  At that tick
 *   - the high-band buffer of 480 samples holds the frames of ticks t-5 .. t and is read from sample 80 (NS_ANALYSIS_WINDOW_16K,
 *     NoiseSup.c:1170-1171): the 200 samples from the start of the frame of tick t-4 = frame onset + k;
 *   - the code pairs it with the head of the three-deep queue BandsForCoding16k (:1225-1234), filled by the first stage two
 *     ticks earlier from the low-band window of tick t-2: 200 samples from sample 60 of the frame of tick t-5 = frame
 *     onset + k - 1 (zeros before the onset: the stage buffer starts as zeros).
 * Both windows go through the dual 256-point transform side by side (same Hanning window, same PSD: ns_front_dual).  Then
 * the three in-order sums of low-band bins 33-38 / 39-48 / 49-64 (GetBandsForCoding16k), the mel triangles 1..3 over the
 * high-band PSD (DoMelFB), the logs with their floors and the nine code values (CodeBands16k).  hp_rows receives the RAW
 * band energies: wb_specsub_kernel subtracts the noise in place. */
__global__ __launch_bounds__(64) void wb_hb_kernel(WbHbArgs a)
{
    __shared__ __attribute__((aligned(16))) float bufA[320], bufB[320], work[512], psdA[68], psdB[68], logs[8];
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const long long off2 = a.offsets[u] / 2;
    const long long nfr = a.lengths[u] / SEA_WB_HOP;
    const long long onset = (long long)a.onset[u] < nfr ? a.onset[u] : nfr;
    const long long nout = nfr - onset - 4;
    const long long row0 = (a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP + onset + 4;
    if (nout <= 0) return;
    Fft2Regs fft;
    load_fft2_regs<false>(fft, &a.ns->fft, lane, nullptr);
    float win8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) win8[k] = a.ns->win8[k][lane];
    const float *lp = a.lp + off2, *hp = a.hp + off2;
    const float floorSpec = a.wb->floorSpec;
    for (long long k = blockIdx.y; k < nout; k += gridDim.y) {
        for (int j = lane; j < 320; j += kLanes) { /* the transforms read buf[60 .. 259] */
            const int i = j - 60;
            const long long ia = (onset + k - 1) * SEA_HOP + j, ib = (onset + k) * SEA_HOP + i; /* < 80 (onset + k + 3) <= 80 (nfr - 2) */
            const bool in = i >= 0 && i < SEA_WIN;
            bufA[j] = (in && ia >= onset * SEA_HOP) ? lp[ia] : 0.0f;
            bufB[j] = in ? hp[ib] : 0.0f;
        }
        wave_sync();
        ns_front_dual<false>(bufA, true, psdA, bufB, true, psdB, work, fft, win8, lane);
        float v = 0.0f;
        if (lane < 3) { /* GetBandsForCoding16k, 16kHzProcessing.c:497-510 */
            const int b0 = lane == 0 ? 33 : (lane == 1 ? 39 : 49), b1 = lane == 0 ? 39 : (lane == 1 ? 49 : 65);
            for (int i = b0; i < b1; ++i) v += psdA[i];
        } else if (lane < 6) { /* DoMelFB, MelProc.c:82-104 */
            const int b = lane - 3, st = a.wb->hpMelStart[b], n = a.wb->hpMelLen[b];
            for (int i = 0; i < n; ++i) v += psdB[st + i] * a.wb->hpMelW[b][i];
            a.hp_rows[(row0 + k) * 3 + b] = v;
        }
        if (lane < 6) logs[lane] = (v > floorSpec) ? ns_logf(v) : -10.0f; /* NoiseSup.c:1230-1233, :1320-1323 */
        wave_sync();
        if (lane < 9) a.code_rows[(row0 + k) * 9 + lane] = logs[lane % 3] - logs[3 + lane / 3]; /* code[3 i + j] = lpBands[j] - fb16k[i] */
        wave_sync();
    }
}

/* DoSpecSub16k (16kHzProcessing.c:388-477) over the outputs of one utterance in order, one lane per utterance: a small VAD
 * on the log of the three bands' sum, a noise estimate per band, subtraction with a floor.  The promotions are the
 * reference's: 1.0 - 1.0 / (float)nbFrame and (1 - 0.98) * .. are double expressions rounded into floats, (1 - lambdaNSE)
 * is float.  nbFrame is the count of second-stage frames (NoiseSup.c:376-379, :1326) = the output's number from 1. */
__global__ __launch_bounds__(64) void wb_specsub_kernel(WbHbArgs a)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.n_utt) return;
    const long long nfr = a.lengths[u] / SEA_WB_HOP;
    const long long onset = (long long)a.onset[u] < nfr ? a.onset[u] : nfr;
    const long long nout = nfr - onset - 4;
    float *row = a.hp_rows + ((a.offsets[u] + SEA_WB_HOP - 1) / SEA_WB_HOP + onset + 4) * 3;
    const float eps = a.wb->floorSpec, logMin = a.wb->logMin16k;
    float noise[3] = {0.0f, 0.0f, 0.0f}, meanEn = 0.0f;
    int nbSpeech = 0, hangOver = 0;
    for (long long k = 0; k < nout; ++k, row += 3) {
        const int nbFrame = k + 1 < 2147483647LL ? (int)(k + 1) : 2147483647;
        const float lambdaNSE = nbFrame < 100 ? (float)(1.0 - 1.0 / (double)(float)nbFrame) : (float)0.99;
        float in[3] = {row[0], row[1], row[2]};
        float frameEn = 0.0f;
        for (int i = 0; i < 3; ++i) frameEn += in[i];
        frameEn = ((double)frameEn > 0.001) ? ns_logf(frameEn) : logMin;
        if (((double)(frameEn - meanEn) < 1.2) || nbFrame < 10) {
            if (nbFrame < 10) meanEn += (1 - lambdaNSE) * (frameEn - meanEn);
            else if (frameEn < meanEn) meanEn = (float)((double)meanEn + (1 - 0.98) * (double)(frameEn - meanEn));
            else meanEn = (float)((double)meanEn + (1 - 0.995) * (double)(frameEn - meanEn));
        }
        int flagVAD;
        if ((double)(frameEn - meanEn) > 2.2) {
            flagVAD = 1;
            nbSpeech++;
        } else {
            if (nbSpeech > 4) hangOver = 15;
            nbSpeech = 0;
            if (hangOver != 0) {
                hangOver--;
                flagVAD = 1;
            } else
                flagVAD = 0;
        }
        if (flagVAD == 0) {
            for (int i = 0; i < 3; ++i) {
                if (nbFrame < 10 || in[i] < noise[i]) noise[i] = lambdaNSE * noise[i] + (1 - lambdaNSE) * in[i];
                else noise[i] = (float)(0.995 * (double)noise[i] + (1 - 0.995) * (double)in[i]);
                if (noise[i] < eps) noise[i] = eps;
            }
        }
        for (int i = 0; i < 3; ++i) {
            const float floor = (float)(0.1 * (double)in[i]);
            const float diff = (float)((double)in[i] - 1.5 * (double)noise[i]);
            row[i] = diff > floor ? diff : floor;
        }
    }
}

} // namespace sea
