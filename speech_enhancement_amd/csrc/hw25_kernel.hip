/*
 * hw25_kernel.hip -- the front half of the Hu-Wang mask estimator createIBM() on its 25-channel 8 kHz gammatone bank, gfx950
 * (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:41-76; constants HuWang.h).  A first form, not tuned.
 *
 *   hw25_periphery_kernel    AudiPeriph: gammaToneFilter:225-251 + hairCell:277-298, one lane per (utterance, channel),
 *                            float in, hOut in float; gOut (the filter's output before the hair cell) on request
 *   hw25_lowpass_kernel      lowPass:318-328: hEv, the 91-tap FIR of hOut, one lane per sample
 *   hw25_correlogram_kernel  computeACF:341-369, crossCorr:377-437, globalPitch:445-461, timeCrn:771-790 and the initial
 *                            labelling :74-76, one workgroup per frame with the frame's 2 x 25 x 101 ACF values held in LDS
 *
 * Every sum keeps the reference's order and every product and sum is rounded on its own (-ffp-contract=off); divisions and
 * the square root are the compiler's correctly rounded ones.  Layout: utterance u's 25 streams form a [25][pitch] float block
 * at offsets[u] * 25, pitch = lengths[u] rounded up to 8; the frame outputs are rows, utterance u's first at row_offsets[u].
 */
#include "hw25_device.h"
#include "sea_device.h"
#include "sea_kernels.h"

namespace sea {

namespace {

constexpr int kCh = SEA_HW25_NCHAN, kDel = SEA_HW25_DELAYS, kHop = SEA_HW25_HOP, kTaps = SEA_HW25_TAPS;
constexpr int kPerTile = 8;                          /* samples per step of the periphery loop */
constexpr int kWinStage = SEA_HW25_MAXWIN + kDel - 1; /* samples one (channel, frame) reads: the window and 100 before it */

} // namespace

/* One wave per utterance, lane = channel (25 of 64 lanes).  The input sample is the same word for every lane; the next
 * eight samples are requested before the current eight are worked on.  Full groups of eight outputs leave as two 16-byte
 * stores per lane; the last, partial group as single words, so the padding between length and pitch is not written. */
__global__ __launch_bounds__(64) void hw25_periphery_kernel(Hw25Args a)
{
    const int c = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u];
    if (c >= kCh || L <= 0) return;
    const long long pitch = (L + 7) & ~7LL;
    const sea_hw25_tables &t = *a.tables;
    const float f1 = t.f1[c], f2 = t.f2[c], gain = t.gain[c];
    const float *in = a.in + off;
    float *out = a.hout + off * kCh + c * pitch;
    float *gout = a.gout ? a.gout + off * kCh + c * pitch : nullptr; /* gOut, the gammatone output computeAM reads (optional) */
    Gt25 g = {};
    Hair25 h = {t.q0, t.c0, t.w0};
    /* in[] holds `pitch` floats: the reads of the last group stay inside the utterance's padded stretch */
    float4 n0 = *reinterpret_cast<const float4 *>(in), n1 = *reinterpret_cast<const float4 *>(in + 4);
    for (long long n = 0; n < L; n += kPerTile) {
        const float x[kPerTile] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
        if (n + kPerTile < L) {
            n0 = *reinterpret_cast<const float4 *>(in + n + kPerTile);
            n1 = *reinterpret_cast<const float4 *>(in + n + kPerTile + 4);
        }
        float o[kPerTile], go[kPerTile];
#pragma unroll
        for (int k = 0; k < kPerTile; ++k) {
            go[k] = gt25_step(g, x[k], f1, f2, gain);
            o[k] = hair25_step(h, go[k], t);
        }
        if (n + kPerTile <= L) {
            *reinterpret_cast<float4 *>(out + n) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4 *>(out + n + 4) = make_float4(o[4], o[5], o[6], o[7]);
            if (gout) {
                *reinterpret_cast<float4 *>(gout + n) = make_float4(go[0], go[1], go[2], go[3]);
                *reinterpret_cast<float4 *>(gout + n + 4) = make_float4(go[4], go[5], go[6], go[7]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPerTile; ++k)
                if (n + k < L) {
                    out[n + k] = o[k];
                    if (gout) gout[n + k] = go[k];
                }
        }
    }
}

/* grid (n_utt, 25) -- the utterances on x, the only grid dimension that takes more than 65535: workgroup = one stream, lane = sample.  hEv[n] = sum over m = 0..90 in order of hOut[n + 45 - m] *
 * filter[m], the terms outside [0, L) skipped. */
__global__ __launch_bounds__(256) void hw25_lowpass_kernel(Hw25Args a)
{
    __shared__ float lp[kTaps];
    const int c = blockIdx.y;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u];
    const long long pitch = (L + 7) & ~7LL;
    for (int i = threadIdx.x; i < kTaps; i += 256) lp[i] = a.tables->lp[i];
    __syncthreads();
    const float *src = a.hout + off * kCh + c * pitch;
    float *dst = a.hev + off * kCh + c * pitch;
    for (long long n = threadIdx.x; n < L; n += 256) {
        float sum = 0.0f;
#pragma unroll 7
        for (int m = 0; m < kTaps; ++m) {
            const long long tim = n + (kTaps - 1) / 2 - m;
            if (tim >= 0 && tim < L) sum += src[tim] * lp[m];
        }
        dst[n] = sum;
    }
}

/* grid (n_utt, G): workgroup (u, g) takes the frames g, g + G, ... of utterance u.  Per frame and channel the window of both
 * streams (winsize + 100 samples each, at most 500) is staged in LDS once; lanes 0..100 of the first half of the workgroup
 * are the delays of hOut, those of the second half the delays of hEv, and the serial `step` loop runs inside the lane:
 * stream[tim] is one LDS word for all lanes (a broadcast), stream[tim - delay] consecutive words (no bank conflict).  The
 * 2 x 25 x 101 results stay in LDS for crossCorr, globalPitch, timeCrn and the labelling. */
__global__ __launch_bounds__(256) void hw25_correlogram_kernel(Hw25Args a)
{
    __shared__ float win[2][kWinStage + 1];
    __shared__ float acf[2][kCh][kDel];
    __shared__ float sumCorr[kDel];
    __shared__ float acf0[kCh];
    __shared__ int sPitch;
    const int tid = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u], row0 = a.row_offsets[u];
    const long long pitch = (L + 7) & ~7LL;
    const long long nfr = L / kHop;
    const float *hout = a.hout + off * kCh, *hev = a.hev + off * kCh;
    const int s = tid >> 7, d = tid & 127;
    for (long long frame = blockIdx.y; frame < nfr; frame += gridDim.y) {
        const long long row = row0 + frame;
        const long long T = (frame + 2) * kHop;
        /* ---- computeACF ---- */
        for (int c = 0; c < kCh; ++c) {
            const int ws = a.tables->winsize[c];
            const long long base = T - ws - (kDel - 1); /* win[.][j] holds sample base + j, j < ws + 100 */
            __syncthreads();
            for (int j = tid; j < ws + kDel - 1; j += 256) {
                const long long tim = base + j;
                const bool in = tim >= 0 && tim < L;
                win[0][j] = in ? hout[c * pitch + tim] : 0.0f;
                win[1][j] = in ? hev[c * pitch + tim] : 0.0f;
            }
            __syncthreads();
            if (d < kDel) {
                const float *w = win[s];
                float sum = 0.0f;
                /* step = 0..ws-1, tim = T - (step + 1); tim < L  <=>  step >= T - L */
                const int first = T > L ? (int)(T - L) : 0;
#pragma unroll 4
                for (int step = first; step < ws; ++step) {
                    const long long tim = T - 1 - step;
                    const int j = ws + (kDel - 2) - step;
                    if (tim - d >= 0) sum += w[j] * w[j - d];
                }
                acf[s][c][d] = sum / (float)ws;
            }
        }
        __syncthreads();
        if (a.acf_hc)
            for (int i = tid; i < kCh * kDel; i += 256) a.acf_hc[row * (kCh * kDel) + i] = (&acf[0][0][0])[i];
        if (a.acf_ev)
            for (int i = tid; i < kCh * kDel; i += 256) a.acf_ev[row * (kCh * kDel) + i] = (&acf[1][0][0])[i];
        /* ---- globalPitch: per delay the 25 channels in order; the first strict maximum over 16..100 ---- */
        if (tid < kDel) {
            float sum = 0.0f;
#pragma unroll 5
            for (int c = 0; c < kCh; ++c) sum += acf[0][c][tid];
            sumCorr[tid] = sum;
        }
        if (tid >= 128 && tid < 128 + kCh) acf0[tid - 128] = acf[0][tid - 128][0];
        __syncthreads();
        if (tid == 0) {
            int p = SEA_HW25_MINDELAY;
            float mp = sumCorr[p];
#pragma unroll 4
            for (int k = SEA_HW25_MINDELAY + 1; k < kDel; ++k)
                if (sumCorr[k] > mp) {
                    mp = sumCorr[k];
                    p = k;
                }
            sPitch = p;
            a.pitch[row] = p;
        }
        __syncthreads();
        /* ---- timeCrn (corrHc): Pitch is >= 16, so its `Pitch > 0` branch is always taken ---- */
        if (tid < kCh) {
            const float at = acf[0][tid][sPitch];
            float mp = at;
#pragma unroll 4
            for (int k = SEA_HW25_MINDELAY; k < kDel; ++k)
                if (acf[0][tid][k] > mp) mp = acf[0][tid][k];
            a.pratio[row * kCh + tid] = at / mp;
        }
        __syncthreads();
        /* ---- crossCorr: remove the mean, divide by the RMS unless it is zero (in place), neighbour products ---- */
        if (tid < 2 * kCh) {
            float *v = acf[tid / kCh][tid % kCh];
            float sum = 0.0f;
#pragma unroll 4
            for (int k = 0; k < kDel; ++k) sum += v[k];
            sum /= (float)kDel;
            float sq = 0.0f;
#pragma unroll 4
            for (int k = 0; k < kDel; ++k) {
                const float x = v[k] - sum;
                v[k] = x;
                sq += x * x;
            }
            const float rms = sqrtf(sq / (float)kDel);
            if (rms != 0.0f)
#pragma unroll 2
                for (int k = 0; k < kDel; ++k) v[k] /= rms;
        }
        __syncthreads();
        if (tid < 2 * kCh) {
            const int st = tid / kCh, c = tid % kCh;
            float cross = 0.0f;
            if (c < kCh - 1) {
                const float *v0 = acf[st][c], *v1 = acf[st][c + 1];
#pragma unroll 4
                for (int k = 0; k < kDel; ++k) cross += v0[k] * v1[k];
                cross /= (float)kDel;
            }
            (st ? a.cross_ev : a.cross_hc)[row * kCh + c] = cross;
            /* :76: cross against the double 0.985, acf[chan][0] against (float)(50 * 50) */
            if (st == 0) a.mark[row * kCh + c] = ((double)cross > 0.985 && acf0[c] > 2500.0f) ? 1.0f : 0.0f;
        }
    }
}

} // namespace sea
