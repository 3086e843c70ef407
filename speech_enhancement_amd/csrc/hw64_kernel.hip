/*
 * hw64_kernel.hip -- the front half of the Hu-Wang mask estimator createIBM() at 16 kHz on its 64-channel gammatone bank, gfx950
 * (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:41-76 at the constants of resyth_64sub_IBM/cpp/HuWang.h).
 * A first form, not tuned.
 *
 *   hw64_periphery_kernel    AudiPeriph: gammaToneFilter:225-251 + hairCell:277-298, one lane per (utterance, channel),
 *                            float in, hOut in float; gOut (the filter's output before the hair cell) on request
 *   hw64_lowpass_kernel      lowPass:318-328: hEv, the 181-tap FIR of hOut, one lane per sample
 *   hw64_correlogram_kernel  computeACF:341-369, crossCorr:377-437, globalPitch:445-461, timeCrn:771-790 and the initial
 *                            labelling :74-76, one workgroup per frame.  Only hOut's 64 x 201 ACF values stay in LDS for the
 *                            frame; hEv's pass through a ring of three channels.
 *
 * Every sum keeps the reference's order and every product and sum is rounded on its own (-ffp-contract=off); divisions and
 * the square root are the compiler's correctly rounded ones.  Layout: utterance u's 64 streams form a [64][pitch] float block
 * at offsets[u] * 64, pitch = lengths[u] rounded up to 8; the frame outputs are rows, utterance u's first at row_offsets[u].
 * The recurrences are those of the 25-channel bank (hw25_device.h); only the tables differ.
 */
#include "hw25_device.h"
#include "sea_device.h"
#include "sea_kernels.h"

namespace sea {

namespace {

constexpr int kCh = SEA_HW64_NCHAN, kDel = SEA_HW64_DELAYS, kHop = SEA_HW64_HOP, kTaps = SEA_HW64_TAPS;
constexpr int kPerTile = 8;                           /* samples per step of the periphery loop */
constexpr int kWinStage = SEA_HW64_MAXWIN + kDel - 1; /* samples one (channel, frame) reads: the window and 200 before it */
constexpr int kAcfLanes = 2 * kDel;                   /* threads 0..401: (stream, delay) */
constexpr int kFollower = kHw64CorrThreads - 64;      /* the last wave's first thread */
static_assert(kAcfLanes <= kFollower, "the (stream, delay) lanes and the following wave do not overlap");

/* between LDS writes of one lane and later reads by another lane of the same wave */
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

/* v[0] + v[1] + .. + v[200] from zero, in that order; every lane of the wave reads the same words and gets the same sum */
__device__ __forceinline__ float sum_in_order(const float *v)
{
    float sum = 0.0f;
#pragma unroll 8
    for (int k = 0; k < kDel; ++k) sum += v[k];
    return sum;
}

/* crossCorr:386-418 for one channel by one wave, v[201] in LDS in place: the mean removed, divided by the RMS unless that is
 * zero.  The sums run in every lane alike; the per-delay work is dealt to the lanes.  prod[201]: the wave's scratch. */
__device__ __forceinline__ void normalise_channel(float *v, float *prod, int lane)
{
    const float mean = sum_in_order(v) / (float)kDel;
    wave_lds_fence();
    for (int k = lane; k < kDel; k += 64) {
        const float x = v[k] - mean;
        v[k] = x;
        prod[k] = x * x;
    }
    wave_lds_fence();
    const float rms = sqrtf(sum_in_order(prod) / (float)kDel);
    wave_lds_fence();
    if (rms != 0.0f)
        for (int k = lane; k < kDel; k += 64) v[k] /= rms;
    wave_lds_fence();
}

/* crossCorr:421-433 for two normalised neighbours by one wave */
__device__ __forceinline__ float cross_of(const float *v0, const float *v1, float *prod, int lane)
{
    for (int k = lane; k < kDel; k += 64) prod[k] = v0[k] * v1[k];
    wave_lds_fence();
    const float cross = sum_in_order(prod) / (float)kDel;
    wave_lds_fence();
    return cross;
}

} // namespace

/* One wave per utterance, lane = channel (all 64 lanes).  The input sample is the same word for every lane; the next eight
 * samples are requested before the current eight are worked on.  Full groups of eight outputs leave as two 16-byte stores
 * per lane; the last, partial group as single words, so the padding between length and pitch is not written. */
__global__ __launch_bounds__(64) void hw64_periphery_kernel(Hw64Args a)
{
    const int c = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u];
    if (c >= kCh || L <= 0) return;
    const long long pitch = (L + 7) & ~7LL;
    const sea_hw64_tables &t = *a.tables;
    const float f1 = t.f1[c], f2 = t.f2[c], gain = t.gain[c];
    const float *in = a.in + off;
    float *out = a.hout + off * kCh + c * pitch;
    float *gout = a.gout ? a.gout + off * kCh + c * pitch : nullptr; /* gOut, which computeAM and the resynthesis read (optional) */
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

/* grid (n_utt, 64) -- the utterances on x, the only grid dimension that takes more than 65535: workgroup = one stream, lane =
 * sample.  hEv[n] = sum over m = 0..180 in order of hOut[n + 90 - m] * filter[m], the terms outside [0, L) skipped. */
__global__ __launch_bounds__(256) void hw64_lowpass_kernel(Hw64Args a)
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
#pragma unroll 4
        for (int m = 0; m < kTaps; ++m) {
            const long long tim = n + (kTaps - 1) / 2 - m;
            if (tim >= 0 && tim < L) sum += src[tim] * lp[m];
        }
        dst[n] = sum;
    }
}

/* grid (n_utt, G) x 512: workgroup (u, g) takes the frames g, g + G, ... of utterance u.  Per frame the channels go by one
 * after the other.  For each, the window of both streams (winsize + 200 samples, at most 1480) is staged in LDS once; threads
 * 0..200 are the delays of hOut, 201..401 those of hEv, and the serial `step` loop runs inside the lane: stream[tim] is one
 * LDS word for all lanes of a stream (a broadcast), stream[tim - delay] consecutive words (no bank conflict).
 *
 * hOut's ACF stays in LDS for the whole frame (timeCrn needs acf[c][Pitch] once the pitch is known; 51 456 bytes); each
 * delay's lane adds its channels to sumCorr[delay] in a register as they finish, which is globalPitch's channel order.
 * hEv's ACF only feeds crossCorr, which reads channels c and c + 1: it lives in a ring of three channels.  While the lanes
 * work on channel c, the last wave of the workgroup normalises hEv's channel c - 1 and multiplies it with c - 2.
 * Static LDS: 67 616 bytes, two workgroups per CU. */
__global__ __launch_bounds__(kHw64CorrThreads) void hw64_correlogram_kernel(Hw64Args a)
{
    __shared__ float win[2][kWinStage + 1];
    __shared__ float acfH[kCh][kDel];
    __shared__ float acfE[3][kDel];
    __shared__ float prod[kDel];
    __shared__ float sumCorr[kDel];
    __shared__ float acf0[kCh];
    __shared__ int sPitch;
    const int tid = threadIdx.x;
    const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    const long long off = a.offsets[u], L = a.lengths[u], row0 = a.row_offsets[u];
    const long long pitch = (L + 7) & ~7LL;
    const long long nfr = L / kHop;
    const float *hout = a.hout + off * kCh, *hev = a.hev + off * kCh;
    const int s = tid >= kDel ? 1 : 0, d = tid - s * kDel; /* meaningful for tid < kAcfLanes */
    const int lane = tid - kFollower;                      /* meaningful in the following wave */
    for (long long frame = blockIdx.y; frame < nfr; frame += gridDim.y) {
        const long long row = row0 + frame;
        const long long T = (frame + 2) * kHop;
        float *cross_ev = a.cross_ev + row * kCh;
        float total = 0.0f; /* sumCorr[d] of globalPitch, in the lanes of hOut */
        /* ---- computeACF, and crossCorr for hEv one channel behind ---- */
        for (int c = 0; c < kCh; ++c) {
            const int ws = a.tables->winsize[c];
            const long long base = T - ws - (kDel - 1); /* win[.][j] holds sample base + j, j < ws + 200 */
            __syncthreads();
            for (int j = tid; j < ws + kDel - 1; j += kHw64CorrThreads) {
                const long long tim = base + j;
                const bool in = tim >= 0 && tim < L;
                win[0][j] = in ? hout[c * pitch + tim] : 0.0f;
                win[1][j] = in ? hev[c * pitch + tim] : 0.0f;
            }
            __syncthreads();
            if (tid < kAcfLanes) {
                const float *w = win[s];
                float sum = 0.0f;
                /* step = 0..ws-1, tim = T - (step + 1); tim < L  <=>  step >= T - L */
                const int first = T > L ? (int)(T - L) : 0;
                if (base >= 0) { /* tim - delay >= 0 throughout */
#pragma unroll 8
                    for (int step = first; step < ws; ++step) {
                        const int j = ws + (kDel - 2) - step;
                        sum += w[j] * w[j - d];
                    }
                } else {
#pragma unroll 4
                    for (int step = first; step < ws; ++step) {
                        const long long tim = T - 1 - step;
                        const int j = ws + (kDel - 2) - step;
                        if (tim - d >= 0) sum += w[j] * w[j - d];
                    }
                }
                const float v = sum / (float)ws;
                float *out = s ? a.acf_ev : a.acf_hc;
                if (out) out[(row * kCh + c) * kDel + d] = v;
                if (s) {
                    acfE[c % 3][d] = v;
                } else {
                    acfH[c][d] = v;
                    total += v;
                    if (d == 0) acf0[c] = v;
                }
            } else if (tid >= kFollower) {
                if (c >= 1) normalise_channel(acfE[(c - 1) % 3], prod, lane);
                if (c >= 2) {
                    const float cross = cross_of(acfE[(c - 2) % 3], acfE[(c - 1) % 3], prod, lane);
                    if (lane == 0) cross_ev[c - 2] = cross;
                }
            }
        }
        __syncthreads();
        if (tid < kDel) sumCorr[tid] = total;
        if (tid >= kFollower) { /* hEv's last channel */
            normalise_channel(acfE[(kCh - 1) % 3], prod, lane);
            const float cross = cross_of(acfE[(kCh - 2) % 3], acfE[(kCh - 1) % 3], prod, lane);
            if (lane == 0) {
                cross_ev[kCh - 2] = cross;
                cross_ev[kCh - 1] = 0.0f;
            }
        }
        __syncthreads();
        /* ---- globalPitch: the first strict maximum over 32..200 ---- */
        if (tid == 0) {
            int p = SEA_HW64_MINDELAY;
            float mp = sumCorr[p];
#pragma unroll 4
            for (int k = SEA_HW64_MINDELAY + 1; k < kDel; ++k)
                if (sumCorr[k] > mp) {
                    mp = sumCorr[k];
                    p = k;
                }
            sPitch = p;
            a.pitch[row] = p;
        }
        __syncthreads();
        /* ---- timeCrn (corrHc): Pitch is >= 32, so its `Pitch > 0` branch is always taken.  Lane = channel from here on:
         * acfH[lane][k] is word 201 lane + k, and 201 = 9 mod 64 is odd, so the 64 lanes read 64 banks. ---- */
        if (tid < kCh) {
            const float at = acfH[tid][sPitch];
            float mp = at;
#pragma unroll 4
            for (int k = SEA_HW64_MINDELAY; k < kDel; ++k)
                if (acfH[tid][k] > mp) mp = acfH[tid][k];
            a.pratio[row * kCh + tid] = at / mp;
        }
        __syncthreads();
        /* ---- crossCorr for hOut: remove the mean, divide by the RMS unless it is zero (in place), neighbour products ---- */
        if (tid < kCh) {
            float *v = acfH[tid];
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
        if (tid < kCh) {
            float cross = 0.0f;
            if (tid < kCh - 1) {
                const float *v0 = acfH[tid], *v1 = acfH[tid + 1];
#pragma unroll 4
                for (int k = 0; k < kDel; ++k) cross += v0[k] * v1[k];
                cross /= (float)kDel;
            }
            a.cross_hc[row * kCh + tid] = cross;
            /* :76: cross against the double 0.985, acf[chan][0] against (float)(50 * 50) */
            a.mark[row * kCh + tid] = ((double)cross > 0.985 && acf0[tid] > 2500.0f) ? 1.0f : 0.0f;
        }
    }
}

} // namespace sea
