/*
 * afe_vad.h -- what DoPostProc (PostProc.c:123-149), DoVADProc (VAD.c:219-317) and DoVADFlush (:342-433) carry and decide, for one
 * utterance per wave, lane = feature index (0..13 cepstra / energies, 14 the VAD flag): the recursion's registers, PostProc's
 * target table and step size, and the VAD's decision.  Used by afe_vad_body<WB> (cc_kernel.hip: a whole utterance) and by
 * afe_vad_slice_body<WB> (afe_slice_kernel.hip: the frames that complete in a time slice, the registers carried in the state).
 *
 * The row loop with its eight-ahead queue and the flush loop are NOT here: each of the two bodies writes them out around a
 * `decide` lambda.  Behind a call they compile to other code in both units -- in cc_kernel.hip, whose kernels are to stay as
 * measured, 2177 -> 2142 / 2205 instructions for afe_vad_kernel; in the slice form the scheduler no longer issued decide's
 * seven LDS reads together (103 instead of 25 full LDS waits) and afe_vad_slice_kernel measured 12 % slower.
 * tests/test_gpu_afe_slices.py and tests/test_gpu_wb_afe_slices.py hold the two loops together bit for bit.
 * Internal to the library.
 */
#pragma once
#include "ns_core.h"

namespace sea {

namespace {

/* the recursion's registers, with the values an utterance starts from.  The members' order is part of what keeps
 * afe_vad_kernel / afe_wb_vad_kernel (cc_kernel.hip) instruction for instruction as measured: another order moves the order of
 * the loop's register initialisations. */
struct AfeVad {
    float wLMS = 0.0f; /* weightLMS[lane] */
    float feat = 0.0f; /* FeatureBuffer[lane]: persists between calls like the reference's buffer */
    int frameCounter = 0, vCount = 0, hCount = 0, hangOver = 23, focus = 0;
};

/* PostProc's LMS step: target[lane] for the twelve cepstra it whitens (0 for the other lanes) and the step size */
__device__ __forceinline__ float afe_postproc_target(int lane)
{
    static const float target[12] = {(float)-6.618909, (float)0.198269, (float)-0.740308, (float)0.055132,
                                     (float)-0.227086, (float)0.144280, (float)-0.112451, (float)-0.146940,
                                     (float)-0.327466, (float)0.134571, (float)0.027884,  (float)-0.114905};
    return (lane < 12) ? target[lane] : 0.0f;
}
constexpr float kPostProcLambda = (float)0.0087890625;

/* trigger = longest run of speech-flagged frames in the ring, scanned from focus+1 round to focus */
__device__ __forceinline__ void afe_vad_decide(AfeVad &v, float (&ring)[7][16], int fc, int lane)
{
    int sum = 0, trigger = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        int r = v.focus + i + 1;
        r = r > 6 ? r - 7 : r;
        if (ring[r][14] != 0.0f)
            sum++;
        else {
            trigger = sum > trigger ? sum : trigger;
            sum = 0;
        }
    }
    trigger = sum > trigger ? sum : trigger;
    if (trigger >= 4) {
        v.hCount = v.hangOver;
        if (fc <= 35) v.hangOver = 50;
    }
    if (v.hCount && trigger < 3) v.hCount--;
    if (trigger >= 3) v.vCount = 5;
    if (v.vCount && trigger < 3) v.vCount--;
    int r = v.focus + 1;
    r = r > 6 ? r - 7 : r;
    v.feat = (lane < 15) ? ring[r][lane] : 0.0f;
    if (lane == 14) v.feat = (v.vCount || v.hCount || trigger >= 3) ? 1.0f : 0.0f;
}

} // namespace

} // namespace sea
