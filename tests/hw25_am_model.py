"""tests/hw25_am_model.py -- TEST INFRASTRUCTURE ONLY: a numpy restatement of the Hu-Wang estimator's AM labels and final
grouping (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp: computeAM:1146-1317 with amPatt, hilbert,
computeAMRate and sinModel, the tools kaiserPara / kaiserBandPass / bessi0 / fft:1553-1677, finalSeg:1321-1494 with
reSegmentation and develope, and the binarisation :99-106), written from the formulas of that file: float32 where the
reference's expression is float, float64 where it is double, every sum in the reference's order.  The FFT is vectorised per
stage (the butterflies of one stage are independent), the FIR and the 200-sample sums run term by term over whole arrays.

sinModel's cosf / sinf / atanf are the one place where the model is NOT the reference: the C library's float functions are
not correctly rounded, so the model (and the engine) take the double function and round it to float.  Everything before it is
bit for bit the reference's; ratio agrees to the fixture's ratio_tol.

tests/test_hw25_am_cpu.py pins the model against tests/golden/hw25_am_golden.npz (tools/gen_hw25_am_golden.py);
tests/test_gpu_hw25_am.py uses it where the fixture holds nothing.  Definitions where the reference has none, as
include/sea_mi355x.h: more than 150000 samples -> AM_TOO_LONG and zeros; more than 400 segments in a reSegmentation ->
FINAL_TOO_MANY_SEGMENTS and zeros; fewer than 3 rows -> zeros.
"""
import math
import os
import zlib

import numpy as np

from tests import hw25_pitch_model as PM

NCH, HOP, WINDOW, FS = 25, 80, 200, 8000
PI = 3.1415926535897932384626433832795
THETAC, THETAT, THETAE = 0.985, 0.85, 0.20
MIN_SEG_LENGTH, MAX_SEG, MAX_LEN = 5, 400, 150000
FINAL_TOO_MANY_SEGMENTS, AM_TOO_LONG, AM_BAD_PITCH = 1 << 18, 1 << 19, 1 << 20
FINAL_STAGES = ("final_reseg1", "final_reseg2", "final_reseg3", "final_dev_minus", "final_dev_plus")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw25_am_golden.npz")
F32 = np.float32
AUDIO_CASES = ("p", "q", "r", "t", "m9", "w2048", "w1600", "p12000")
SAMPLES = 256  # sampled values per array kept in the fixture beside the CRCs


# ---- the inputs of the fixture ------------------------------------------------------------------------------------------------
def audio_inputs():
    """tests/hw25_pitch_model.audio_inputs() cut to 4000 samples around a voiced stretch, one input of exactly 2048 samples (a
    power of two: 25 frames and 48 samples over), one of 1600, and p whole: 12000 samples, N = 14, the one input whose FFT
    is longer than the 4096 points that the engine keeps in LDS"""
    xs = PM.audio_inputs()
    out = {"p": xs["p"][1200:5200], "q": xs["q"][3000:7000], "r": xs["r"][3000:7000], "t": xs["t"][1000:5000],
           "m9": xs["m9"][1000:5000], "w2048": xs["p"][2000:4048], "w1600": xs["t"][2000:3600], "p12000": xs["p"]}
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def _blank(nfr):
    return dict(grp=np.zeros((nfr, NCH), np.float32), amcrn=np.zeros((nfr, NCH), np.float32),
                cross_ev=np.zeros((nfr, NCH), np.float32), pratio=np.zeros((nfr, NCH), np.float32))


def hand_prune():
    """each of the three reSegmentations drops a component of 4 frames and keeps one of exactly 5"""
    c = _blank(16)
    # first: Grp == 0, AmCrn, cross_ev > THETAC
    for f0, f1, ch in ((1, 5, 2), (8, 11, 2)):
        c["amcrn"][f0:f1 + 1, ch] = 1
        c["cross_ev"][f0:f1 + 1, ch] = 0.99
    c["amcrn"][1:6, 4], c["cross_ev"][1:6, 4] = 1, 0.98  # a label without the cross-channel correlation: no unit
    # second: Grp == 1, pRatio > THETAT
    for f0, f1, ch in ((2, 6, 8), (9, 12, 8)):
        c["grp"][f0:f1 + 1, ch] = 1
        c["pratio"][f0:f1 + 1, ch] = 0.9
    # third: Grp == 1, pRatio <= THETAT
    for f0, f1, ch in ((3, 7, 14), (10, 13, 14)):
        c["grp"][f0:f1 + 1, ch] = 1
        c["pratio"][f0:f1 + 1, ch] = 0.5
    c["grp"][2:9, 20] = -1
    return c


def hand_sweeps():
    """develope (m, 1) has to grow along a snake that runs down the channels, back in time, up the channels and forward in
    time again: the reference's in-place sweep needs several passes, and so does any sweep in the other direction"""
    c = _blank(20)

    def snake(lo, hi):
        """columns at frames 17, 14, .., 2 over the channels lo..hi, joined alternately at channel hi and at channel lo"""
        path = []
        for turn, f in enumerate(range(17, 1, -3)):
            path += [(f, ch) for ch in (range(lo, hi + 1) if turn % 2 == 0 else range(hi, lo - 1, -1))]
            if f - 3 >= 2:
                end = hi if turn % 2 == 0 else lo
                path += [(f - 1, end), (f - 2, end)]
        return path

    # develope (m, 1): a snake of labelled units with Grp == 0 and no cross-channel correlation (not units of the first
    # reSegmentation), its head next to a + segment of five frames
    for f, ch in snake(1, 11):
        c["amcrn"][f, ch], c["cross_ev"][f, ch] = 1, 0.5
    c["grp"][15:20, 0], c["pratio"][15:20, 0] = 1, 0.9
    # develope (m, -1): a snake of + units whose pRatio alternates above / below THETAT from unit to unit, so that each is a
    # component of its own in the second or the third reSegmentation, has no seed and turns -2; its head next to a segment
    # of five frames below THETAT, which the third reSegmentation keeps as -1
    for i, (f, ch) in enumerate(snake(13, 24)):
        c["grp"][f, ch], c["pratio"][f, ch] = 1, (0.9 if i % 2 == 0 else 0.5)
    c["grp"][15:20, 12], c["pratio"][15:20, 12] = 1, 0.5
    return c


def hand_minus2():
    """units that become -2 (pruned from the + and from the - side) and then turn to 1, away from any -1 unit"""
    c = _blank(12)
    c["grp"][1:4, 5], c["pratio"][1:4, 5] = 1, 0.95    # 3 frames, pRatio above: pruned -> -2 -> 1
    c["grp"][2:6, 9], c["pratio"][2:6, 9] = 1, 0.2     # 4 frames, pRatio below: pruned -> -2 -> 1
    c["grp"][4:10, 15], c["pratio"][4:10, 15] = 1, 0.95  # 6 frames: kept, stays 1
    c["grp"][3:9, 20], c["pratio"][3:9, 20] = 1, 0.3   # 6 frames, below: kept as -1
    c["grp"][5, 21], c["pratio"][5, 21] = 1, 0.95      # a single unit beside the -1 segment: -2, then develope makes it -1
    c["grp"][1:11, 12] = -1
    return c


def hand_empty():
    """no unit at all"""
    return _blank(14)


HAND_CASES = {"prune": hand_prune, "sweeps": hand_sweeps, "minus2": hand_minus2, "empty": hand_empty}


def edge_frame0():
    """Edge set: finalSeg's develope with a unit of the growing value at frame 0 (HuWang.cpp:1456, the outcome `no earlier
    frame`), and at the last frame.  A + segment of six frames from frame 0 in channel 5 with a labelled unit beside it at
    frame 0, which develope (m, 1) adds; a segment below THETAT that ends at the last frame in the top channel, with a single
    + unit beside it at the last frame, which develope (m, -1) turns to -1."""
    c = _blank(12)
    c["grp"][0:6, 5], c["pratio"][0:6, 5] = 1, 0.9
    c["amcrn"][0, 6], c["cross_ev"][0, 6] = 1, 0.5
    c["grp"][6:12, NCH - 1], c["pratio"][6:12, NCH - 1] = 1, 0.5
    c["grp"][11, NCH - 2], c["pratio"][11, NCH - 2] = 1, 0.9
    return c


EDGE_HAND_CASES = {"eframe0": edge_frame0}


def many_final_segments_case():
    """more than 400 segments in the first reSegmentation: 442 isolated columns of three frames (model only)"""
    nfr = 34 * 4 + 1
    c = _blank(nfr)
    for b in range(34):
        c["amcrn"][1 + 4 * b:4 + 4 * b, 0::2] = 1
        c["cross_ev"][1 + 4 * b:4 + 4 * b, 0::2] = 0.99
    return c


# ---- constants -----------------------------------------------------------------------------------------------------------------
def kaiser_constants():
    """kaiserPara (0.01, ..):1557-1561 -> (a, beta), float"""
    a = F32(F32(-20) * F32(math.log10(float(F32(0.01)))))
    assert 21 < a <= 50
    beta = F32(0.5842 * float(F32(math.pow(float(F32(a - F32(21))), float(F32(0.4))))) + 0.07889 * float(F32(a - F32(21))))
    assert beta < 3.75
    return a, beta


def fft_log2(L):
    """computeAM:1156, in double with the C library's log"""
    return int(math.ceil(math.log(L * 1.0) / math.log(2 * 1.0)))


def n_at_pow2():
    return np.array([fft_log2(1 << k) for k in range(7, 18)], np.int32)


def twiddles(period, direct=1):
    """fft:1654-1674 for one stage: u of j = 0 .. period - 1, (re, im) float32 [period][2]"""
    w_r = F32(math.cos(PI / period))
    w_i = F32(-1.0 * math.sin(PI / period * float(F32(direct))))
    out = np.zeros((period, 2), np.float32)
    u_r, u_i = F32(1), F32(0)
    for j in range(period):
        out[j] = (u_r, u_i)
        u_r, u_i = F32(F32(u_r * w_r) - F32(u_i * w_i)), F32(F32(u_r * w_i) + F32(u_i * w_r))
    return out


_TW = {}


def _tw(period, direct):
    key = (period, direct)
    if key not in _TW:
        _TW[key] = twiddles(period, direct)
    return _TW[key]


# ---- gOut ----------------------------------------------------------------------------------------------------------------------
def gout(x, t):
    """gammaToneFilter:225-251 on the bank of tests/hw25_model.tables() -> gOut float32 [25][L]"""
    x = np.asarray(x, dtype=np.float32)
    f1, f2, gain = t["f1"], t["f2"], t["gain"]
    p = [np.zeros(NCH, np.float32) for _ in range(4)]
    q = [np.zeros(NCH, np.float32) for _ in range(4)]
    out = np.zeros((NCH, len(x)), np.float32)
    for n in range(len(x)):
        out[:, n] = p[3] * gain
        xs = [f1 * p[i] - f2 * q[i] for i in range(4)]
        ys = [f2 * p[i] + f1 * q[i] for i in range(4)]
        p[0] = x[n] * f1 + xs[0]
        q[0] = x[n] * f2 + ys[0]
        p[1] = p[0] + xs[1]
        q[1] = q[0] + ys[1]
        p[2] = p[1] + xs[1] + xs[2]
        q[2] = q[1] + ys[1] + ys[2]
        p[3] = p[2] + xs[1] + F32(2) * xs[2] + xs[3]
        q[3] = q[2] + ys[1] + F32(2) * ys[2] + ys[3]
    return out


# ---- amPatt --------------------------------------------------------------------------------------------------------------------
def _bessi0(x):
    """bessi0:1603-1614, the polynomial branch, on a float32 array"""
    x = np.asarray(x, np.float32)
    assert (np.abs(x) < 3.75).all()
    y = (x.astype(np.float64) / 3.75).astype(np.float32)
    y = (y * y).astype(np.float64)
    return (1.0 + y * (3.5156229 + y * (3.0899424 + y * (1.2067492 + y * (0.2659732 + y * (0.360768e-1 + y * 0.45813e-2)))))).astype(np.float32)


def kaiser_bandpass(mp):
    """kaiserPara (0.01, 0.4 / mp) and kaiserBandPass (.., 2.1 / mp, 0.7 / mp) -> the fLength + 1 taps, float32"""
    a, beta = kaiser_constants()
    mp = F32(mp)
    trans_bw = F32(0.4 / float(mp))
    length = F32((float(a) - 7.95) / 14.36 / float(trans_bw))
    flen = int(length)
    flen += 1 if float(F32(length - F32(flen))) < 0.5 else 2
    flen += flen % 2
    wc, wn = F32(2.1 / float(mp)), F32(0.7 / float(mp))
    tim = np.arange(flen + 1)
    k = (2 * tim).astype(np.float32) / F32(flen) - F32(1)
    f = _bessi0(beta * np.sqrt(F32(1) - k * k)) / _bessi0(beta)
    step = tim - flen // 2
    safe = np.where(step == 0, 1, step).astype(np.float64)
    side = (f.astype(np.float64) * (np.sin(float(wn) * PI * step) / PI / safe)).astype(np.float32)
    f = np.where(step == 0, f * wn, side).astype(np.float32)
    arg = (step.astype(np.float32) * wc).astype(np.float64) * PI
    return (f.astype(np.float64) * (2 * np.cos(arg))).astype(np.float32)


def block_mean_pitch(pitch, frame):
    """amPatt:1199-1211 -> the float mean of the positive pitches of frames frame - 2 .. frame + 2, or None"""
    mp, count = F32(0), 0
    for f in range(frame - 2, frame + 3):
        if 0 <= f < len(pitch) and pitch[f] > 0:
            mp = F32(mp + F32(pitch[f]))
            count += 1
    return F32(mp / F32(count)) if count else None


def am_patt(g, pitch):
    """amPatt:1189-1234 on max (gOut, 0), all channels at once -> float32 [25][L]"""
    L = g.shape[1]
    inp = np.where(g > 0, g, F32(0)).astype(np.float32)
    out = np.zeros_like(inp)
    nfr = L // HOP
    for frame in range(2, nfr, 5):
        mp = block_mean_pitch(pitch, frame)
        if mp is None:
            continue
        taps = kaiser_bandpass(mp)
        flen = len(taps) - 1
        n = np.arange((frame - 2) * HOP, min((frame + 3) * HOP, L))
        acc = np.zeros((inp.shape[0], len(n)), np.float32)
        for m in range(flen + 1):
            tim = n + flen // 2 - m
            ok = (tim >= 0) & (tim < L)
            acc[:, ok] = acc[:, ok] + inp[:, tim[ok]] * taps[m]
        out[:, n] = acc
    return out


# ---- fft, hilbert ----------------------------------------------------------------------------------------------------------------
def _bitrev(N):
    idx = np.arange(1 << N)
    rev = np.zeros_like(idx)
    for b in range(N):
        rev |= ((idx >> b) & 1) << (N - 1 - b)
    return rev


def fft(re, im, N, direct):
    """fft:1623-1677 on float32 [.., 2^N] arrays (the last axis is transformed), a stage at a time"""
    rev = _bitrev(N)
    re, im = re[..., rev].astype(np.float32), im[..., rev].astype(np.float32)
    lead = re.shape[:-1]
    for n in range(1, N + 1):
        period = 1 << (n - 1)
        tw = _tw(period, direct)
        u_r, u_i = tw[:, 0], tw[:, 1]
        r = re.reshape(lead + (-1, 2, period))
        i = im.reshape(lead + (-1, 2, period))
        lo_r, hi_r, lo_i, hi_i = r[..., 0, :], r[..., 1, :], i[..., 0, :], i[..., 1, :]
        t_r = hi_r * u_r - hi_i * u_i
        t_i = hi_r * u_i + hi_i * u_r
        re = np.stack((lo_r + t_r, lo_r - t_r), axis=-2).reshape(lead + (-1,))
        im = np.stack((lo_i + t_i, lo_i - t_i), axis=-2).reshape(lead + (-1,))
    return re, im


def normalised(patt):
    """computeAM:1170-1178: the pattern over its Hilbert envelope -> float32 [25][L].  A channel whose pattern is all zeros
    is not transformed: its spectrum and envelope are zeros and 0 / (0 + 1e-30) is 0."""
    live = patt.any(axis=1)
    if not live.all():
        out = np.zeros_like(patt)
        if live.any():
            out[live] = normalised(patt[live])
        return out
    L = patt.shape[1]
    N = fft_log2(L)
    sig_l = 1 << N
    re = np.zeros((patt.shape[0], sig_l), np.float32)
    re[:, :L] = patt
    re, im = fft(re, np.zeros_like(re), N, 1)
    re[:, 1:sig_l // 2] *= F32(2)
    im[:, 1:sig_l // 2] *= F32(2)
    re[:, sig_l // 2 + 1:] = 0
    im[:, sig_l // 2 + 1:] = 0
    re, im = fft(re, im, N, -1)
    env = np.sqrt(re[:, :L] * re[:, :L] + im[:, :L] * im[:, :L]) / F32(sig_l)
    return (patt.astype(np.float64) / (env.astype(np.float64) + 1e-30)).astype(np.float32)


# ---- computeAMRate, sinModel -----------------------------------------------------------------------------------------------------
def _cosf(x):
    return np.cos(x.astype(np.float64)).astype(np.float32)


def _sinf(x):
    return np.sin(x.astype(np.float64)).astype(np.float32)


def am_rate(am, pitch):
    """computeAMRate:1259-1287 + sinModel:1289-1317 on all (frame, channel) at once -> sEng, ratio, AmCrn float32 [F][25]"""
    L = am.shape[1]
    nfr = L // HOP
    seng = np.zeros((nfr, NCH), np.float32)
    ratio = np.zeros((nfr, NCH), np.float32)
    label = np.zeros((nfr, NCH), np.float32)
    if nfr < 3:
        return seng, ratio, label
    frames = np.arange(1, nfr - 1)
    start = (frames - 1) * HOP
    win = np.stack([am[:, s:s + WINDOW].T for s in start])  # [frames][200][25]
    e = np.zeros((len(frames), NCH), np.float32)
    for tim in range(WINDOW):
        e = e + win[:, tim] * win[:, tim]
    seng[1:nfr - 1] = e
    p = np.asarray(pitch[1:nfr - 1])
    voiced = p > 0
    freq = (F32(FS) / np.where(voiced, p, 1).astype(np.float32)).astype(np.float32)
    freq = (freq.astype(np.float64) * (2 * PI / FS)).astype(np.float32)[:, None]
    pa = np.zeros_like(e)
    pb = np.zeros_like(e)
    for tim in range(WINDOW):
        arg = freq * F32(tim)
        pa = pa + _cosf(arg) * win[:, tim]
        pb = pb + _sinf(arg) * win[:, tim]
    with np.errstate(invalid="ignore", divide="ignore"):
        phase = np.where(pa == 0, F32(PI / 2), np.arctan((-pb / pa).astype(np.float64)).astype(np.float32)).astype(np.float32)
    e1 = np.zeros_like(e)
    e2 = np.zeros_like(e)
    for tim in range(WINDOW):
        s = _cosf(freq * F32(tim) + phase)
        e1 = e1 + (win[:, tim] - s) * (win[:, tim] - s)
        e2 = e2 + (win[:, tim] + s) * (win[:, tim] + s)
    err = np.where(e1 < e2, e1, e2)
    run = voiced[:, None] & (e > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(run, err / np.where(run, e, 1), 0).astype(np.float32)
    ratio[1:nfr - 1] = r
    label[1:nfr - 1] = np.where(run & ~(r.astype(np.float64) > THETAE), 1, 0)
    return seng, ratio, label


def am_stage(g, pitch):
    """computeAM on gOut [25][L] and Pitch [F] -> dict ampatt, am [25][L], seng, ratio, amcrn [F][25], status"""
    L = g.shape[1]
    nfr = L // HOP
    pitch = np.asarray(pitch, np.int32)
    out = dict(ampatt=np.zeros((NCH, L), np.float32), am=np.zeros((NCH, L), np.float32), status=0,
               **{k: np.zeros((nfr, NCH), np.float32) for k in ("seng", "ratio", "amcrn")})
    if L > MAX_LEN:
        out["status"] = AM_TOO_LONG
        return out
    if (pitch > 100).any():
        out["status"] = AM_BAD_PITCH
        return out
    if nfr < 3 or not (pitch > 0).any():
        return out
    out["ampatt"] = am_patt(g, pitch)
    out["am"] = normalised(out["ampatt"])
    out["seng"], out["ratio"], out["amcrn"] = am_rate(out["am"], pitch)
    return out


# ---- finalSeg ------------------------------------------------------------------------------------------------------------------
def re_segmentation(m):
    """reSegmentation:1390-1440 on a bool array [F][25] -> (the pruned marks, the number of segments)"""
    nfr = m.shape[0]
    units, seg_mark = PM.segmentation(m.astype(np.float32))
    out = np.zeros_like(m)
    lo = 0
    for hi in seg_mark:
        us = units[lo:hi]
        fr = [f for _, f in us]
        if max(fr) - min(fr) + 1 >= MIN_SEG_LENGTH:
            for c, f in us:
                out[f, c] = True
        lo = hi
    return out, len(seg_mark)


def develope(m, v, grp):
    """develope:1442-1494, the reference's in-place sweep; returns the number of sweeps that changed something"""
    nfr = grp.shape[0]
    sweeps = 0
    judge = 1
    while judge:
        judge = 0
        for f in range(nfr):
            for c in range(NCH):
                if grp[f, c] == v:
                    for ff, cc in ((f - 1, c), (f + 1, c), (f, c - 1), (f, c + 1)):
                        if 0 <= ff < nfr and 0 <= cc < NCH and m[ff, cc] and grp[ff, cc] != v:
                            grp[ff, cc] = v
                            judge += 1
        sweeps += 1 if judge else 0
    return sweeps


def closure(m, v, grp, reverse=False):
    """the closure of {grp == v} over 4-neighbours with m set, by whole-array passes (optionally scanning backwards): what
    develope's fixpoint must be whatever the sweep order; returns the number of passes that changed something"""
    nfr = grp.shape[0]
    passes = 0
    while True:
        changed = False
        order = [(f, c) for f in range(nfr) for c in range(NCH)]
        for f, c in (reversed(order) if reverse else order):
            if grp[f, c] != v and m[f, c]:
                for ff, cc in ((f - 1, c), (f + 1, c), (f, c - 1), (f, c + 1)):
                    if 0 <= ff < nfr and 0 <= cc < NCH and grp[ff, cc] == v:
                        grp[f, c] = v
                        changed = True
                        break
        if not changed:
            return passes
        passes += 1


def final_seg(grp, amcrn, cross_ev, pratio, grow=develope):
    """finalSeg:1321-1388 and the binarisation -> dict mask, grp_final [F][25] float32, the five FINAL_STAGES, status"""
    grp = np.asarray(grp, np.float32)
    nfr = grp.shape[0]
    zero = np.zeros((nfr, NCH), np.float32)
    out = dict(mask=zero.copy(), grp_final=zero.copy(), status=0, **{k: zero.copy() for k in FINAL_STAGES})
    if nfr < 3:
        return out
    g = grp.astype(np.int32)
    am = np.asarray(amcrn, np.float32)
    cross = np.asarray(cross_ev, np.float32).astype(np.float64)
    pr = np.asarray(pratio, np.float32).astype(np.float64)
    st = {}
    too_many = False
    m, n = re_segmentation((g == 0) & (am != 0) & (cross > THETAC))
    too_many |= n > MAX_SEG
    g = g + 2 * m
    st[FINAL_STAGES[0]] = g.copy()
    sel = (g == 1) & (pr > THETAT)
    m, n = re_segmentation(sel)
    too_many |= n > MAX_SEG
    g[sel] = np.where(m[sel], 1, -2)
    st[FINAL_STAGES[1]] = g.copy()
    sel = (g == 1) & (pr <= THETAT)
    m, n = re_segmentation(sel)
    too_many |= n > MAX_SEG
    g[sel] = np.where(m[sel], -1, -2)
    st[FINAL_STAGES[2]] = g.copy()
    grow(g == -2, -1, g)
    g[(g == -2) | (g == 2)] = 1
    st[FINAL_STAGES[3]] = g.copy()
    grow((am == 1) & (g == 0), 1, g)
    st[FINAL_STAGES[4]] = g.copy()
    if too_many:
        out["status"] = FINAL_TOO_MANY_SEGMENTS
        return out
    out.update({k: v.astype(np.float32) for k, v in st.items()})
    out["grp_final"] = g.astype(np.float32)
    out["mask"] = (g > 0).astype(np.float32)
    return out


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def crc32(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def channel_crcs(a):
    """CRC32 of every channel's row of a float32 [25][L] array"""
    return np.array([crc32(row) for row in np.asarray(a, np.float32)], np.uint32)


def sample_index(L):
    """the flat indices into a [25][L] array whose values the fixture keeps beside the CRCs"""
    return np.linspace(0, NCH * L - 1, SAMPLES).astype(np.int64)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
