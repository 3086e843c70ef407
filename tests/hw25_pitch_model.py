"""tests/hw25_pitch_model.py -- TEST INFRASTRUCTURE ONLY: a plain Python / numpy restatement of the Hu-Wang estimator's initial
grouping and pitch tracking (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp: initGroup:639-702 with
segmentation / search / relationship:466-637, pitchDtm:795-824 with findPitch, sumAuto, pitchCrn, checkPitch, leftDevelope,
rightDevelope, linearEstimate, timeCrn, reGroup and relationship2), written from the formulas of that file: float32 where the
reference's expression is float, float64 where it is double, every sum and every scan in the reference's order.

tests/test_hw25_pitch_cpu.py pins it against what the reference's own functions produced (tests/golden/hw25_pitch_golden.npz,
written by tools/gen_hw25_pitch_golden.py); tests/test_gpu_hw25_pitch.py uses it as the expected value where the fixture
holds nothing.  Where the reference is undefined the model takes the definitions of include/sea_mi355x.h:
  * no segment (rows < 3 included): segment count 0, pitch / grp / pratio all 0;
  * more than 400 segments: status bit 16 (TOO_MANY_SEGMENTS), pitch / grp / pratio all 0;
  * chan_mark read before leftDevelope / rightDevelope computed it: it starts at zeros, status bit 17 (CHANMARK_UNSET);
  * the Developes' number2 loop runs over 40 channels: on the last frame the fifteen past the arrays are not counted.
"""
import os
import zlib

import numpy as np

NCH, NDEL, MIN_DELAY, MAX_DELAY, HOP = 25, 101, 16, 101, 80
THETAP, THETAT = 0.95, 0.85
MAX_SEG = 400
TOO_MANY_SEGMENTS, CHANMARK_UNSET = 1 << 16, 1 << 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw25_pitch_golden.npz")
F32 = np.float32
AUDIO_CASES = ("p", "q", "r", "t", "m9")
PITCH_STAGES = ("pitch_find1", "pitch_find2", "pitch_check", "pitch_left", "pitch_right")
GRP_STAGES = ("grp_init", "grp_thetap")
FS = 8000


# ---- the inputs of the fixture ------------------------------------------------------------------------------------------------
def voiced(L, f0, amp, nharm, tilt=1.0):
    """f0: per-sample Hz, 0 = silent"""
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(L)
    for h in range(1, nharm + 1):
        x += (amp / h ** tilt) * np.sin(h * ph) * (f0 * h < 3800)
    x[f0 == 0] = 0
    return x


def mixed(seed):
    """the m<seed> family: one modulated voice, one to three intruders (noise bursts or a second voice), a noise floor"""
    rng = np.random.default_rng(seed)
    L = 10000
    n = np.arange(8400)
    base = rng.uniform(90, 220)
    f0 = np.zeros(L)
    f0[800:9200] = base * (1 + 0.15 * np.sin(2 * np.pi * rng.uniform(0.5, 3) * n / FS))
    x = voiced(L, f0, rng.uniform(800, 3000), int(rng.integers(6, 20)), rng.uniform(0.3, 1.2))
    for _ in range(int(rng.integers(1, 4))):
        a = int(rng.integers(2000, 8000))
        w = int(rng.integers(240, 900))
        if rng.random() < 0.5:
            x[a:a + w] += rng.normal(0, rng.uniform(1500, 6000), w)
        else:
            g = np.zeros(L)
            g[a:a + w] = base * rng.uniform(1.3, 1.9)
            x += voiced(L, g, rng.uniform(2000, 6000), 8)
    x += rng.normal(0, rng.uniform(50, 500), L)
    return x.astype(np.float32)


def audio_inputs():
    """p, q, r, s, t drawn in this order from one generator, then m9; s has no segment on the reference (model only)"""
    rng = np.random.default_rng(20141106)
    out = {}
    L = 12000
    f0 = np.zeros(L)
    f0[1600:6400] = np.linspace(100, 160, 4800)
    f0[8000:11200] = 200
    out["p"] = voiced(L, f0, 2000, 12) + rng.uniform(-40, 40, L)
    fa, fb = np.zeros(L), np.zeros(L)
    fa[800:11000] = 110
    fb[4000:9000] = np.linspace(230, 170, 5000)
    out["q"] = voiced(L, fa, 1500, 10) + voiced(L, fb, 2500, 8) + rng.uniform(-100, 100, L)
    L = 14000
    f0 = np.zeros(L)
    f0[800:4000] = 125
    f0[4000:4800] = 250
    f0[4800:8000] = 130
    f0[8800:9600] = 90
    f0[9600:13000] = np.linspace(180, 120, 3400)
    out["r"] = voiced(L, f0, 1200, 15) + rng.normal(0, 250, L)
    out["s"] = rng.normal(0, 800, 8000)
    L = 10000
    f0 = np.zeros(L)
    f0[1000:9000] = 140 + 30 * np.sin(2 * np.pi * 3 * np.arange(8000) / FS)
    out["t"] = voiced(L, f0, 3000, 20, 0.5) + rng.normal(0, 600, L)
    out = {k: v.astype(np.float32) for k, v in out.items()}
    out["m9"] = mixed(9)
    return out


def rect_case(nfr, segs):
    """acf 100 everywhere, 5000 at delay 0; seg = (f0, f1, c0, c1, delay, p) sets on its inclusive frame and channel ranges
    mark = 1, pratio = p and acf[..][delay] = 1100.  Returns acf [nfr][25][101], pratio, mark [nfr][25]."""
    acf = np.full((nfr, NCH, NDEL), 100, np.float32)
    acf[:, :, 0] = 5000
    pratio = np.zeros((nfr, NCH), np.float32)
    mark = np.zeros((nfr, NCH), np.float32)
    for f0, f1, c0, c1, delay, p in segs:
        mark[f0:f1 + 1, c0:c1 + 1] = 1
        pratio[f0:f1 + 1, c0:c1 + 1] = p
        acf[f0:f1 + 1, c0:c1 + 1, delay] = 1100
    return acf, pratio, mark


def handmade_case():
    """The hand-made input of 36 frames, four rectangular segments, each with its own peak delay and pRatio: the only input
    found that reaches `number == 0` in both Developes."""
    return rect_case(36, [(5, 30, 0, 3, 50, 0.5), (8, 12, 10, 12, 40, 0.99), (13, 19, 18, 20, 70, 0.99), (20, 24, 14, 16, 40, 0.99)])


def vote_case():
    """A frame that has + units and loses findPitch's vote OUTSIDE the outermost frame that keeps its pitch: at frame 3 two +
    channels peak at delay 40 and two at 70, sumAuto gives 40 and n2 * 2 <= n1 zeroes it.  findPitch takes lFrame from
    sumAuto's result BEFORE the vote (lFrame = 3, the first frame with a pitch left is 4), so leftDevelope reaches frame 3."""
    return rect_case(16, [(3, 12, 4, 5, 40, 0.99), (4, 7, 10, 12, 70, 0.99), (3, 3, 10, 11, 70, 0.99)])


def cross_case():
    """The one hand-made input with a cross array that decides a bit.  Channel 0 is marked over frames 5..12 and peaks at
    delay 20 from frame 6 on, at 60 in frame 5.  leftDevelope at frame 5 finds delay 20 in its window, the frame's own unit
    fails the ratio test (600 / 1100), and number2's forty-channel loop takes channel 25 for its only vote: flat element
    25 * 101 + 20, which is cross[5][20], over a maximum that is cross[5][20] too.  With cross zero the frame stays unvoiced.
    Returns acf, pratio, mark, cross."""
    acf, pratio, mark = rect_case(16, [(5, 12, 0, 0, 20, 0.99)])
    acf[5, 0, 20], acf[5, 0, 60] = 600, 1100
    cross = np.full((16, NCH), 0.5, np.float32)
    cross[5, 20] = 6000
    return acf, pratio, mark, cross


HAND_CASES = {"h": handmade_case, "v": vote_case, "x": cross_case}


def edge_grid_case():
    """Edge set: a segment that lies against three edges of the grid at once -- frame 0, the last frame and the top channel
    (channels NCH - 3 .. NCH - 1 over all 12 frames) -- and a second one inside.  The segment search meets a unit at frame 0
    (HuWang.cpp:590, the outcome `no earlier frame`), at the last frame (:602) and in the top channel (:626)."""
    return rect_case(12, [(0, 11, NCH - 3, NCH - 1, MIN_DELAY + 24, 0.99), (2, 9, 3, 5, MIN_DELAY + 24, 0.99)])


def edge_crn_case():
    """Edge set: pitchCrn decided by its last test (HuWang.cpp:897).  One segment whose peak delay is 41 over frames 2..7 and
    50 over frames 8..13 (twice that on the 64-channel bank): 41 lies within 20 % of 50 counted from 50 (above 40), 50 does
    not lie within 20 % of 41 (49.2), so `d1 > lowerP, d1 < upperP, d2 > lowerP` hold and `d2 < upperP` fails."""
    k = MIN_DELAY // 16
    return rect_case(16, [(2, 7, 4, 6, 41 * k, 0.99), (8, 13, 4, 6, 50 * k, 0.99)])


def edge_rclamp_case():
    """Edge set: rightDevelope's lower search bound clamped at MIN_DELAY (HuWang.cpp:1077): the mirror image of cross_case
    without its cross.  Channels 0-1 are marked over frames 3..12 and peak at delay MIN_DELAY + 1 up to frame 11, at three
    times that in frame 12, where the earlier delay keeps 600 of 1100.  rightDevelope at frame 12 finds the two delays
    inconsistent and searches from 0.65 (MIN_DELAY + 2) - 1, which lies below MIN_DELAY.  In frame 12 the delay MIN_DELAY - 1,
    which only a search without the clamp reaches and which is consistent with the earlier delay, holds 2000: with the clamp
    Pitch[12] is 0, without it MIN_DELAY - 1."""
    d = MIN_DELAY + 1
    acf, pratio, mark = rect_case(16, [(3, 12, 0, 1, d, 0.99)])
    acf[12, 0:2, d], acf[12, 0:2, 3 * d], acf[12, 0:2, MIN_DELAY - 1] = 600, 1100, 2000
    return acf, pratio, mark


def edge_lclamp_case():
    """Edge set: edge_rclamp_case with the frames in reverse order, for leftDevelope's clamp (HuWang.cpp:999; the older
    inputs take the outcome, but none of them changes when the clamp is removed): with the clamp Pitch[3] is 0, without
    it MIN_DELAY - 1."""
    return tuple(np.ascontiguousarray(a[::-1]) for a in edge_rclamp_case())


EDGE_HAND_CASES = {"egrid": edge_grid_case, "ecrn": edge_crn_case, "erclamp": edge_rclamp_case, "elclamp": edge_lclamp_case}


def hand_inputs(k):
    """acf, pratio, mark, cross of a hand-made case (cross zero where the case has none)"""
    c = {**HAND_CASES, **EDGE_HAND_CASES}[k]()
    return c if len(c) == 4 else c + (np.zeros_like(c[1]),)


def many_segments_case():
    """more than 400 segments and no checkerboard: 34 blocks of 3 frames x 13 isolated channels (0, 2, .., 24) = 442"""
    nfr = 34 * 4 + 1
    acf = np.full((nfr, NCH, NDEL), 100, np.float32)
    acf[:, :, 0] = 5000
    acf[:, :, 60] = 900
    mark = np.zeros((nfr, NCH), np.float32)
    for b in range(34):
        mark[1 + 4 * b:4 + 4 * b, 0::2] = 1
    pratio = np.where(mark > 0, F32(0.99), F32(0)).astype(np.float32)
    return acf, pratio, mark


def no_streak_case():
    """no streak of three consistent frames: one segment whose per-frame peak delay alternates between 30 and 60, so that
    checkPitch keeps nothing and rightDevelope starts at frame 2 with Pitch[1] == 0"""
    nfr = 12
    acf = np.full((nfr, NCH, NDEL), 100, np.float32)
    acf[:, :, 0] = 5000
    mark = np.zeros((nfr, NCH), np.float32)
    mark[1:11, 4:8] = 1
    for f in range(nfr):
        acf[f, 4:8, 30 if f % 2 else 60] = 1500
    pratio = np.where(mark > 0, F32(0.99), F32(0)).astype(np.float32)
    return acf, pratio, mark


# ---- segmentation:466-497 + search:584-637 ----------------------------------------------------------------------------------
def segmentation(mark, limit=None):
    """The reference's flood fill on a copy of the marks: the unit list (chan, frame) and segMark, the running unit count at the
    end of each segment.  limit: stop counting past it (the reference's segMark holds 400)."""
    m = np.array(mark) != 0
    nfr = m.shape[0]
    units, seg_mark = [], []
    for frame in range(1, nfr - 1):
        for chan in range(NCH):
            if m[frame, chan] and m[frame - 1, chan] and m[frame + 1, chan]:
                units.append((chan, frame))
                m[frame, chan] = False
                active = len(units) - 1
                while active < len(units):
                    c, f = units[active]
                    for ff, cc in ((f - 1, c), (f + 1, c), (f, c - 1), (f, c + 1)):
                        if 0 <= ff < nfr and 0 <= cc < NCH and m[ff, cc]:
                            units.append((cc, ff))
                            m[ff, cc] = False
                    active += 1
                seg_mark.append(len(units))
                if limit is not None and len(seg_mark) > limit:
                    return units, seg_mark
    return units, seg_mark


class _Segments:
    """per segment its units, sFrame / eFrame and, for a threshold, count[0] / count[1] per frame"""

    def __init__(self, units, seg_mark, nfr):
        self.nfr = nfr
        self.units = []
        lo = 0
        for hi in seg_mark:
            self.units.append(units[lo:hi])
            lo = hi
        self.s = [min(f for _, f in us) for us in self.units]
        self.e = [max(f for _, f in us) for us in self.units]

    def counts(self, pratio, above):
        out = []
        for us in self.units:
            cnt = np.zeros((2, self.nfr), np.int64)
            for c, f in us:
                cnt[0 if above(pratio[f, c]) else 1, f] += 1
            out.append(cnt)
        return out


def _relationship(sg, cnt):
    """relationship:499-558 -> (Longest, relation per segment)"""
    n = len(sg.units)
    length = longest = 0
    for i in range(n):
        if sg.e[i] - sg.s[i] > length:
            length, longest = sg.e[i] - sg.s[i], i
    cl = cnt[longest]
    count = 0
    for f in range(sg.s[longest], sg.e[longest] + 1):
        count += 1 if cl[0, f] > cl[1, f] else -1
    rel_l = -1 if count <= 0 else 1
    rel = []
    for i in range(n):
        n1 = n2 = 0
        for f in range(max(sg.s[longest], sg.s[i]), min(sg.e[longest], sg.e[i]) + 1):
            a, b, c, d = cl[0, f], cl[1, f], cnt[i][0, f], cnt[i][1, f]
            if (a > b and c > d) or (a < b and c < d):
                n1 += 1
            else:
                n2 += 1
        rel.append(rel_l if n1 > n2 * 2 else -rel_l)
    return longest, rel


def init_group(sg, pratio):
    """initGroup:639-702: pRatio (float) against the double THETAP; only the frames of the longest segment are labelled"""
    cnt = sg.counts(pratio, lambda v: float(v) > THETAP)
    longest, rel = _relationship(sg, cnt)
    grp = np.zeros((sg.nfr, NCH), np.float32)
    for i, us in enumerate(sg.units):
        for c, f in us:
            if sg.s[longest] <= f <= sg.e[longest]:
                grp[f, c] = rel[i]
    return grp


def re_group(sg, pratio, theta):
    """reGroup:704-764 + relationship2:560-582: pRatio against the FLOAT theta"""
    th = F32(theta)
    cnt = sg.counts(pratio, lambda v: F32(v) > th)
    grp = np.zeros((sg.nfr, NCH), np.float32)
    for i, us in enumerate(sg.units):
        n1 = n2 = 0
        for f in range(sg.s[i], sg.e[i] + 1):
            if cnt[i][0, f] >= cnt[i][1, f]:
                n1 += 1
            else:
                n2 += 1
        r = 1 if n1 >= n2 else -1
        for c, f in us:
            grp[f, c] = r
    return grp


# ---- the pitch side ------------------------------------------------------------------------------------------------------------
def sum_auto(m, acg, lo, hi):
    """sumAuto:862-885: per delay the channels with m > 0 in order, the first strict maximum from mvalue = 0"""
    pos, mvalue = 0, F32(0)
    chans = [c for c in range(NCH) if m[c] > 0]
    if lo >= hi:
        return 0
    total = np.zeros(hi - lo, np.float32)
    for c in chans:
        total = total + acg[c, lo:hi]
    for k in range(hi - lo):
        if total[k] > mvalue:
            mvalue, pos = total[k], lo + k
    return pos


def _mvalue(acf_row):
    """[25] the maximum of acf[c][16..100] from mvalue = 0 (a NaN never wins a comparison)"""
    a = acf_row[:, MIN_DELAY:MAX_DELAY]
    return np.maximum(np.nanmax(np.where(np.isnan(a), -np.inf, a), axis=1), 0).astype(np.float32)


def _ratio_above(acf_row, delay, mv):
    """[25] bool: (acf[c][delay] / mvalue) > THETAP, the float quotient against the double 0.95 (x / 0 is inf or NaN)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (acf_row[:, delay] / mv).astype(np.float32)
    return q.astype(np.float64) > THETAP


def find_pitch(acf, grp):
    """findPitch:826-860 -> (Pitch, lFrame, rFrame)"""
    nfr = acf.shape[0]
    pitch = np.zeros(nfr, np.int32)
    lf, rf = nfr, 0
    for f in range(nfr):
        p = sum_auto(grp[f], acf[f], MIN_DELAY, MAX_DELAY)
        if p > 0 and lf > f:
            lf = f
        if p > 0 and rf < f:
            rf = f
        pos = grp[f] > 0
        n1 = int(pos.sum())
        n2 = int((pos & _ratio_above(acf[f], p, _mvalue(acf[f]))).sum())
        pitch[f] = 0 if n2 * 2 <= n1 else p
    return pitch, lf, rf


def time_crn(acf, pitch):
    """timeCrn:766-791"""
    nfr = acf.shape[0]
    out = np.zeros((nfr, NCH), np.float32)
    for f in range(nfr):
        p = int(pitch[f])
        if p > 0:
            at = acf[f, :, p]
            a = acf[f, :, MIN_DELAY:MAX_DELAY]
            mx = np.nanmax(np.where(np.isnan(a), -np.inf, a), axis=1).astype(np.float32)
            mp = np.where(mx > at, mx, at)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[f] = (at / mp).astype(np.float32)
    return out


def pitch_crn(d1, d2):
    """pitchCrn:887-899: the double products stored in float variables, the ints compared as floats"""
    lower, upper = F32(0.8 * float(F32(d1))), F32(1.2 * float(F32(d1)))
    if d1 > d2:
        upper = F32(1.2 * float(F32(d2)))
    else:
        lower = F32(0.8 * float(F32(d2)))
    return int(F32(d1) > lower and F32(d1) < upper and F32(d2) > lower and F32(d2) < upper)


def check_pitch(pitch, lf, rf):
    """checkPitch:901-952 -> (pitch, buffer, sStreak, eStreak); sStreak = 0, eStreak = 1 to start with, as the reference"""
    buf = pitch.copy()
    pitch = np.zeros_like(pitch)
    ss, es = 0, 1
    frame = sf = ef = lf

    def close():
        nonlocal ss, es
        if ef - sf > es - ss:
            ss, es = sf, ef
        if ef - sf + 1 > 2:
            pitch[sf:ef + 1] = buf[sf:ef + 1]

    while frame < rf:
        if pitch_crn(int(buf[frame]), int(buf[frame + 1])):
            ef = frame + 1
        else:
            close()
            sf = ef = frame + 1
        frame += 1
    close()
    return pitch, buf, ss, es


def _window(b):
    """k1, k2 of the Develope functions: a double expression stored in a float, clamped, then int ()"""
    k1 = F32(0.65 * float(F32(b + 1)) - 1)
    if k1 < MIN_DELAY:
        k1 = F32(MIN_DELAY)
    k2 = F32(1.55 * float(F32(b + 1)) - 1)
    if k2 > MAX_DELAY - 1:
        k2 = F32(MAX_DELAY - 1)
    return int(k1), int(k2)


def _number2(acf, cross, pratio, grp, frame, p):
    """number2 of the Developes (:1009-1018, :1087-1096).  Its loop runs over FORTY channels on a bank of 25: channel 25 + j
    is, by the layout of the corrLgm and mask arrays, the flat element (25 + j) * 101 + delay of [acf | cross | pRatio | the
    next frame's acf] with the next frame's mark of channel j.  On the last frame those fifteen lie past the arrays: not
    counted (the model's fourth definition)."""
    n2 = int(((grp[frame] > 0) & _ratio_above(acf[frame], p, _mvalue(acf[frame]))).sum())
    if frame + 1 < acf.shape[0]:
        flat = np.concatenate((acf[frame].ravel(), cross[frame], pratio[frame], acf[frame + 1].ravel()))
        ghost = flat[NCH * NDEL:40 * NDEL].reshape(15, NDEL)
        n2 += int(((grp[frame + 1, :15] > 0) & _ratio_above(ghost, p, _mvalue(ghost))).sum())
    return n2


def _develope(acf, cross, pratio, grp, pitch, buf, start, stop, step, own_mark):
    """leftDevelope:954-1030 (step -1, own_mark: mark > 0) / rightDevelope:1032-1108 (step +1, own_mark: mark != 0).  Returns
    True when chan_mark was read before it was computed (it starts at zeros)."""
    chan_mark = np.zeros(NCH, bool)
    valid = unset = False
    frame = start
    while (frame >= stop) if step < 0 else (frame <= stop):
        nb = frame - step
        if pitch[nb]:
            chan_mark = (grp[nb] > 0) & _ratio_above(acf[nb], int(pitch[nb]), _mvalue(acf[nb]))
            valid = True
        if pitch_crn(int(buf[frame]), int(buf[nb])):
            pitch[frame] = buf[frame]
        else:
            unset = unset or not valid
            mark2 = own_mark(grp[frame]) & chan_mark
            number = int(mark2.sum())
            if number:
                k1, k2 = _window(int(buf[nb]))
                pitch[frame] = sum_auto(mark2.astype(np.float32), acf[frame], k1, k2)
                keep = False
                if pitch_crn(int(pitch[frame]), int(buf[nb])):
                    n2 = _number2(acf, cross, pratio, grp, frame, int(pitch[frame]))
                    keep = n2 * 2 > number
                if keep:
                    buf[frame] = pitch[frame]
                else:
                    pitch[frame] = 0
                    buf[frame] = buf[nb]
            else:
                buf[frame] = buf[nb]
        frame += step
    return unset


def linear_estimate(pitch, rf):
    """linearEstimate:1110-1142, `else if (sd)` as it stands: frame 0 never starts an interpolation"""
    frame = judge = sd = 0
    while frame <= rf:
        if pitch[frame]:
            if judge:
                k = F32(pitch[frame] - pitch[sd]) / F32(frame - sd)
                for t in range(sd + 1, frame):
                    pd = F32(F32(pitch[sd]) + F32(k * F32(t - sd)))
                    pitch[t] = int(pd)
                    if float(F32(pd - F32(pitch[t]))) >= 0.5:
                        pitch[t] += 1
                judge = 0
            sd = frame
        elif sd:
            judge = 1
        frame += 1


def pitch_stage(acf, pratio, mark, cross=None):
    """The whole stage on one utterance: acf [F][25][101], the front half's pratio, mark and cross_hc [F][25] (cross: zeros
    when not given; only _number2 reads it) -> dict with pitch, grp, pratio, status and the stage arrays (PITCH_STAGES,
    GRP_STAGES)."""
    acf = np.asarray(acf, np.float32).reshape(-1, NCH, NDEL)
    nfr = acf.shape[0]
    pratio = np.asarray(pratio, np.float32).reshape(nfr, NCH)
    mark = np.asarray(mark, np.float32).reshape(nfr, NCH)
    cross = np.zeros((nfr, NCH), np.float32) if cross is None else np.asarray(cross, np.float32).reshape(nfr, NCH)
    out = {k: np.zeros(nfr, np.int32) for k in ("pitch",) + PITCH_STAGES}
    out.update({k: np.zeros((nfr, NCH), np.float32) for k in ("grp", "pratio") + GRP_STAGES})
    units, seg_mark = segmentation(mark, MAX_SEG) if nfr >= 3 else ([], [])
    out["status"] = len(seg_mark)
    if len(seg_mark) > MAX_SEG:
        units, seg_mark = segmentation(mark)
        out["status"] = min(len(seg_mark), 0xFFFF) | TOO_MANY_SEGMENTS
        return out
    if not seg_mark:
        return out
    sg = _Segments(units, seg_mark, nfr)
    grp = out["grp_init"] = init_group(sg, pratio)
    pitch, lf, rf = find_pitch(acf, grp)
    out["pitch_find1"] = pitch.copy()
    pr = time_crn(acf, pitch)
    grp = out["grp_thetap"] = re_group(sg, pr, THETAP)
    pitch, lf, rf = find_pitch(acf, grp)
    out["pitch_find2"] = pitch.copy()
    pitch, buf, ss, es = check_pitch(pitch, lf, rf)
    out["pitch_check"] = pitch.copy()
    unset = _develope(acf, cross, pr, grp, pitch, buf, ss - 1, lf, -1, lambda m: m > 0)
    out["pitch_left"] = pitch.copy()
    unset = _develope(acf, cross, pr, grp, pitch, buf, es + 1, rf, +1, lambda m: m != 0) or unset
    out["pitch_right"] = pitch.copy()
    linear_estimate(pitch, rf)
    out["pitch"] = pitch
    out["pratio"] = time_crn(acf, pitch)
    out["grp"] = re_group(sg, out["pratio"], THETAT)
    if unset:
        out["status"] |= CHANMARK_UNSET
    return out


def crc32(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
