"""tests/hw25_model.py -- TEST INFRASTRUCTURE ONLY: a numpy model of the Hu-Wang estimator's front half on the 25-channel 8 kHz
bank (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:41-76), written from the formulas of that file and
HuWang.h: float32 wherever the reference's expression is float, float64 where it is double, every sum in the reference's
order.  The sample recurrences (gammatone, hair cell) and the ACF's step sum are Python loops over time with all channels /
frames / delays side by side; everything else is vectorised.

tests/test_hw25_cpu.py pins it bit for bit against what the reference's own functions produced (tests/golden/
hw25_golden.npz, written by tools/gen_hw25_golden.py); tests/test_gpu_hw25.py uses it as the expected value at shapes the
fixture does not hold.

The float overloads of the C++ math functions (expf, cosf, sinf, log10f, powf) are taken as the double function of the
promoted argument rounded once to float; that differs from a correctly rounded float function only where the double result
lies within 2^-29 ulp of a float rounding boundary, which the comparison with the fixture rules out for the values used.
"""
import math
import os

import numpy as np

from tests.gammatone_model import _BS_AF, _BS_BF, _BS_F, _BS_TF

FS, NCH, NDEL, MIN_DELAY, WINDOW, HOP, TAPS = 8000, 25, 101, 16, 200, 80, 91
THETAC, THETAA = 0.985, 50
PI = 3.1415926535897932384626433832795
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw25_golden.npz")
F = np.float32


def load_golden():
    """The fixture as a dict; the arrays stored as four byte planes (uint8 [4][shape]) are float32 again."""
    out = {}
    with np.load(GOLDEN) as z:
        for k in z.files:
            a = z[k]
            if a.dtype == np.uint8:
                a = np.ascontiguousarray(np.moveaxis(a, 0, -1)).view("<f4")[..., 0].astype(np.float32)
            out[k] = a
    return out


def frames(length):
    return max(int(length), 0) // HOP


# ---- the edge inputs ------------------------------------------------------------------------------------------------------
def edge_dc():
    """One frame of silence, then a step to -10000 held to the end (21 frames and 10 samples): very loud and very abrupt.  The
    gammatone's response to the constant settles below -MED_A in the low channels, so the hair cell's permeability is 0
    there, its cleft contents fall to exactly 0 (through the clamp at 8 kHz, by underflow at 16 kHz) and hOut and hEv are
    exactly 0 over whole ACF windows: both normalising sums of crossCorr are 0 (HuWang.cpp:408 and :413, the outcome `not
    divided`), pRatio is 0 / 0 there.  createIBM finds no segment in it: the front half alone judges it."""
    x = np.zeros(21 * HOP + 10, np.float32)
    x[HOP:] = -10000.0
    return x


def edge_whole():
    """A voice with vibrato from the first sample to the last (seed 1203), voiced up to the last frame: the last block of five
    frames is voiced and three frames long, so that amPatt's window runs past the signal's end (HuWang.cpp:1221, the outcome
    `no such sample`), and the last frame holds units for the searches and developes.

    33 frames and HOP // 2 + 17 samples: with a unit set in the last frame f the reference's resynthesis stays inside its
    weight array only if HOP f + (WINDOW - HOP - 1) < L (80 f + 119 < L at 25 bands; hw25_resynth_model.in_bounds), which
    asks for at least half a hop after the last whole frame."""
    L = 33 * HOP + HOP // 2 + 17
    n = np.arange(L, dtype=np.float64)
    f0 = 150.0 + 10.0 * np.sin(2 * np.pi * 2.5 * n / FS)
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(L)
    for h in range(1, 40):
        x += (2500.0 / h ** 0.6) * np.sin(h * ph) * (f0 * h < 0.475 * FS)
    return (x + np.random.default_rng(1203).normal(0, 40, L)).astype(np.float32)


EDGE_INPUTS = {"edc": edge_dc, "ewhole": edge_whole}


def edge_inputs():
    """the audio inputs of the edge set (tools/hw_oracle_coverage.py --set edge), by name"""
    return {k: make() for k, make in EDGE_INPUTS.items()}


# ---- step 1: the tables --------------------------------------------------------------------------------------------------
def _phons(freq):
    """loudnessLevelInPhons:184-204: float table rows, float interpolation, the closing expression in double"""
    f, af, bf, tf = (t.astype(np.float32) for t in (_BS_F, _BS_AF, _BS_BF, _BS_TF))
    i = 0
    while f[i] < freq:
        i += 1
    ratio = F(freq - f[i - 1]) / F(f[i] - f[i - 1])
    afy, bfy, tfy = (float(F(t[i - 1] + F(ratio * F(t[i] - t[i - 1])))) for t in (af, bf, tf))
    return F(4.2 + afy * (60.0 - tfy) / (1.0 + bfy * (60.0 - tfy)))


def _bessi0(x):
    """bessi0:1603-1621; only its small-argument branch is reached (beta < 3.75)"""
    assert abs(float(x)) < 3.75
    y = F(float(x) / 3.75)
    y = float(F(y * y))
    return F(1.0 + y * (3.5156229 + y * (3.0899424 + y * (1.2067492 + y * (0.2659732 + y * (0.360768e-1 + y * 0.45813e-2))))))


def tables():
    erb_lo = F(21.4 * math.log10(80 * 0.00437 + 1.0))
    erb_hi = F(21.4 * math.log10(4000 * 0.00437 + 1.0))
    step = F(erb_hi - erb_lo) / F(NCH - 1)
    dt = F(1) / F(FS)
    two_pi_t = F(2 * PI * float(dt))
    t = {k: np.zeros(NCH, np.float32) for k in ("cf", "bw", "midEarCoeff", "gain", "f1", "f2")}
    t["winsize"] = np.zeros(NCH, np.int32)
    for c in range(NCH):
        cf = F((math.pow(10.0, float(F(erb_lo + F(F(c) * step))) / 21.4) - 1) / 0.00437)
        bw = F(24.7 * (float(cf) * 0.00437 + 1.0) * 1.019)
        phon = F(float(_phons(cf)) - 60.0)
        ear = F(math.pow(10.0, float(F(phon / F(20)))))
        z = F(math.exp(float(F(-two_pi_t * bw))))
        t["cf"][c], t["bw"][c], t["midEarCoeff"][c] = cf, bw, ear
        t["gain"][c] = F(float(ear) * math.pow(float(F(two_pi_t * bw)), 4.0) / 3.0)
        t["f1"][c] = F(F(math.cos(float(F(cf * two_pi_t)))) * z)
        t["f2"][c] = F(F(math.sin(float(F(cf * two_pi_t)))) * z)
        t["winsize"][c] = max(WINDOW, int(F(4 * FS) / cf))
    # kaiserPara (0.01, 200 / 8000.), :1553-1569
    a = F(F(-20) * F(math.log10(float(F(0.01)))))
    trans_bw = F(F(200) / F(FS))
    assert 21 < a <= 50
    beta = F(0.5842 * float(F(math.pow(float(F(a - F(21))), float(F(0.4))))) + 0.07889 * float(F(a - F(21))))
    length = F((float(a) - 7.95) / 14.36 / float(trans_bw))
    flen = int(length)
    flen += 1 if float(F(length - F(flen))) < 0.5 else 2
    flen += flen % 2
    assert flen == TAPS - 1
    # kaiserLowPass (.., (1000 + 1200) / 8000.), :1576-1590
    wn = F(F(2200) / F(FS))
    lp = np.zeros(TAPS, np.float32)
    for tim in range(TAPS):
        k = F(F(F(2 * tim) / F(flen)) - F(1))
        f = F(_bessi0(F(beta * np.sqrt(F(F(1) - F(k * k))))) / _bessi0(beta))
        s = tim - flen // 2
        lp[tim] = F(float(f) * (math.sin(float(wn) * PI * s) / PI / s)) if s else F(f * wn)
    t["lp"] = lp
    # hairCell:261-274
    Y, G, L, R, X, A, B, H, M = 5.05, 2000.0, 2500.0, 6580.0, 66.31, 3.0, 300.0, 48000.0, 1.0
    d = float(dt)
    kt = float(F(G * A / (A + B)))
    c0 = F(M * Y * kt / (L * kt + Y * (L + R)))
    t["hair"] = np.array([Y * M * d, X * d, Y * d, (L + R) * d, R * d, G * d, H, float(c0) * (L + R) / kt, c0, float(c0) * R / X],
                         dtype=np.float32)  # ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0
    return t


# ---- step 2: the periphery -----------------------------------------------------------------------------------------------
def periphery(x, t):
    """gammaToneFilter:225-251 + hairCell:277-298 -> hOut float32 [25][L]"""
    x = np.asarray(x, dtype=np.float32)
    f1, f2, gain = t["f1"], t["f2"], t["gain"]
    ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0 = (F(v) for v in t["hair"])
    p = [np.zeros(NCH, np.float32) for _ in range(4)]
    q = [np.zeros(NCH, np.float32) for _ in range(4)]
    hq, hc, hw = (np.full(NCH, v, np.float32) for v in (q0, c0, w0))
    zero = F(0)
    out = np.zeros((NCH, len(x)), np.float32)
    for n in range(len(x)):
        g = p[3] * gain
        xs = [f1 * p[i] - f2 * q[i] for i in range(4)]
        ys = [f2 * p[i] + f1 * q[i] for i in range(4)]
        p[0] = x[n] * f1 + xs[0]
        q[0] = x[n] * f2 + ys[0]
        p[1] = p[0] + xs[1]
        q[1] = q[0] + ys[1]
        p[2] = p[1] + xs[1] + xs[2]
        q[2] = q[1] + ys[1] + ys[2]
        p[3] = p[2] + xs[1] + F(2) * xs[2] + xs[3]
        q[3] = q[2] + ys[1] + F(2) * ys[2] + ys[3]
        s = g.astype(np.float64) + 3.0
        kt = np.where(s > 0.0, (float(gdt) * s / (s + 300.0)).astype(np.float32), zero)
        replenish = np.where(hq < F(1), ymdt - ydt * hq, zero)
        eject = kt * hq
        loss = lplusrdt * hc
        reuptake = rdt * hc
        reprocess = xdt * hw
        hq = hq + replenish - eject + reprocess
        hq = np.where(hq < zero, zero, hq)
        hc = hc + eject - loss
        hc = np.where(hc < zero, zero, hc)
        hw = hw + reuptake - reprocess
        hw = np.where(hw < zero, zero, hw)
        out[:, n] = hdt * hc
    return out


def lowpass(hout, lp):
    """lowPass:318-328: hEv[n] = sum over m = 0..90 in order of hOut[n + 45 - m] filter[m], terms outside [0, L) skipped"""
    L = hout.shape[1]
    n = np.arange(L)
    out = np.zeros_like(hout)
    for m in range(TAPS):
        tim = n + (TAPS - 1) // 2 - m
        ok = (tim >= 0) & (tim < L)
        out[:, ok] = out[:, ok] + hout[:, tim[ok]] * lp[m]
    return out


# ---- step 3: the correlogram ---------------------------------------------------------------------------------------------
def acf(stream, winsize, reverse_steps=False):
    """computeACF:341-369 for one stream [25][L] -> [F][25][101].  reverse_steps: the same terms added from the oldest sample
    to the newest -- a mutant for the tests to tell from the reference's order."""
    L = stream.shape[1]
    nfr = frames(L)
    out = np.zeros((nfr, NCH, NDEL), np.float32)
    if not nfr:
        return out
    fr, d = np.arange(nfr)[:, None], np.arange(NDEL)[None, :]
    for c in range(NCH):
        s, ws = stream[c], int(winsize[c])
        acc = np.zeros((nfr, NDEL), np.float32)
        for step in (range(ws - 1, -1, -1) if reverse_steps else range(ws)):
            tim = (fr + 2) * HOP - (step + 1)
            ok = (tim - d >= 0) & (tim < L)
            prod = s[np.clip(tim, 0, L - 1)] * s[np.clip(tim - d, 0, L - 1)]
            acc = np.where(ok, acc + prod, acc)
        out[:, c, :] = acc / F(ws)
    return out


def cross_corr(a):
    """crossCorr:377-437 on [F][25][101] -> [F][25]"""
    mean = np.zeros(a.shape[:2], np.float32)
    for k in range(NDEL):
        mean = mean + a[:, :, k]
    mean = mean / F(NDEL)
    v = a - mean[:, :, None]
    sq = np.zeros(a.shape[:2], np.float32)
    for k in range(NDEL):
        sq = sq + v[:, :, k] * v[:, :, k]
    rms = np.sqrt(sq / F(NDEL))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where((rms != 0)[:, :, None], v / rms[:, :, None], v)
    out = np.zeros(a.shape[:2], np.float32)
    acc = np.zeros((a.shape[0], NCH - 1), np.float32)
    for k in range(NDEL):
        acc = acc + v[:, :-1, k] * v[:, 1:, k]
    out[:, :-1] = acc / F(NDEL)
    return out


def global_pitch(acf_hc):
    """globalPitch:445-461: the channel sums in channel order, the first strict maximum over delays 16..100"""
    total = np.zeros((acf_hc.shape[0], NDEL), np.float32)
    for c in range(NCH):
        total = total + acf_hc[:, c, :]
    return (MIN_DELAY + np.argmax(total[:, MIN_DELAY:], axis=1)).astype(np.int32)  # argmax takes the first of equal maxima


def p_ratio(acf_hc, pitch):
    """timeCrn:771-790: acf[chan][pitch] / max (acf[chan][pitch], acf[chan][16..100]); 0 / 0 is NaN"""
    at = np.take_along_axis(acf_hc, pitch[:, None, None].astype(np.int64), axis=2)[:, :, 0]
    mp = np.maximum(at, acf_hc[:, :, MIN_DELAY:].max(axis=2))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (at / mp).astype(np.float32)


def initial_mark(cross_hc, acf_hc):
    """createIBM:74-76: the cross test in double against 0.985, the energy test in float against (float)(50 * 50)"""
    return ((cross_hc.astype(np.float64) > THETAC) & (acf_hc[:, :, 0] > F(THETAA * THETAA))).astype(np.float32)


def frontend(x, t=None, reverse_steps=False):
    """Everything the GPU front half produces for one utterance, under the fixture's names."""
    t = t or tables()
    hout = periphery(x, t)
    hev = lowpass(hout, t["lp"])
    acf_hc, acf_ev = acf(hout, t["winsize"], reverse_steps), acf(hev, t["winsize"], reverse_steps)
    pitch = global_pitch(acf_hc)
    cross_hc = cross_corr(acf_hc)
    return dict(hOut=hout, hEv=hev, acf_hc=acf_hc, acf_ev=acf_ev, cross_hc=cross_hc, cross_ev=cross_corr(acf_ev), pitch=pitch,
                pRatio=p_ratio(acf_hc, pitch), mark=initial_mark(cross_hc, acf_hc))


def same_bits(got, want):
    """float arrays equal bit for bit, NaNs at the same places (sign and payload of a NaN are not compared)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    gn, wn = np.isnan(got), np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))
