"""tests/hw25_resynth_model.py -- TEST INFRASTRUCTURE ONLY: a numpy restatement of the Hu-Wang estimator's resynthesis
(function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1498-1549), written from the loop of that function: float32
where the reference's expression is float, float64 where it is double, every `+=` in the reference's order.

Per channel c = 0..24 in order: reverse[L-1-n] = gOut[c][n] / midEarCoeff[c]; gammaToneFilter on it (state zeroed, the output
taken before the update); reverse[L-1-n] = that / midEarCoeff[c]; weight = 0, then for every frame in ascending order whose
mark is set, `weight[(frame-1)*80 + n] += 0.5*(1.0+cos(n*PI/80+PI))` for n = 0..79 unless frame is 0, and `weight[(frame-1)*80
+ n] += 0.5*(1.0+cos((n-80)*PI/80))` for n = 80..199 (WINDOW is 200, OFFSET 80: 120 samples, the last 40 of which rise again),
each a double sum rounded to float; resynth[t] += weight[t] * reverse[t], from +0.0f.

The drop rule: the reference's frame loop writes weight[] up to index 80 F + 39 of L (F = L // 80), past the array when L % 80
< 40 and the last row has a unit set.  The engine drops what lies at indices >= L, and so does weights() below.  The reference
pins this model (tests/golden/hw25_resynth_golden.npz, tools/gen_hw25_resynth_golden.py) only on inputs where every channel's
largest set frame f has 80 f + 119 < L (in_bounds()); elsewhere the model alone says what the engine must give.

tests/test_hw25_resynth_cpu.py pins the model against the fixture; tests/test_gpu_hw25_resynth.py uses it where the fixture
holds nothing.
"""
import functools
import math
import os

import numpy as np

from tests import hw25_am_model as AM
from tests import hw25_model as M

NCH, HOP, WINDOW = 25, 80, 200
PI = 3.1415926535897932384626433832795
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw25_resynth_golden.npz")
F32 = np.float32
# the audio inputs of tests/hw25_am_model.audio_inputs() on which createIBM's own mask keeps the reference in bounds; on m9 and r
# it sets units in frame 49 of 50 at L = 4000, where the reference writes past weight[]: the model alone pins those two
AUDIO_CASES = ("p", "q", "t", "w1600", "w2048", "p12000")
MODEL_ONLY_CASES = ("m9", "r")
HAND_INPUTS = ("w2048", "t1640")
HAND_MASKS = ("ones", "checker", "frame0", "last", "single", "soft")
TEXT_CASES = ("a_w1600", "h_t1640_checker")  # the cases whose text file the fixture keeps whole; the others as a CRC32


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _audio():
    return AM.audio_inputs()


def hand_input(name):
    """w2048: L % 80 = 48; t1640: 1640 samples of t, L % 80 = 40, where frame 19's last index 80 * 19 + 119 is exactly L - 1"""
    xs = _audio()
    return {"w2048": xs["w2048"], "t1640": np.ascontiguousarray(xs["t"][:1640])}[name]


def hand_mask(name, nfr):
    """float32 [nfr][25]; `soft` holds 0.3 and 0.7 beside 0 (every other mask is 0 / 1)"""
    m = np.zeros((nfr, NCH), np.float32)
    f, c = np.indices(m.shape)
    if name == "ones":
        m[:] = 1
    elif name == "checker":
        m[(f + c) % 2 == 0] = 1
    elif name == "frame0":
        m[0] = 1
    elif name == "last":
        m[nfr - 1] = 1
    elif name == "single":
        m[nfr // 2, 7] = 1
    elif name == "soft":
        m[(f + 2 * c) % 3 == 0] = 0.3
        m[(f + 2 * c) % 3 == 1] = 0.7
    else:
        raise KeyError(name)
    return m


def reference_cases(am_golden):
    """name -> (x, mask float32 [F][25] of 0 / 1) for every case of the fixture: the audio cases with createIBM's own mask (as
    tests/golden/hw25_am_golden.npz holds it), then the hand-made masks; `soft` goes to the reference as mark > 0"""
    out = {}
    for k in AUDIO_CASES:
        out[f"a_{k}"] = (_audio()[k], am_golden[f"mask_{k}"].astype(np.float32))
    for i in HAND_INPUTS:
        x = hand_input(i)
        for name in HAND_MASKS:
            out[f"h_{i}_{name}"] = (x, (hand_mask(name, len(x) // HOP) > 0).astype(np.float32))
    return out


def in_bounds(mask_set, L):
    """every channel's largest set frame f satisfies 80 f + 119 < L: the reference stays inside weight[]"""
    frames = np.flatnonzero(np.asarray(mask_set, bool).any(axis=1))
    return not len(frames) or HOP * int(frames[-1]) + (WINDOW - HOP - 1) < L


# ---- the overlap-add weight -----------------------------------------------------------------------------------------------------
def ola_tables():
    """the reference's two double expressions: up [80] (:1530) and down [120] (:1534)"""
    up = np.array([0.5 * (1.0 + math.cos(n * PI / HOP + PI)) for n in range(HOP)], np.float64)
    down = np.array([0.5 * (1.0 + math.cos((n - HOP) * PI / HOP)) for n in range(HOP, WINDOW)], np.float64)
    return up, down


def weights(mask_set, L):
    """:1521-1536 as the literal `+=` sequence, float32 [25][L]; what falls at indices >= L is dropped"""
    up, down = ola_tables()
    mask_set = np.asarray(mask_set, bool)
    w = np.zeros((NCH, L), np.float32)
    for c in range(NCH):
        for frame in np.flatnonzero(mask_set[:, c]):
            parts = [(np.arange(HOP, WINDOW), down)]
            if frame > 0:
                parts.insert(0, (np.arange(HOP), up))
            for n, term in parts:
                idx = (frame - 1) * HOP + n
                keep = idx < L
                w[c, idx[keep]] = (w[c, idx[keep]].astype(np.float64) + term[keep]).astype(np.float32)
    return w


def weight_table():
    """float32 [80][8]: the weight at position o of a hop for the eight states of the frames k - 1, k, k + 1 (bit 0, 1, 2), read
    off weights() on five-frame masks at frame k = 2 -- independent of how the engine's host table is built"""
    out = np.zeros((HOP, 8), np.float32)
    for bits in range(8):
        m = np.zeros((5, NCH), bool)
        for b in range(3):
            m[1 + b, 0] = bool(bits >> b & 1)
        out[:, bits] = weights(m, 5 * HOP)[0, 2 * HOP:3 * HOP]
    return out


# ---- the second pass ---------------------------------------------------------------------------------------------------------------
def gammatone_rows(xin, t):
    """gammaToneFilter:225-251, channel c on row c of xin float32 [25][L] -> float32 [25][L]"""
    f1, f2, gain = t["f1"], t["f2"], t["gain"]
    p = [np.zeros(NCH, np.float32) for _ in range(4)]
    q = [np.zeros(NCH, np.float32) for _ in range(4)]
    out = np.zeros_like(xin)
    for n in range(xin.shape[1]):
        out[:, n] = p[3] * gain
        xs = [f1 * p[i] - f2 * q[i] for i in range(4)]
        ys = [f2 * p[i] + f1 * q[i] for i in range(4)]
        p[0] = xin[:, n] * f1 + xs[0]
        q[0] = xin[:, n] * f2 + ys[0]
        p[1] = p[0] + xs[1]
        q[1] = q[0] + ys[1]
        p[2] = p[1] + xs[1] + xs[2]
        q[2] = q[1] + ys[1] + ys[2]
        p[3] = p[2] + xs[1] + F32(2) * xs[2] + xs[3]
        q[3] = q[2] + ys[1] + F32(2) * ys[2] + ys[3]
    return out


def reverse_pass(g, t):
    """:1513-1519 -> `reverse` float32 [25][L], in forward time"""
    ear = t["midEarCoeff"][:, None]
    with np.errstate(all="ignore"):
        rin = np.ascontiguousarray((np.asarray(g, np.float32) / ear)[:, ::-1])
        return np.ascontiguousarray((gammatone_rows(rin, t) / ear)[:, ::-1])


def resynth_from_reverse(rev, mask, threshold=0.0):
    """:1521-1540: the weights of `mask > threshold` and the sum over the channels in order from +0.0f"""
    L = rev.shape[1]
    with np.errstate(invalid="ignore"):
        w = weights(np.asarray(mask, np.float32).reshape(-1, NCH) > F32(threshold), L)
    out = np.zeros(L, np.float32)
    with np.errstate(all="ignore"):
        for c in range(NCH):
            out = out + w[c] * rev[c]
    return out


def resynth(g, mask, threshold=0.0, t=None):
    """resynthesis (mask) on gOut `g` float32 [25][L] -> float32 [L]"""
    return resynth_from_reverse(reverse_pass(g, t or M.tables()), mask, threshold)


@functools.lru_cache(maxsize=None)
def _reverse_of_input(name):
    x = _audio()[name] if name in _audio() else hand_input(name)
    t = M.tables()
    return reverse_pass(AM.gout(x, t), t)


def resynth_input(name, mask, threshold=0.0):
    """resynth() on a named input of the fixture (audio_inputs()'s, or a hand input); the two filter passes are computed once"""
    return resynth_from_reverse(_reverse_of_input(name), mask, threshold)


# ---- the outputs' other forms --------------------------------------------------------------------------------------------------
def to_short(v):
    """(short) of a float as the x86-64 build converts it (cvttss2si + low half): int32 truncating toward zero, the low 16 bits;
    NaN or a magnitude of 2^31 and more give 0"""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(v) < 2147483648.0
    i = np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16).view(np.int16)


def text(v):
    """the file resynthesis() writes (:1543-1544): "%f\\n" per sample"""
    return b"".join(b"%f\n" % float(s) for s in np.asarray(v, np.float32))


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
