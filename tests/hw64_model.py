"""tests/hw64_model.py -- TEST INFRASTRUCTURE ONLY: a numpy model of the Hu-Wang estimator's front half at 16 kHz on the
64-channel bank (HuWang.cpp:41-76 compiled against resyth_64sub_IBM/cpp/HuWang.h: SAMPLING_FREQUENCY 16000, NUMBER_CHANNEL 64,
MINCF 50, MAXCF 8000, WINDOW 320, OFFSET 160, MAX_DELAY 201, MIN_DELAY 32).

The reference's source is the same at both rates, and so is the model's: the functions of tests/hw25_model.py read the bank's
constants from their module's globals, so this file loads a second instance of that module and gives it the 64-band
constants.  Only tables() has the 8 kHz bank's numbers written into it and is restated here.

cos, sin and exp of a float are the C library's cosf, sinf and expf, which the reference's C++ overloads are, called through
ctypes: at channel 61 the library's sinf (cf * twoPiT) is one ulp above the correctly rounded value, which the double function
rounded once (the 25-band model's stand-in) gives; hOut of that channel tells the two apart.

tests/test_hw64_cpu.py pins the model bit for bit against what the reference's own functions produced (tests/golden/
hw64_*.npz, written by tools/gen_hw64_golden.py); the GPU tests use it as the expected value at shapes the fixture does not
hold.
"""
import ctypes
import ctypes.util
import glob
import hashlib
import importlib.util
import math
import os

import numpy as np

from tests import hw25_model as _M25

FS, NCH, NDEL, MIN_DELAY, WINDOW, HOP, TAPS = 16000, 64, 201, 32, 320, 160, 181
MINCF, MAXCF, PASSBAND, STOPBAND = 50, 8000, 1000, 1200
PI = _M25.PI
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGE = ("hOut", "hEv", "acf_hc", "acf_ev")
F = np.float32


def _libm_float(name):
    fn = getattr(ctypes.CDLL(ctypes.util.find_library("m")), name)
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return lambda v: F(fn(float(F(v))))


_cosf, _sinf, _expf = _libm_float("cosf"), _libm_float("sinf"), _libm_float("expf")


def _second_instance():
    spec = importlib.util.spec_from_file_location("tests._hw25_model_at_64_bands", _M25.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.FS, m.NCH, m.NDEL, m.MIN_DELAY, m.WINDOW, m.HOP, m.TAPS = FS, NCH, NDEL, MIN_DELAY, WINDOW, HOP, TAPS
    return m


_B = _second_instance()
frames, periphery, lowpass, acf, cross_corr, global_pitch, p_ratio, initial_mark, same_bits = (
    _B.frames, _B.periphery, _B.lowpass, _B.acf, _B.cross_corr, _B.global_pitch, _B.p_ratio, _B.initial_mark, _B.same_bits)
# the edge inputs of tests/hw25_model.py at this bank's rate and hop: the same docstrings hold, at 16 kHz
EDGE_INPUTS, edge_inputs = _B.EDGE_INPUTS, _B.edge_inputs


def load_golden():
    """The fixture's files as one dict; the arrays stored as four byte planes (uint8 [4][shape]) are float32 again, the
    digests (sha256_NAME_k, uint8 [32]) stay as they are."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "hw64_*.npz"))):
        with np.load(path) as z:
            for k in z.files:
                a = z[k]
                if a.dtype == np.uint8 and not k.startswith("sha256_"):
                    a = np.ascontiguousarray(np.moveaxis(a, 0, -1)).view("<f4")[..., 0].astype(np.float32)
                out[k] = a
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").tobytes()).digest(), np.uint8)


def equals_golden(got, g, name, k):
    """got against what the fixture holds of array `name` of input k: the array, bit for bit, and for a large array its
    SHA-256 as well (nothing in the fixture is NaN, so the bytes are the comparison)"""
    got = np.ascontiguousarray(got)
    ok = same_bits(got, g[f"{name}_{k}"])
    if name in LARGE:
        ok = ok and np.array_equal(digest(got), g[f"sha256_{name}_{k}"])
    return bool(ok)


def tables():
    """sea_build_hw64_tables's values from the reference's expressions (AudiPeriph:121-140, gammaToneFilter:216-223,
    computeACF:345-346, kaiserPara:1553-1569, kaiserLowPass:1576-1590, hairCell:261-274) at the 64-band header's constants"""
    erb_lo = F(21.4 * math.log10(MINCF * 0.00437 + 1.0))
    erb_hi = F(21.4 * math.log10(MAXCF * 0.00437 + 1.0))
    step = F(erb_hi - erb_lo) / F(NCH - 1)
    dt = F(1) / F(FS)
    two_pi_t = F(2 * PI * float(dt))
    t = {k: np.zeros(NCH, np.float32) for k in ("cf", "bw", "midEarCoeff", "gain", "f1", "f2")}
    t["winsize"] = np.zeros(NCH, np.int32)
    for c in range(NCH):
        cf = F((math.pow(10.0, float(F(erb_lo + F(F(c) * step))) / 21.4) - 1) / 0.00437)
        bw = F(24.7 * (float(cf) * 0.00437 + 1.0) * 1.019)
        phon = F(float(_M25._phons(cf)) - 60.0)
        ear = F(math.pow(10.0, float(F(phon / F(20)))))
        z = _expf(-two_pi_t * bw)
        t["cf"][c], t["bw"][c], t["midEarCoeff"][c] = cf, bw, ear
        t["gain"][c] = F(float(ear) * math.pow(float(F(two_pi_t * bw)), 4.0) / 3.0)
        t["f1"][c] = F(_cosf(cf * two_pi_t) * z)
        t["f2"][c] = F(_sinf(cf * two_pi_t) * z)
        t["winsize"][c] = max(WINDOW, int(F(4 * FS) / cf))
    a = F(F(-20) * F(math.log10(float(F(0.01)))))
    trans_bw = F(F(STOPBAND - PASSBAND) / F(FS))
    assert 21 < a <= 50
    beta = F(0.5842 * float(F(math.pow(float(F(a - F(21))), float(F(0.4))))) + 0.07889 * float(F(a - F(21))))
    length = F((float(a) - 7.95) / 14.36 / float(trans_bw))
    flen = int(length)
    flen += 1 if float(F(length - F(flen))) < 0.5 else 2
    flen += flen % 2
    assert flen == TAPS - 1
    wn = F(F(PASSBAND + STOPBAND) / F(FS))
    lp = np.zeros(TAPS, np.float32)
    for tim in range(TAPS):
        k = F(F(F(2 * tim) / F(flen)) - F(1))
        f = F(_M25._bessi0(F(beta * np.sqrt(F(F(1) - F(k * k))))) / _M25._bessi0(beta))
        s = tim - flen // 2
        lp[tim] = F(float(f) * (math.sin(float(wn) * PI * s) / PI / s)) if s else F(f * wn)
    t["lp"] = lp
    Y, G, L, R, X, A, B, H, M = 5.05, 2000.0, 2500.0, 6580.0, 66.31, 3.0, 300.0, 48000.0, 1.0
    d = float(dt)
    kt = float(F(G * A / (A + B)))
    c0 = F(M * Y * kt / (L * kt + Y * (L + R)))
    t["hair"] = np.array([Y * M * d, X * d, Y * d, (L + R) * d, R * d, G * d, H, float(c0) * (L + R) / kt, c0, float(c0) * R / X],
                         dtype=np.float32)  # ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0
    return t


def frontend(x, t=None, reverse_steps=False):
    """Everything the GPU front half produces for one utterance, under the fixture's names."""
    return _B.frontend(x, t or tables(), reverse_steps)
