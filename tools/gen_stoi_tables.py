#!/usr/bin/env python3
"""Writes speech_enhancement_amd/csrc/stoi_tables.inc: the constant tables of the STOI contract,
computed in float64, rounded once to float32 and written as hex-float literals, so that the library and the plain-C model
(tests/stoi_model_driver.c) read the same bits whatever libm either machine has.

  w[256]     w[n] = 0.5 (1 - cos (2 pi (n + 1) / 257)): the 256 inner points of a 258-point Hann window (hanning (256))
  cs[512]    cs[j] = cos (2 pi j / 512): the basis of the 512-point transform, C[n][k] = cs[(n k) & 511],
             S[n][k] = cs[(n k + 128) & 511] = -sin (2 pi n k / 512)
  h16[161]   the 16 k -> 10 k resampler (p / q = 5 / 8), h8[101] the 8 k -> 10 k one (5 / 4): a Kaiser-windowed sinc, beta 5,
             half-length 10 max (p, q), cut-off 1 / (2 max (p, q)) of the upsampled rate, gain p -- the design of MATLAB's
             resample, not renormalised to unit sum.  sinc of a non-zero integer is exactly 0.  I0 by its power series.

Also stated and asserted here: the third-octave band edges on the 512-point transform at 10 kHz, and the clip constant.

    python tools/gen_stoi_tables.py            # rewrite the file
    python tools/gen_stoi_tables.py --print    # to stdout (tests/test_stoi_cpu.py compares it with the committed file)
"""
import math
import os
import struct
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech_enhancement_amd", "csrc", "stoi_tables.inc")
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
CLIP = "0x1.a7e600p+2"  # the float nearest 1 + 10^(15 / 20) = 6.6234132519...
BETA = 5.0


def f32(v):
    """v rounded once to float32, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", v))[0]


def lit(v):
    v = f32(v)
    m, e = math.frexp(abs(v))  # exact: a float32 has 24 significant bits
    if v == 0.0:
        return "0x0p+0f"
    digits = int(m * 2 ** 24)  # 24 bits, the top one set
    return f"{'-' if v < 0 else ''}0x1.{(digits & 0x7FFFFF) << 1:06x}p{e - 1:+d}f"


def bessel_i0(x):
    """I0 (x) = sum over k of ((x / 2)^k / k!)^2"""
    total, term, k = 1.0, 1.0, 0
    while term > 1e-20 * total:
        k += 1
        term *= (x / 2.0 / k) ** 2
        total += term
    return total


def taps(p, q):
    big = max(p, q)
    half = 10 * big
    out = []
    for n in range(-half, half + 1):
        sinc = 1.0 if n == 0 else 0.0 if n % big == 0 else math.sin(math.pi * n / big) / (math.pi * n / big)
        window = bessel_i0(BETA * math.sqrt(1.0 - (n / half) ** 2)) / bessel_i0(BETA)
        out.append(p * sinc / big * window)
    return out


def band_edges():
    """stoi.m's thirdoct (10000, 512, 15, 150): the bin nearest each band's lower and upper edge; a band is lo .. hi - 1"""
    freqs = [k * 10000.0 / 512 for k in range(257)]
    nearest = lambda f: min(range(257), key=lambda k: (freqs[k] - f) ** 2)  # noqa: E731
    lo, hi = [], []
    for j in range(15):
        cf = 150.0 * 2.0 ** (j / 3.0)
        lo.append(nearest(cf * 2.0 ** (-1.0 / 6.0)))
        hi.append(nearest(cf * 2.0 ** (1.0 / 6.0)))
    return lo, hi


def table(name, values):
    rows = [", ".join(lit(v) for v in values[i:i + 6]) for i in range(0, len(values), 6)]
    return f"#define {name}_N {len(values)}\n#define {name}_VALUES \\\n    " + ", \\\n    ".join(rows) + "\n"


def text():
    lo, hi = band_edges()
    assert tuple(lo) == BAND_LO[:15] and tuple(hi) == BAND_LO[1:], (lo, hi)
    assert lit(1.0 + 10.0 ** (15.0 / 20.0)) == CLIP + "f", lit(1.0 + 10.0 ** (15.0 / 20.0))
    w = [0.5 * (1.0 - math.cos(2.0 * math.pi * (n + 1) / 257.0)) for n in range(256)]
    cs = [math.cos(2.0 * math.pi * j / 512.0) for j in range(512)]
    h16, h8 = taps(5, 8), taps(5, 4)
    assert len(h16) == 161 and len(h8) == 101
    assert all(float.fromhex(lit(v)[:-1]) == f32(v) for t in (w, cs, h16, h8) for v in t)
    head = ("/* stoi_tables.inc -- written by tools/gen_stoi_tables.py; do not edit.  The constant tables of the STOI contract\n"
            " * (DESIGN.md section 5.24): float64 values rounded once to float. */\n")
    consts = (f"#define SEA_STOI_CLIP {CLIP}f /* the float nearest 1 + 10^(15 / 20) */\n"
              f"#define SEA_STOI_BAND_LO {', '.join(str(v) for v in BAND_LO)}\n")
    return head + consts + table("SEA_STOI_W", w) + table("SEA_STOI_CS", cs) + table("SEA_STOI_H16", h16) + table("SEA_STOI_H8", h8)


if __name__ == "__main__":
    if "--print" in sys.argv:
        sys.stdout.write(text())
    else:
        with open(OUT, "w") as f:
            f.write(text())
