#!/usr/bin/env python3
"""tools/gen_hw64_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw64_*.npz: four short float signals and what THE REFERENCE ITSELF makes of them in the front half of
createIBM() (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:41-76) at 16 kHz on 64 channels: data only,
no reference source.  Runs only where the reference tree exists:

    python tools/gen_hw64_golden.py [/root/reference]

HuWang.cpp is written entirely against the macros of HuWang.h.  The 16 kHz estimator is that file compiled against
resyth_64sub_IBM/cpp/HuWang.h (SAMPLING_FREQUENCY 16000, NUMBER_CHANNEL 64, MINCF 50, MAXCF 8000): HuWang.cpp is copied
UNMODIFIED into a temporary directory outside the repository, where its `#include "HuWang.h"` does not find the 8 kHz header
that sits beside the original, and compiled (g++ -O2 -ffp-contract=off) with -I resyth_64sub_IBM/cpp, whose own
NoiseSupExports.h supplies `struct mask`.  The driver is the one of tools/gen_hw25_golden.py, unchanged.

Inputs: the three harmonic signals of the hw25 tool at 16 kHz with L = 1770 (11 frames, not a multiple of 8 or 160: frames
0-7 cut the 1280 + 200 sample window at the start of the signal, 8 and 9 are whole, 10 is cut at the end), and d = the first
160 samples of a (one frame, every window cut at both ends).

Files (every one under 1 MiB):
    hw64_golden.npz        x_k; the tables cf, bw, midEarCoeff, winsize [64], lp [181]; per input cross_hc, cross_ev, pRatio,
                           mark [F][64], pitch [F]; all four large arrays of d; sha256_NAME_k, the SHA-256 of every large array's
                           little-endian float32 bytes, as uint8 [32]
    hw64_streams_k.npz     hOut_k, hEv_k [64][L], k = a, b, c
    hw64_acf_k.npz         acf_hc_k, acf_ev_k [F][64][201], k = a, b, c
The large float arrays are stored as their four byte planes, uint8 [4][shape], least significant byte first, as in
hw25_golden.npz.  tests/hw64_model.py::load_golden() puts everything together again.

Before hw64_golden.npz is written the tool asserts what tools/gen_hw25_golden.py asserts: on the instrumented 64-band build
under oracle/_ref/hwcov its inputs execute every executable line of HuWang.cpp:117-465 but that tool's UNREACHABLE.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_hw25_golden import DRIVER, assert_lines_executed, outcomes, planes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test", "HuWang.cpp")
INC = os.path.join("resyth_64sub_IBM", "cpp")
FS, NCH, NDEL, HOP, L_FULL = 16000, 64, 201, 160, 1770
LARGE = ("hOut", "hEv", "acf_hc", "acf_ev")
LIMIT = 1 << 20


def harmonic(L, amp, f0, nharm, noise, seed):
    """silence (or the noise alone) for the first third, then sum over h <= nharm of (amp / h) sin (2 pi f0 h n / 16000)"""
    n = np.arange(L, dtype=np.float64)
    x = np.zeros(L, np.float64)
    for h in range(1, nharm + 1):
        x += (amp / h) * np.sin(2 * np.pi * f0 * h * n / float(FS))
    x[n < L // 3] = 0.0
    if noise:
        x += np.random.default_rng(seed).uniform(-noise, noise, L)
    return x.astype(np.float32)


def inputs():
    a = harmonic(L_FULL, 30.0, 150.0, 3, 0.0, 0)
    return {"a": a,
            "b": harmonic(L_FULL, 300.0, 110.0, 8, 0.3, 20141106),
            "c": harmonic(L_FULL, 3000.0, 100.0, 30, 0.0, 0),
            "d": a[:HOP].copy()}


def build(ref_root, tmp):
    src, inc = os.path.join(ref_root, SRC), os.path.join(ref_root, INC)
    if not os.path.exists(src) or not os.path.exists(os.path.join(inc, "HuWang.h")):
        raise SystemExit(f"{src} or {inc}/HuWang.h is missing: this tool runs only where the reference tree exists")
    shutil.copy(src, os.path.join(tmp, "HuWang.cpp"))
    with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "hw64_ref")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-w", "-I", inc, os.path.join(tmp, "driver.cpp"),
                           os.path.join(tmp, "HuWang.cpp"), "-o", exe])
    return exe


def run(exe, tmp, x):
    fin, fout = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")
    x.tofile(fin)
    subprocess.check_call([exe, fin, fout], stdout=subprocess.DEVNULL)
    raw = np.fromfile(fout, np.uint8)
    pos = 0

    def take(dtype, *shape):
        nonlocal pos
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out = raw[pos:pos + n].view(dtype).reshape(shape).copy()
        pos += n
        return out

    L, F = len(x), len(x) // HOP
    r = {"cf": take(np.float32, NCH), "bw": take(np.float32, NCH), "midEarCoeff": take(np.float32, NCH),
         "winsize": take(np.int32, NCH)}
    flen = int(take(np.int32, 1)[0])
    r["lp"] = take(np.float32, flen + 1)
    r["hOut"], r["hEv"] = take(np.float32, NCH, L), take(np.float32, NCH, L)
    r["acf_hc"], r["acf_ev"] = take(np.float32, F, NCH, NDEL), take(np.float32, F, NCH, NDEL)
    r["cross_hc"], r["cross_ev"] = take(np.float32, F, NCH), take(np.float32, F, NCH)
    r["pRatio"], r["mark"] = take(np.float32, F, NCH), take(np.float32, F, NCH)
    r["pitch"] = take(np.int32, F)
    assert pos == len(raw), "the driver wrote more than was read"
    return r


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").tobytes()).digest(), np.uint8).copy()


def save(name, **arrays):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes")
    assert size < LIMIT, f"{name} must stay under 1 MiB"


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    data, total, pitches = {}, np.zeros(4, np.int64), set()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp)
        for k, x in inputs().items():
            r = run(exe, tmp, x)
            for name in ("cf", "bw", "midEarCoeff", "winsize", "lp"):
                if name in data:
                    assert np.array_equal(data[name], r[name])
                data[name] = r.pop(name)
            assert np.array_equal(r["mark"] == 1, (r["cross_hc"].astype(np.float64) > 0.985) & (r["acf_hc"][:, :, 0] > np.float32(2500)))
            assert not any(np.isnan(v).any() for v in r.values()), f"input {k}: NaN"
            data[f"x_{k}"] = x
            for name, v in r.items():
                if name in LARGE:
                    data[f"sha256_{name}_{k}"] = digest(v)
                    if k == "d":
                        data[f"{name}_{k}"] = planes(v)
                else:
                    data[f"{name}_{k}"] = v
            o = outcomes(r)
            print(f"input {k}: L {len(x)}, frames {len(x) // HOP}, labelled 1 / cross fails / energy fails / both: {o.tolist()}, "
                  f"pitches {sorted(set(r['pitch'].tolist()))}")
            if k == "d":
                continue
            assert (o >= 5).all(), f"input {k}: the labelling's four outcomes are {o.tolist()}: each needs 5 cells"
            total += o
            pitches |= set(r["pitch"].tolist())
            save(f"hw64_streams_{k}.npz", **{f"hOut_{k}": planes(r["hOut"]), f"hEv_{k}": planes(r["hEv"])})
            save(f"hw64_acf_{k}.npz", **{f"{n}_{k}": planes(r[n]) for n in ("acf_hc", "acf_ev")})
    assert len(data["lp"]) == 181 and data["winsize"][:8].tolist() == [1280, 978, 784, 647, 547, 470, 410, 360]
    assert (data["winsize"][8:] == 320).all() and int(data["winsize"].sum()) == 23396
    assert (total >= 5).all(), f"the labelling's four outcomes over (a)-(c) are {total.tolist()}: each needs 5 cells"
    print(f"outcomes over (a)-(c): {total.tolist()}, pitches {min(pitches)}..{max(pitches)}")
    assert_lines_executed("hw64", inputs().values())
    save("hw64_golden.npz", **data)


if __name__ == "__main__":
    main()
