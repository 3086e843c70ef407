#!/usr/bin/env python3
"""tools/gen_hw64_am_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw64_am_golden.npz: what THE REFERENCE ITSELF makes of a few signals in computeAM, finalSeg and the final
binarisation (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1146-1494, :99-106, with the tools of
:1553-1677) when it is compiled against the 64-band header resyth_64sub_IBM/cpp/HuWang.h (SAMPLING_FREQUENCY 16000,
NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320): data only, no reference source.  Runs only where the reference tree exists:

    python tools/gen_hw64_am_golden.py <reference tree>

The procedure is tools/gen_hw25_am_golden.py's, and so is the code: this file loads a second instance of that module at 64
channels and a hop of 160, as tools/gen_hw64_pitch_golden.py does with the pitch tool.  HuWang.cpp is copied UNMODIFIED to a
temporary directory outside the repository and compiled there against the 64-band header into a shared library; the
interposing driver of that tool (our own code, which only CALLS the reference) is linked against it; createIBM is called once
per audio input (tests/hw64_am_model.py::audio_inputs) and finalSeg once per hand-made case (HAND_CASES).  The fixture holds
what tools/gen_hw25_am_golden.py describes, at [F][64].

Asserted before anything is written:
  * a --coverage build executes every executable line of HuWang.cpp:1146-1494, and of :1553-1677 all but the three lines
    that the constants make unreachable (UNREACHABLE of the 25-band tool: delta = 0.01 knows neither rate nor bank);
  * the model (tests/hw64_am_model.py: the 25-band model's functions at the 64-band constants, no literal rate or channel
    count) equals the reference on gOut, the pattern, the normalised pattern, sEng, AmCrn, every stage of finalSeg and the
    mask, bit for bit, on every input: no rate or channel literal hides in the reference's stage;
  * no unit's reference ratio lies within ratio_tol (twice the largest relative difference between the model's ratio and the
    reference's, measured here on the CPU) of THETAE.  A condition on the inputs: replace the input, widen nothing;
  * each input reaches the point it was chosen for (purposes () below).  One point no audio input can reach: a block
    without a voiced frame BETWEEN voiced ones, because linearEstimate fills every such run of frames
    (tests/hw64_am_model.py::audio_inputs says when it does not); the tests make that block by hand;
  * the fixture stays under 1 MiB.
"""
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hw64_am_model as AM  # noqa: E402
from tests import hw64_model as M  # noqa: E402

PATH = AM.GOLDEN
SRC = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test", "HuWang.cpp")
INC = os.path.join("resyth_64sub_IBM", "cpp")
NCH, HOP, BLOCK = AM.NCH, AM.HOP, 5 * AM.HOP


def _second_instance():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen_hw25_am_golden.py")
    spec = importlib.util.spec_from_file_location("gen_hw25_am_golden_at_64_bands", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.NCH, m.HOP, m.AM, m.M, m.PATH = NCH, HOP, AM, M, PATH
    return m


G = _second_instance()


def build(ref_root, tmp, name, extra):
    """HuWang.cpp unmodified, compiled against the 64-band header into a shared library, the driver linked against it"""
    src, inc = os.path.join(ref_root, SRC), os.path.join(ref_root, INC)
    if not os.path.exists(src) or not os.path.exists(os.path.join(inc, "HuWang.h")):
        raise SystemExit(f"{src} or {inc}/HuWang.h is missing: this tool runs only where the reference tree exists")
    work = os.path.join(tmp, name)
    os.makedirs(work)
    shutil.copy(src, os.path.join(work, "HuWang.cpp"))
    with open(os.path.join(work, "driver.cpp"), "w") as fh:
        fh.write(G.DRIVER)
    exe = os.path.join(work, "hw64_am_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-fPIC", "-w", *extra, "-I", inc]
    subprocess.check_call(flags + ["-c", "HuWang.cpp", "-o", "HuWang.o"], cwd=work)
    subprocess.check_call(["g++", "-shared", *extra, "HuWang.o", "-o", "libhuwang.so"], cwd=work)
    subprocess.check_call(flags + ["-c", "driver.cpp", "-o", "driver.o"], cwd=work)
    subprocess.check_call(["g++", "-rdynamic", *extra, "driver.o", "-L", work, "-lhuwang", "-ldl", "-Wl,-rpath," + work, "-o", exe],
                          cwd=work)
    return exe


def blocks_of(pitch, L):
    """per block of five frames: (mean pitch or None, fLength or 0), as amPatt sees them"""
    out = []
    for frame in range(2, L // HOP, 5):
        mp = AM.block_mean_pitch(pitch, frame)
        out.append((None, 0) if mp is None else (float(mp), AM.filter_length(mp)))
    return out


def purposes(r, data):
    """what each input was chosen for -> {name: bool}"""
    info = {k: (len(data[f"x_{k}"]), blocks_of(r[k]["pitch"], len(data[f"x_{k}"]))) for k in r}

    def reaches_outside(k, at_least):
        L, bl = info[k]
        first = [b for b, (mp, fl) in enumerate(bl) if fl >= at_least and b * BLOCK - fl // 2 < 0]
        last = [b for b, (mp, fl) in enumerate(bl) if fl >= at_least and b * BLOCK + BLOCK + fl // 2 > L]
        return bool(first) and bool(last)

    late = {k: (v["final_dev_plus"][:, 40:] == 1) & (v["final_dev_minus"][:, 40:] == 0) for k, v in r.items()}
    return {
        "an input with N <= 12 and one with N >= 13": min(v["N"] for v in r.values()) <= 12 and r["p11900"]["N"] >= 13,
        "a length that is a power of two": len(data["x_w4096"]) == 4096 and r["w4096"]["N"] == 12,
        "at least nine blocks": len(info["p11900"][1]) >= 9,
        "frames not a multiple of 5, length not a multiple of 160": (info["p11900"][0] // HOP) % 5 != 0 and info["p11900"][0] % HOP != 0,
        "a block mean near 200 whose window leaves the utterance at both ends": reaches_outside("lo", 1060),
        "a block mean near 32": any(mp is not None and mp <= 36 for mp, _ in info["hi"][1]),
        "a block without a voiced frame before the first or after the last voiced one": any(
            None in [mp for mp, _ in bl] for _, bl in info.values()),
        "AM labels in channels 40..63": any(v["amcrn"][:, 40:].any() for v in r.values()),
        "mask units in channels 40..63 that only develope adds": any(m.any() for m in late.values()),
    }


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/gen_hw64_am_golden.py <reference tree>")
    ref_root = sys.argv[1]
    data, results = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp, "plain", [])
        cov = build(ref_root, tmp, "cov", ["--coverage"])
        for k, v in G.run_constants(exe, tmp).items():
            data[k] = v
        G.run_constants(cov, tmp)
        print(f"N at 2^7..2^17: {data['n_at_pow2'].tolist()}, beta {data['beta']!r}")
        t = M.tables()
        worst, refs = 0.0, []
        for k, x in AM.audio_inputs().items():
            r = G.run_audio(exe, tmp, x)
            c = G.run_audio(cov, tmp, x)
            assert all(np.asarray(c[n]).tobytes() == np.asarray(r[n]).tobytes() for n in r), f"{k}: the coverage build differs"
            L = len(x)
            assert r["N"] == AM.fft_log2(L)
            idx = AM.sample_index(L)
            data[f"x_{k}"] = x
            for name in ("pitch", "grp", "cross_ev", "pratio", "seng", "ratio", "amcrn", "grp_final", "mask") + AM.FINAL_STAGES:
                data[f"{name}_{k}"] = r[name]
            for name in ("gout", "ampatt", "am"):
                data[f"{name}_crc_{k}"] = AM.channel_crcs(r[name])
                data[f"{name}_s_{k}"] = r[name].ravel()[idx]
            # the model, which holds no rate or channel literal, on the same input: exact on every array but ratio
            g = AM.gout(x, t)
            assert M.same_bits(g, r["gout"]), f"{k}: the model's gOut differs"
            m = AM.am_stage(g, r["pitch"])
            for name in ("ampatt", "am", "seng"):
                assert M.same_bits(m[name], r[name]), f"{k}: the model's {name} differs from the reference's"
            assert np.array_equal(m["amcrn"], r["amcrn"].astype(np.float32)), f"{k}: the model's AmCrn differs"
            f = AM.final_seg(r["grp"], r["amcrn"], r["cross_ev"], r["pratio"])
            for name in AM.FINAL_STAGES + ("grp_final", "mask"):
                assert np.array_equal(f[name], r[name].astype(np.float32)), f"{k}: the model's {name} differs"
            run = r["ratio"] != 0
            rel = np.abs(m["ratio"][run].astype(np.float64) - r["ratio"][run]) / r["ratio"][run]
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            refs.append(r["ratio"][run].astype(np.float64))
            results[k] = r
            print(f"input {k}: L {L}, N {r['N']}, frames {L // HOP}, voiced {int((r['pitch'] > 0).sum())}, pitches "
                  f"{int(r['pitch'][r['pitch'] > 0].min()) if run.any() else 0}..{int(r['pitch'].max())}, sinModel units {int(run.sum())}, "
                  f"AM labels {int(r['amcrn'].sum())} ({int(r['amcrn'][:, 40:].sum())} in channels 40..63), mask units "
                  f"{int(r['mask'].sum())}, model ratio rel. diff {float(rel.max()) if rel.size else 0:.3g}, blocks "
                  f"{[(round(mp, 1), fl) if mp else None for mp, fl in blocks_of(r['pitch'], L)]}")
        tol = 2 * worst
        refs = np.concatenate(refs)
        band = int((np.abs(refs - AM.THETAE) <= tol * AM.THETAE).sum())
        print(f"ratio_tol {tol:.3g}; units within it of THETAE: {band}; nearest {np.abs(refs - AM.THETAE).min():.3g}")
        assert band == 0, "a fixture unit lies within the tolerance band of THETAE: change the input"
        data["ratio_tol"] = np.float64(tol)
        data["ratio_band_units"] = np.int32(band)
        reached = purposes(results, data)
        for name, ok in reached.items():
            print(f"{'reached' if ok else 'NOT REACHED'}: {name}")
        assert all(reached.values()), "an input does not reach the point it was chosen for"
        for k, make in AM.HAND_CASES.items():
            c = make()
            r = G.run_hand(exe, tmp, c)
            rc = G.run_hand(cov, tmp, c)
            assert all(np.array_equal(rc[n], r[n]) for n in r)
            f = AM.final_seg(**c)
            for name, v in r.items():
                assert np.array_equal(f[name], v.astype(np.float32)), f"hand-made {k}: the model's {name} differs"
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: mask units {int(r['mask'].sum())}, -1 units {int((r['grp_final'] < 0).sum())}")
        executable, missed = G.uncovered(os.path.dirname(cov), 1146, 1494)
        print(f"HuWang.cpp:1146-1494: {executable} executable lines, {len(missed)} never executed")
        assert not missed, f"lines never executed by the fixture's inputs: {missed}"
        executable, missed = G.uncovered(os.path.dirname(cov), 1553, 1677)
        print(f"HuWang.cpp:1553-1677: {executable} executable lines, never executed: " + ", ".join(f"{n} ({G.UNREACHABLE.get(n, '?')})" for n in missed))
        assert set(missed) == set(G.UNREACHABLE), f"expected exactly the unreachable lines {sorted(G.UNREACHABLE)}, got {missed}"
    data["max_taps"] = np.int32(max(AM.filter_length(mp) for mp in AM.reachable_mean_pitches()) + 1)
    G.GP.save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
