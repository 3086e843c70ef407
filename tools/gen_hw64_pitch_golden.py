#!/usr/bin/env python3
"""tools/gen_hw64_pitch_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw64_pitch_golden.npz: what THE REFERENCE ITSELF makes of a few signals in initGroup and pitchDtm
(function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:79-87 of createIBM, the functions of :466-1142) at 16 kHz on
the 64-channel bank: data only, no reference source.  Runs only where the reference tree exists:

    python tools/gen_hw64_pitch_golden.py <reference tree>

It follows tools/gen_hw25_pitch_golden.py and uses its driver, its reader of the driver's output, its gcov reader and its
writer, as a second instance of that module at 64 channels, 201 delays and a hop of 160.  As tools/gen_hw64_golden.py does,
HuWang.cpp is copied UNMODIFIED into a temporary directory outside the repository, where its `#include "HuWang.h"` does not
find the 8 kHz header that sits beside the original, and compiled (g++ -O2 -ffp-contract=off) with -I resyth_64sub_IBM/cpp,
whose own NoiseSupExports.h supplies `struct mask`.

Inputs (tests/hw64_pitch_model.py, the same functions the tests call): the audio cases AUDIO_CASES, 62 to 87 frames each, and
the hand-made array cases HAND_CASES at [F][64][201], handed to the driver with a zero `cross` (nothing of this stage reads it
on this bank).  Per audio case k: x_k, acfcrc_k (CRC32 of the reference's corrHc acf bytes, [F][64][201] floats), nseg_k,
pitch_k and the five pitch stages [F] int32, lrframe_k, grp_k and the two grp stages [F][64] int8, pratio_k [F][64] float32.
The hand-made cases: the same without x and the CRC.

Before anything is written the tool asserts, and prints:
  * every input has 1..400 segments and no uninitialised chan_mark read (the driver's refusals 3 and 4);
  * pitchDtm itself gives the same bytes as its steps called one by one;
  * a --coverage build executes every executable line of HuWang.cpp:466-1142;
  * some input separates lFrame / rFrame before and after findPitch's vote;
  * the model (tests/hw64_pitch_model.py) equals the reference on every input with the Developes' four bounds at 40, and for
    each of the four bounds some input's pitch differs from the reference's when the model moves that bound alone to 64;
  * the same four against THE REFERENCE with `chan<40` patched to `chan<64` in the temporary copy: it equals the model at 64
    and differs from the unpatched build on the hand-made cases made for it.
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
from tests import hw64_pitch_model as PM  # noqa: E402

PATH = PM.GOLDEN
SRC = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test", "HuWang.cpp")
INC = os.path.join("resyth_64sub_IBM", "cpp")
COMPARED = ("pitch",) + PM.PITCH_STAGES + ("grp",) + PM.GRP_STAGES + ("pratio",)


def _second_instance():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen_hw25_pitch_golden.py")
    spec = importlib.util.spec_from_file_location("gen_hw25_pitch_golden_at_64_bands", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.NCH, m.NDEL, m.HOP, m.PM = PM.NCH, PM.NDEL, PM.HOP, PM
    return m


G = _second_instance()


def build(ref_root, tmp, name, extra, patch=False):
    src, inc = os.path.join(ref_root, SRC), os.path.join(ref_root, INC)
    if not os.path.exists(src) or not os.path.exists(os.path.join(inc, "HuWang.h")):
        raise SystemExit(f"{src} or {inc}/HuWang.h is missing: this tool runs only where the reference tree exists")
    work = os.path.join(tmp, name)
    os.makedirs(work)
    if patch:  # the port that replaces 25 by 64 throughout, for the separation check alone
        with open(src, errors="surrogateescape") as fh:
            text = fh.read()
        assert text.count("chan<40") == 4
        with open(os.path.join(work, "HuWang.cpp"), "w", errors="surrogateescape") as fh:
            fh.write(text.replace("chan<40", "chan<64"))
    else:
        shutil.copy(src, os.path.join(work, "HuWang.cpp"))
    with open(os.path.join(work, "driver.cpp"), "w") as fh:
        fh.write(G.DRIVER)
    exe = os.path.join(work, "hw64_pitch_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-w", *extra, "-I", inc]
    for unit in ("HuWang", "driver"):
        subprocess.check_call(flags + ["-c", unit + ".cpp", "-o", unit + ".o"], cwd=work)
    subprocess.check_call(["g++", *extra, "driver.o", "HuWang.o", "-o", exe], cwd=work)
    return exe


def arrays_of(k):
    acf, pratio, mark = PM.hand_inputs(k)
    return acf, pratio, mark, np.zeros_like(pratio)


def model_differs(r, got):
    return [n for n in COMPARED if np.asarray(got[n]).astype(np.float32).tobytes() != np.asarray(r[n]).astype(np.float32).tobytes()]


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/gen_hw64_pitch_golden.py <reference tree>")
    ref_root = sys.argv[1]
    data, results = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp, "plain", [])
        cov = build(ref_root, tmp, "cov", ["--coverage"])
        at64 = build(ref_root, tmp, "at64", [], patch=True)
        xs = PM.audio_inputs()
        for k in PM.AUDIO_CASES:
            r = G.run(exe, tmp, x=xs[k])
            if isinstance(r, int):
                raise SystemExit(f"input {k}: the driver refused it ({r})")
            G.both(exe, cov, tmp, r, x=xs[k])
            data[f"x_{k}"] = xs[k]
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"input {k}: L {len(xs[k])}, frames {len(xs[k]) // PM.HOP}, segments {int(r['nseg'])}, "
                  f"voiced frames {int((r['pitch'] > 0).sum())}, + / - units {int((r['grp'] > 0).sum())} / {int((r['grp'] < 0).sum())}, "
                  f"+ units in channels >= 40: {int((r['grp'][:, 40:] > 0).sum())}, frames changed by leftDevelope / rightDevelope: "
                  f"{int((r['pitch_left'] != r['pitch_check']).sum())} / {int((r['pitch_right'] != r['pitch_left']).sum())}")
        for k in PM.HAND_CASES:
            arrays = arrays_of(k)
            r = G.run(exe, tmp, arrays=arrays)
            assert not isinstance(r, int), f"hand-made {k}: the driver refused it ({r})"
            G.both(exe, cov, tmp, r, arrays=arrays)
            r.pop("acfcrc")
            results[k] = r
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: segments {int(r['nseg'])}, lFrame / rFrame {r['lrframe'].tolist()}, pitch {r['pitch'].tolist()}")
            got = PM.pitch_stage(*arrays[:3])
            assert got["status"] == int(r["nseg"]) and not model_differs(r, got), f"hand-made {k}: the model differs from the reference"
        # findPitch takes lFrame / rFrame before its vote zeroes Pitch: at least one input must tell the two apart
        apart = []
        for k in PM.AUDIO_CASES + tuple(PM.HAND_CASES):
            voiced = np.flatnonzero(data[f"pitch_find2_{k}"] > 0)
            after = [int(voiced[0]), int(voiced[-1])] if len(voiced) else [len(data[f"pitch_find2_{k}"]), 0]
            if after != data[f"lrframe_{k}"].tolist():
                apart.append(k)
        print(f"lFrame / rFrame differ from the first / last frame that keeps its pitch on: {apart}")
        assert apart, "no fixture input separates findPitch's lFrame / rFrame from the frames that keep their pitch"
        # forty channels, not sixty-four, at each of the Developes' four bounds
        for bound, (k, frame, at40, at_all) in PM.SEPARATES.items():
            arrays = arrays_of(k)
            r, moved = results[k], PM.pitch_stage(*arrays[:3], bounds={bound: PM.NCH})
            assert int(r["pitch"][frame]) == at40 and int(moved["pitch"][frame]) == at_all and at40 != at_all, (bound, k)
            stage = "pitch_left" if bound.startswith("left") else "pitch_right"
            assert stage in model_differs(r, moved), f"{bound}: moving it to 64 does not change {stage} of {k}"
            q = G.run(at64, tmp, arrays=arrays)
            assert not isinstance(q, int) and not model_differs(q, PM.pitch_stage(*arrays[:3], bounds=PM.ALL_64)), (bound, k)
            assert int(q["pitch"][frame]) == at_all
            print(f"{bound}: hand-made {k}, Pitch[{frame}] = {at40} with the reference's chan<40, {at_all} with chan<64 "
                  f"(the model with this bound moved, and the reference patched)")
        executable, missed = G.uncovered(os.path.dirname(cov))
        print(f"HuWang.cpp:{G.FIRST_LINE}-{G.LAST_LINE}: {executable} executable lines, {len(missed)} never executed")
        assert not missed, f"lines never executed by the fixture's inputs: {missed}"
    G.save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
