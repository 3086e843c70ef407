#!/usr/bin/env python3
"""tools/gen_hw64_resynth_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw64_resynth_golden.npz: what THE REFERENCE ITSELF makes of a few signals and masks in resynthesis
(function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1498-1549) when it is compiled against the 64-band header
resyth_64sub_IBM/cpp/HuWang.h (SAMPLING_FREQUENCY 16000, NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320): data only, no reference
source.  Runs only where the reference tree exists:

    python tools/gen_hw64_resynth_golden.py <reference tree>

The procedure is tools/gen_hw25_resynth_golden.py's, and so is the code: this file loads a second instance of that module at 64
channels and a hop of 160, as tools/gen_hw64_am_golden.py does with the AM tool.  Only the build is restated: HuWang.cpp is
copied UNMODIFIED to a temporary directory outside the repository and compiled there against the 64-band header; that tool's
driver (our own code, which only CALLS the reference) is linked with it.  The driver takes `resynth`'s exact floats from the
first pointer handed to operator delete during resynthesis, and the text file is cross-checked within 5e-7 in decimal
arithmetic.

  * audio cases (tests/hw64_am_model.AUDIO_CASES): createIBM (x), then resynthesis (its mask, fp); the mask must be the one
    tests/golden/hw64_am_golden.npz holds;
  * hand-made masks (tests/hw64_resynth_model: HAND_INPUTS x HAND_MASKS): AudiPeriph (), then resynthesis (the mask, fp).

On this bank WINDOW = 2 * OFFSET and the reference stays inside weight[] whatever the mask: masks whose last row is set are
cases for the reference.  The bounds condition is asserted all the same, by the tool (160 f + 159 < L for every set frame f)
and by the driver on createIBM's mask (exit 6).

Per case k (a_<input> or h_<input>_<mask>): out_k float32 [L], mask_k int8 [F][64], text_crc_k uint32 (CRC32 of the text file)
and, for TEXT_CASES, text_k int8 (the file's bytes).  Asserted before anything is written: the numpy model (tests/
hw64_resynth_model.py, which holds no channel, hop or window literal) gives the same floats bit for bit on every case; a
--coverage build executes every executable line of HuWang.cpp:1498-1549; the fixture stays under 1 MiB.
"""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hw64_am_model as AM  # noqa: E402
from tests import hw64_model as M  # noqa: E402
from tests import hw64_resynth_model as RM  # noqa: E402

PATH = RM.GOLDEN
SRC = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test", "HuWang.cpp")
INC = os.path.join("resyth_64sub_IBM", "cpp")
NCH, HOP = RM.NCH, RM.HOP


def build(ref_root, tmp, name, extra):
    """HuWang.cpp unmodified, compiled against the 64-band header, and the driver into one program -> its path"""
    src, inc = os.path.join(ref_root, SRC), os.path.join(ref_root, INC)
    if not os.path.exists(src) or not os.path.exists(os.path.join(inc, "HuWang.h")):
        raise SystemExit(f"{src} or {inc}/HuWang.h is missing: this tool runs only where the reference tree exists")
    work = os.path.join(tmp, name)
    os.makedirs(work)
    shutil.copy(src, os.path.join(work, "HuWang.cpp"))
    with open(os.path.join(work, "driver.cpp"), "w") as fh:
        fh.write(G.DRIVER)
    exe = os.path.join(work, "hw64_resynth_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-fPIC", "-w", *extra, "-I", inc]
    subprocess.check_call(flags + ["-c", "HuWang.cpp", "-o", "HuWang.o"], cwd=work)
    subprocess.check_call(flags + ["-c", "driver.cpp", "-o", "driver.o"], cwd=work)
    subprocess.check_call(["g++", *extra, "driver.o", "HuWang.o", "-o", exe], cwd=work)
    return exe


def _second_instance():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gen_hw25_resynth_golden.py")
    spec = importlib.util.spec_from_file_location("gen_hw25_resynth_golden_at_64_bands", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.NCH, m.HOP, m.AM, m.M, m.RM, m.PATH, m.build = NCH, HOP, AM, M, RM, PATH, build
    return m


G = _second_instance()


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/gen_hw64_resynth_golden.py <reference tree>")
    assert (RM.HOP, RM.WINDOW) == (160, 320) and RM.WINDOW - RM.HOP - 1 == 159, "the bounds condition is 160 f + 159 < L"
    G.main()
    # tests/hw64_model.load_golden reads every hw64_*.npz of the golden directory and takes a uint8 array for the byte planes of
    # a float array: the text files are kept as int8 (the same bytes)
    with np.load(PATH) as z:
        data = {k: (z[k].view(np.int8) if k.startswith("text_") and z[k].dtype == np.uint8 else z[k]) for k in z.files}
    G.GP.save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"


if __name__ == "__main__":
    main()
