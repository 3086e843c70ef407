#!/usr/bin/env python3
"""tools/gen_hw25_resynth_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw25_resynth_golden.npz: what THE REFERENCE ITSELF makes of a few signals and masks in resynthesis
(function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1498-1549): data only, no reference source.  Runs only where
the reference tree exists:

    python tools/gen_hw25_resynth_golden.py <reference tree>

The reference's HuWang.cpp is compiled UNMODIFIED (g++ -O2 -ffp-contract=off -fPIC) in a temporary directory outside the
repository, with the two-line header of tools/gen_hw25_pitch_golden.py for `struct mask`.  A driver of our own only CALLS it:

  * audio cases (tests/hw25_resynth_model.AUDIO_CASES): createIBM (x), then resynthesis (its mask, fp);
  * hand-made masks (HAND_INPUTS x HAND_MASKS): the driver sets Input, sigLength and numFrame, allocates gOut / hOut, calls
    AudiPeriph () and then resynthesis (the mask, fp).  The marks are 0 / 1 (`soft` goes in as mark > 0).

The exact floats are taken without touching the reference: the driver replaces operator delete (createIBM deletes one pointer
past gOut[], so every block is kept anyway), and the first pointer handed to it during resynthesis is `resynth`, still intact.
The text file that resynthesis writes is kept as a cross-check: every parsed line must lie within 5e-7 of the float.

The reference writes weight[] past its end when a unit of the last frames is set and L % 80 < 40 (tests/hw25_resynth_model.py).
Before the reference is called the tool asserts, for every case, that every channel's largest set frame f has 80 f + 119 < L,
and refuses otherwise; the driver checks the same on createIBM's mask before it calls resynthesis (exit 6).

Per case k (a_<input> or h_<input>_<mask>): out_k float32 [L], mask_k int8 [F][25], text_crc_k uint32 (CRC32 of the text file)
and, for TEXT_CASES, text_k uint8 (the file).  The tool asserts that the numpy model gives the same floats bit for bit.

A second build with --coverage runs every input; gcov must show every executable line of HuWang.cpp:1498-1549 executed.
"""
import os
import subprocess
import sys
import tempfile
import zlib
from decimal import Decimal

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hw25_am_model as AM  # noqa: E402
from tests import hw25_model as M  # noqa: E402
from tests import hw25_resynth_model as RM  # noqa: E402
from tools import gen_hw25_am_golden as GA  # noqa: E402
from tools import gen_hw25_pitch_golden as GP  # noqa: E402

PATH = RM.GOLDEN
NCH, HOP = 25, 80

DRIVER = r"""
#include <new>
#include "HuWang.h"
extern long sigLength;
extern float Input[], *gOut[], *hOut[];
extern int numFrame;
void AudiPeriph();
void resynthesis(mask *m, FILE *fp);

static bool watching;
static void *firstDeleted;
static void seen(void *p) { if (watching && !firstDeleted) firstDeleted = p; }
/* every block is kept: createIBM deletes one pointer past gOut[], and resynth must stay readable after its delete */
void operator delete(void *p) noexcept { seen(p); }
void operator delete(void *p, std::size_t) noexcept { seen(p); }
void operator delete[](void *p) noexcept { seen(p); }
void operator delete[](void *p, std::size_t) noexcept { seen(p); }

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb"), *ft = fopen(argv[3], "w");
    if (!fi || !fo || !ft) return 2;
    const char mode = argv[4][0];
    int len;
    if (fread(&len, sizeof len, 1, fi) != 1 || len < 0 || len > MAX_SIG_LENGTH) return 2;
    static float x[MAX_SIG_LENGTH];
    if ((int)fread(x, sizeof(float), len, fi) != len) return 2;
    const int frames = len / OFFSET;
    mask *m = new mask[frames + 1];
    if (mode == 'a') {
        createIBM(x, len, m);
    } else {
        for (int f = 0; f < frames; f++) if (fread(m[f].mark, sizeof m[f].mark, 1, fi) != 1) return 2;
        sigLength = len;
        numFrame = frames;
        for (int i = 0; i < len; i++) Input[i] = x[i];
        for (int c = 0; c < NUMBER_CHANNEL; c++) {
            gOut[c] = new float[len];
            hOut[c] = new float[len];
        }
        AudiPeriph();
    }
    for (int f = 0; f < frames; f++)
        for (int c = 0; c < NUMBER_CHANNEL; c++)
            if (m[f].mark[c] > 0 && !(OFFSET * f + (WINDOW - OFFSET - 1) < len)) return 6;
    watching = true;
    resynthesis(m, ft);
    watching = false;
    if (!firstDeleted) return 7;
    for (int f = 0; f < frames; f++) if (fwrite(m[f].mark, sizeof m[f].mark, 1, fo) != 1) return 2;
    if ((int)fwrite(firstDeleted, sizeof(float), len, fo) != len) return 2;
    fclose(fo);
    fclose(ft);
    return 0;
}
"""


def build(ref_root, tmp, name, extra):
    """HuWang.cpp unmodified and the driver into one program -> its path"""
    src = os.path.join(ref_root, GP.REL, "HuWang.cpp")
    if not os.path.exists(src):
        raise SystemExit(f"{src} is missing: this tool runs only where the reference tree exists")
    work = os.path.join(tmp, name)
    inc = os.path.join(work, "inc")
    os.makedirs(inc)
    with open(os.path.join(inc, "..\\aurora_etsi\\NoiseSupExports.h"), "w") as fh:
        fh.write(GP.HEADER)
    with open(os.path.join(work, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(work, "hw25_resynth_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-fPIC", "-w", *extra, "-I", inc, "-I", os.path.join(ref_root, GP.REL)]
    subprocess.check_call(flags + ["-c", src, "-o", os.path.join(work, "HuWang.o")], cwd=work)
    subprocess.check_call(flags + ["-c", os.path.join(work, "driver.cpp"), "-o", os.path.join(work, "driver.o")], cwd=work)
    subprocess.check_call(["g++", *extra, os.path.join(work, "driver.o"), os.path.join(work, "HuWang.o"), "-o", exe], cwd=work)
    return exe


def run(exe, tmp, x, mask, mode):
    """one case through the driver -> (the mask resynthesis saw, resynth's floats, the text file's bytes)"""
    L, nfr = len(x), len(x) // HOP
    assert RM.in_bounds(mask > 0, L), "a set unit would make the reference write past weight[]: not a case for the reference"
    assert np.isin(mask, (0, 1)).all()
    fin, fout, ftxt = (os.path.join(tmp, n) for n in ("in.bin", "out.bin", "out.txt"))
    with open(fin, "wb") as fh:
        fh.write(np.int32(L).tobytes() + x.astype(np.float32).tobytes() + (mask.astype(np.float32).tobytes() if mode == "h" else b""))
    rc = subprocess.call([exe, fin, fout, ftxt, mode], stdout=subprocess.DEVNULL, cwd=os.path.dirname(exe))
    if rc:
        raise SystemExit(f"the driver failed with {rc} (6: a set unit out of bounds; 7: resynthesis deleted nothing)")
    r = GA.Reader(fout)
    seen, out = r.take(np.float32, nfr, NCH), r.take(np.float32, L)
    r.done()
    with open(ftxt, "rb") as fh:
        txt = fh.read()
    lines = txt.split(b"\n")
    assert len(lines) == L + 1 and lines[-1] == b"", "the text file does not hold one line per sample"
    # in exact decimal arithmetic: a float that ends in ...5 at the seventh decimal lies exactly 5e-7 from its line, and a
    # double difference would round that up
    worst = max(abs(Decimal(s.decode()) - Decimal(float(v))) for s, v in zip(lines[:-1], out))
    assert worst <= Decimal("5e-7"), f"the text file is not the floats: a line differs by {worst}"
    return seen, out, txt


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/gen_hw25_resynth_golden.py <reference tree>")
    ref_root = sys.argv[1]
    data = {}
    am_golden = AM.load_golden()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp, "plain", [])
        cov = build(ref_root, tmp, "cov", ["--coverage"])
        for k, (x, mask) in RM.reference_cases(am_golden).items():
            mode = k[0]
            seen, out, txt = run(exe, tmp, x, mask, mode)
            seen_c, out_c, txt_c = run(cov, tmp, x, mask, mode)
            assert out.tobytes() == out_c.tobytes() and txt == txt_c and np.array_equal(seen, seen_c), f"{k}: the coverage build differs"
            assert np.array_equal(seen, mask), f"{k}: the mask resynthesis saw is not the expected one"
            name = k.split("_")[1]
            model = RM.resynth_input(name, mask)
            assert M.same_bits(model, out), f"{k}: the numpy model differs from the reference"
            assert RM.text(out) == txt, f"{k}: the model's text form differs from the reference's file"
            data[f"out_{k}"] = out
            data[f"mask_{k}"] = mask.astype(np.int8)
            data[f"text_crc_{k}"] = np.uint32(zlib.crc32(txt) & 0xFFFFFFFF)
            if k in RM.TEXT_CASES:
                data[f"text_{k}"] = np.frombuffer(txt, np.uint8)
            print(f"{k}: L {len(x)}, set units {int(mask.sum())}, largest |sample| {float(np.abs(out).max()):.6g}, model equal")
        GP.FIRST_LINE, GP.LAST_LINE = 1498, 1549
        executable, missed = GP.uncovered(os.path.dirname(cov))
        print(f"HuWang.cpp:1498-1549: {executable} executable lines, {len(missed)} never executed")
        assert executable > 20 and not missed, f"lines never executed by the fixture's inputs: {missed}"
    GP.save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
