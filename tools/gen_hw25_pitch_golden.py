#!/usr/bin/env python3
"""tools/gen_hw25_pitch_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw25_pitch_golden.npz: what THE REFERENCE ITSELF makes of a few signals in initGroup and pitchDtm
(function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:79-87 of createIBM, the functions of :466-1142): data only, no
reference source.  Runs only where the reference tree exists:

    python tools/gen_hw25_pitch_golden.py <reference tree>

As tools/gen_hw25_golden.py does, the reference's HuWang.cpp is compiled UNMODIFIED (g++ -O2 -ffp-contract=off) in a temporary
directory outside the repository, with a two-line header of our own for `struct mask` and a driver of our own.  The driver

  * audio cases: runs the front half and the labelling of createIBM:74-76, counts the segments on a copy of the marks and
    refuses an input with none or more than 400 (exit 3), calls initGroup, then pitchDtm's steps one by one in its order
    (findPitch, timeCrn, reGroup (THETAP), findPitch, checkPitch, leftDevelope, rightDevelope, linearEstimate, timeCrn,
    reGroup (THETAT); run a second time it calls pitchDtm itself, and the tool checks that both give the same bytes), dumping Pitch / Grp after the steps named in tests/hw25_pitch_model.py; between checkPitch and
    leftDevelope it refuses an input on which a Develope would read chan_mark uninitialised (exit 4);
  * the hand-made cases: takes acf / pRatio / mark / cross as arrays (tests/hw25_pitch_model.py::HAND_CASES, the same
    functions the tests call) straight into corrHc / Grp and runs the same steps.  h reaches `number == 0` in both Developes;
    v has a frame that loses findPitch's vote outside the outermost frame that keeps its pitch (findPitch takes lFrame /
    rFrame BEFORE the vote: the tool asserts that some input tells the two apart); x has a cross value that decides a bit.

The number2 loops of leftDevelope and rightDevelope run over forty channels on this bank of 25, so they read the frame's cross
and pRatio and the NEXT frame's acf and marks as channels 25..39 (the arrays are contiguous).  On the last frame that is one
entry past the frames: the driver allocates it and zeroes it, which is the "not counted" of include/sea_mi355x.h.

Per audio case k: x_k, acfcrc_k (CRC32 of the reference's corrHc acf bytes, [F][25][101] floats), nseg_k, pitch_k and the five
pitch stages [F] int32, lrframe_k (lFrame, rFrame of the second findPitch), grp_k and the two grp stages [F][25] int8, pratio_k
[F][25] float32.  The hand-made cases: the same without x and the CRC.

A second build of the same driver with --coverage runs every fixture input; gcov must then show every executable line of
HuWang.cpp:466-1142 executed, or the tool fails and prints the lines that were not.
"""
import io
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hw25_pitch_model as PM  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "hw25_pitch_golden.npz")
REL = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test")
NCH, NDEL, HOP = 25, 101, 80
FIRST_LINE, LAST_LINE = 466, 1142

HEADER = "#define NUMBER_CHANNEL 25\nstruct mask { float mark[NUMBER_CHANNEL]; };\n"

DRIVER = r"""
#include "HuWang.h"
extern long sigLength;
extern float Input[], *gOut[], *hOut[], *hEv[];
extern int numFrame;
extern corrLgm *corrHc, *corrEv;
extern int *Pitch;
extern int *Unit[2];
extern int segMark[];
extern int numSegment;

static FILE *fo;
static void put(const void *p, size_t n) { if (fwrite(p, 1, n, fo) != n) exit(2); }
static void putPitch() { put(Pitch, sizeof(int) * numFrame); }
static void putGrp(mask *Grp) { for (int f = 0; f < numFrame; f++) put(Grp[f].mark, sizeof Grp[f].mark); }

/* the number of segments of the marks, on a copy and without the reference's 400-entry array */
static long countSegments(mask *Grp)
{
    mask *m = new mask[numFrame + 1];
    int *u[2] = {new int[long(numFrame + 1) * NUMBER_CHANNEL], new int[long(numFrame + 1) * NUMBER_CHANNEL]};
    for (int f = 0; f < numFrame; f++) m[f] = Grp[f];
    long segs = 0, numUnit = 0;
    for (int f = 1; f < numFrame - 1; f++)
        for (int c = 0; c < NUMBER_CHANNEL; c++)
            if (m[f].mark[c] && m[f - 1].mark[c] && m[f + 1].mark[c]) {
                u[0][numUnit] = c;
                u[1][numUnit] = f;
                m[f].mark[c] = 0;
                long active = numUnit++;
                while (active < numUnit) search(m, numFrame, u, active++, numUnit);
                segs++;
            }
    delete[] m;
    delete[] u[0];
    delete[] u[1];
    return segs;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const bool audio = argv[3][0] == 'a';
    FILE *fi = fopen(argv[1], "rb");
    fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    mask *Grp;
    if (audio) {
        sigLength = (long)fread(Input, sizeof(float), MAX_SIG_LENGTH, fi);
        numFrame = sigLength / OFFSET;
        for (int c = 0; c < NUMBER_CHANNEL; c++) {
            gOut[c] = new float[sigLength];
            hOut[c] = new float[sigLength];
            hEv[c] = new float[sigLength];
        }
        corrHc = new corrLgm[numFrame + 1];
        corrEv = new corrLgm[numFrame + 1];
        Pitch = new int[numFrame + 1];
        Grp = new mask[numFrame + 1];
        memset(&corrHc[numFrame], 0, sizeof(corrLgm)); /* the Developes' 40-channel loops read one entry past the frames */
        memset(&Grp[numFrame], 0, sizeof(mask));
        AudiPeriph();
        lowPass();
        computeACF();
        crossCorr();
        globalPitch();
        timeCrn(corrHc);
        for (int f = 0; f < numFrame; f++)
            for (int c = 0; c < NUMBER_CHANNEL; c++) {
                const bool coherent = corrHc[f].cross[c] > THETAC;
                const bool loud = corrHc[f].acf[c][0] > (THETAA * THETAA);
                Grp[f].mark[c] = (coherent && loud) ? 1.0f : 0.0f;
            }
    } else {
        if (fread(&numFrame, sizeof(int), 1, fi) != 1) return 2;
        corrHc = new corrLgm[numFrame + 1];
        Pitch = new int[numFrame + 1];
        Grp = new mask[numFrame + 1];
        memset(corrHc, 0, sizeof(corrLgm) * (numFrame + 1));
        memset(&Grp[numFrame], 0, sizeof(mask));
        for (int f = 0; f < numFrame; f++) {
            Pitch[f] = 0;
            if (fread(corrHc[f].acf, sizeof corrHc[f].acf, 1, fi) != 1) return 2;
        }
        for (int f = 0; f < numFrame; f++)
            if (fread(corrHc[f].pRatio, sizeof corrHc[f].pRatio, 1, fi) != 1) return 2;
        for (int f = 0; f < numFrame; f++)
            if (fread(Grp[f].mark, sizeof Grp[f].mark, 1, fi) != 1) return 2;
        for (int f = 0; f < numFrame; f++)
            if (fread(corrHc[f].cross, sizeof corrHc[f].cross, 1, fi) != 1) return 2;
    }
    const long segs = countSegments(Grp);
    if (segs < 1 || segs > MAX_NUMBER_SEGMENT) return 3;
    for (int f = 0; f < numFrame; f++) put(corrHc[f].acf, sizeof corrHc[f].acf);

    Unit[0] = new int[long(numFrame) * NUMBER_CHANNEL];
    Unit[1] = new int[long(numFrame) * NUMBER_CHANNEL];
    initGroup(Grp);
    put(&numSegment, sizeof(int));
    putGrp(Grp);

    if (argv[3][1] == 'w') { /* pitchDtm itself: the tool compares its final arrays with the stepwise run's */
        pitchDtm(Grp);
        putPitch();
        putGrp(Grp);
        for (int f = 0; f < numFrame; f++) put(corrHc[f].pRatio, sizeof corrHc[f].pRatio);
        fclose(fo);
        return 0;
    }
    int lFrame, rFrame, sStreak, eStreak;
    int *buffer = new int[numFrame + 1];
    findPitch(lFrame, rFrame, Grp);
    putPitch();
    timeCrn(corrHc);
    reGroup(THETAP, Grp);
    putGrp(Grp);
    findPitch(lFrame, rFrame, Grp);
    putPitch();
    put(&lFrame, sizeof(int)); /* taken from sumAuto's result before findPitch's vote zeroes Pitch */
    put(&rFrame, sizeof(int));
    checkPitch(Pitch, buffer, numFrame, lFrame, rFrame, sStreak, eStreak);
    putPitch();
    if ((sStreak - 1 >= lFrame && Pitch[sStreak] == 0) || (eStreak + 1 <= rFrame && Pitch[eStreak] == 0)) return 4;
    leftDevelope(corrHc, Grp, Pitch, buffer, sStreak, lFrame);
    putPitch();
    rightDevelope(corrHc, Grp, Pitch, buffer, eStreak, rFrame);
    putPitch();
    linearEstimate(Pitch, lFrame, rFrame);
    timeCrn(corrHc);
    reGroup(THETAT, Grp);
    putPitch();
    putGrp(Grp);
    for (int f = 0; f < numFrame; f++) put(corrHc[f].pRatio, sizeof corrHc[f].pRatio);
    fclose(fo);
    return 0;
}
"""


def build(ref_root, tmp, name, extra):
    src = os.path.join(ref_root, REL, "HuWang.cpp")
    if not os.path.exists(src):
        raise SystemExit(f"{src} is missing: this tool runs only where the reference tree exists")
    work = os.path.join(tmp, name)
    inc = os.path.join(work, "inc")
    os.makedirs(inc)
    with open(os.path.join(inc, "..\\aurora_etsi\\NoiseSupExports.h"), "w") as fh:
        fh.write(HEADER)
    with open(os.path.join(work, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(work, "hw25_pitch_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-w", *extra, "-I", inc, "-I", os.path.join(ref_root, REL)]
    subprocess.check_call(flags + ["-c", src, "-o", os.path.join(work, "HuWang.o")], cwd=work)
    subprocess.check_call(flags + ["-c", os.path.join(work, "driver.cpp"), "-o", os.path.join(work, "driver.o")], cwd=work)
    subprocess.check_call(["g++", *extra, os.path.join(work, "driver.o"), os.path.join(work, "HuWang.o"), "-o", exe], cwd=work)
    return exe


def run(exe, tmp, x=None, arrays=None, whole=False):
    """one input through the driver -> dict, or the driver's refusal as an int (3: segment count, 4: chan_mark unset)"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    if x is not None:
        x.tofile(fin)
        nfr = len(x) // HOP
    else:
        acf, pratio, mark, cross = arrays
        nfr = acf.shape[0]
        with open(fin, "wb") as fh:
            fh.write(np.int32(nfr).tobytes() + acf.tobytes() + pratio.tobytes() + mark.tobytes() + cross.tobytes())
    rc = subprocess.call([exe, fin, fout, ("a" if x is not None else "h") + ("w" if whole else "s")], stdout=subprocess.DEVNULL, cwd=os.path.dirname(exe))
    if rc in (3, 4):
        return rc
    if rc:
        raise SystemExit(f"the driver failed with {rc}")
    raw = np.fromfile(fout, np.uint8)
    pos = 0

    def take(dtype, *shape):
        nonlocal pos
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out = raw[pos:pos + n].view(dtype).reshape(shape).copy()
        pos += n
        return out

    def grp():
        g = take(np.float32, nfr, NCH)
        assert np.isin(g, (-1, 0, 1)).all()
        return g.astype(np.int8)

    r = {"acfcrc": np.uint32(PM.crc32(take(np.float32, nfr, NCH, NDEL)))}
    r["nseg"] = np.int32(take(np.int32, 1)[0])
    r["grp_init"] = grp()
    if whole:
        r.update(pitch=take(np.int32, nfr), grp=grp(), pratio=take(np.float32, nfr, NCH))
        assert pos == len(raw)
        return r
    r["pitch_find1"] = take(np.int32, nfr)
    r["grp_thetap"] = grp()
    r["pitch_find2"] = take(np.int32, nfr)
    r["lrframe"] = take(np.int32, 2)
    for k in ("pitch_check", "pitch_left", "pitch_right", "pitch"):
        r[k] = take(np.int32, nfr)
    r["grp"] = grp()
    r["pratio"] = take(np.float32, nfr, NCH)
    assert pos == len(raw), "the driver wrote more than was read"
    return r


def both(exe, cov, tmp, r, **kw):
    """the coverage build on the same input, stepwise and through pitchDtm itself: the same final arrays as `r` every time"""
    for which, whole in ((cov, False), (cov, True), (exe, True)):
        w = run(which, tmp, whole=whole, **kw)
        assert not isinstance(w, int)
        for name in ("nseg", "grp_init", "pitch", "grp", "pratio"):
            assert np.asarray(w[name]).tobytes() == np.asarray(r[name]).tobytes(), f"{name}: pitchDtm and its steps differ"


def uncovered(work):
    """the executable lines of HuWang.cpp:466-1142 that the coverage build never ran"""
    subprocess.check_call(["gcov", "-o", work, "HuWang.cpp"], cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = os.path.join(work, "HuWang.cpp.gcov")
    missed, executable = [], 0
    with open(path, errors="replace") as fh:
        for line in fh:
            m = re.match(r"\s*([^:]+):\s*(\d+):", line)
            if not m or not FIRST_LINE <= int(m.group(2)) <= LAST_LINE:
                continue
            count = m.group(1).strip()
            if count == "-":
                continue
            executable += 1
            if count.startswith("#") or count.startswith("="):
                missed.append(int(m.group(2)))
    return executable, missed


def save(path, data):
    """an .npz with fixed member times, so that the same data gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, value in data.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp, "plain", [])
        cov = build(ref_root, tmp, "cov", ["--coverage"])
        xs = PM.audio_inputs()
        assert run(exe, tmp, x=xs["s"]) == 3, "input s must have no segment on the reference"
        for k in PM.AUDIO_CASES:
            r = run(exe, tmp, x=xs[k])
            if isinstance(r, int):
                raise SystemExit(f"input {k}: the driver refused it ({r})")
            both(exe, cov, tmp, r, x=xs[k])
            data[f"x_{k}"] = xs[k]
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"input {k}: L {len(xs[k])}, frames {len(xs[k]) // HOP}, segments {int(r['nseg'])}, "
                  f"voiced frames {int((r['pitch'] > 0).sum())}, + / - units {int((r['grp'] > 0).sum())} / {int((r['grp'] < 0).sum())}")
        for k in PM.HAND_CASES:
            arrays = PM.hand_inputs(k)
            r = run(exe, tmp, arrays=arrays)
            assert not isinstance(r, int), f"hand-made {k}: the driver refused it ({r})"
            both(exe, cov, tmp, r, arrays=arrays)
            r.pop("acfcrc")
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: segments {int(r['nseg'])}, lFrame / rFrame {r['lrframe'].tolist()}, pitch {r['pitch'].tolist()}")
        # findPitch takes lFrame / rFrame before its vote zeroes Pitch: at least one input must tell the two apart
        apart = []
        for k in PM.AUDIO_CASES + tuple(PM.HAND_CASES):
            voiced = np.flatnonzero(data[f"pitch_find2_{k}"] > 0)
            after = [int(voiced[0]), int(voiced[-1])] if len(voiced) else [len(data[f"pitch_find2_{k}"]), 0]
            if after != data[f"lrframe_{k}"].tolist():
                apart.append(k)
        print(f"lFrame / rFrame differ from the first / last frame that keeps its pitch on: {apart}")
        assert apart, "no fixture input separates findPitch's lFrame / rFrame from the frames that keep their pitch"
        executable, missed = uncovered(os.path.dirname(cov))
        print(f"HuWang.cpp:{FIRST_LINE}-{LAST_LINE}: {executable} executable lines, {len(missed)} never executed")
        assert not missed, f"lines never executed by the fixture's inputs: {missed}"
    save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
