#!/usr/bin/env python3
"""tools/gen_hw25_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw25_golden.npz: four short float signals and what THE REFERENCE ITSELF makes of them in the front
half of createIBM() (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:41-76): data only, no reference
source.  Runs only where the reference tree exists:

    python tools/gen_hw25_golden.py [/root/reference]

The reference's HuWang.cpp is compiled UNMODIFIED (g++ -O2 -ffp-contract=off) in a temporary directory outside the
repository.  It needs one thing from the absent aurora/aurora_include.h chain, `struct mask` and NUMBER_CHANNEL: a two-line
header of our own under the literal name its `#include "..\\aurora_etsi\\NoiseSupExports.h"` asks for supplies them.  A small
driver of our own sets the file's globals, calls AudiPeriph / lowPass / computeACF / crossCorr / globalPitch / timeCrn, applies
the labelling rule of createIBM:74-76, and dumps the arrays; the low-pass taps come from the file's kaiserPara /
kaiserLowPass called with lowPass's arguments.

Per input k in a, b, c, d: x_k, hOut_k / hEv_k [25][L], acf_hc_k / acf_ev_k [F][25][101], cross_hc_k / cross_ev_k / pRatio_k /
mark_k [F][25], pitch_k [F]; the tables cf, bw, midEarCoeff, winsize [25] and lp [91].

The large float arrays (hOut, hEv, both ACFs) are stored as their four byte planes, uint8 [4][shape], least significant byte
first: zlib packs the sign / exponent planes far tighter than interleaved floats (1.09 MB -> 0.87 MB), which keeps the file
under 1 MiB.  tests/hw25_model.py::load_golden() puts them together again.

Before the file is written the tool asserts, on the instrumented build that `make -C oracle hwcov` leaves under
oracle/_ref/hwcov (tools/hw_oracle_coverage.py), that its inputs execute every executable line of HuWang.cpp:117-465 but the
two of UNREACHABLE below.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "hw25_golden.npz")
REL = os.path.join("function", "20141106_speech_enhancement", "aurora_etsi_test")
NCH, NDEL, HOP, L_FULL = 25, 101, 80, 1210

HEADER = "#define NUMBER_CHANNEL 25\nstruct mask { float mark[NUMBER_CHANNEL]; };\n"

DRIVER = r"""
#include "HuWang.h"
extern long sigLength;
extern float Input[], *gOut[], *hOut[], *hEv[];
extern gammaTone fChan[];
extern int numFrame;
extern corrLgm *corrHc, *corrEv;
extern int *Pitch;

static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(2); }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
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
    mask *Grp = new mask[numFrame + 1];
    AudiPeriph();
    lowPass();
    computeACF();
    crossCorr();
    globalPitch();
    timeCrn(corrHc);
    /* the labelling of createIBM: both tests in the types the header's constants give them (double, int) */
    for (int f = 0; f < numFrame; f++)
        for (int c = 0; c < NUMBER_CHANNEL; c++) {
            const bool coherent = corrHc[f].cross[c] > THETAC;
            const bool loud = corrHc[f].acf[c][0] > (THETAA * THETAA);
            Grp[f].mark[c] = (coherent && loud) ? 1.0f : 0.0f;
        }

    for (int c = 0; c < NUMBER_CHANNEL; c++) put(fo, &fChan[c].cf, sizeof(float));
    for (int c = 0; c < NUMBER_CHANNEL; c++) put(fo, &fChan[c].bw, sizeof(float));
    for (int c = 0; c < NUMBER_CHANNEL; c++) put(fo, &fChan[c].midEarCoeff, sizeof(float));
    for (int c = 0; c < NUMBER_CHANNEL; c++) { /* computeACF's window: four periods of the centre frequency, WINDOW at least */
        const int periods4 = int(4 * SAMPLING_FREQUENCY / fChan[c].cf);
        const int win = periods4 < WINDOW ? WINDOW : periods4;
        put(fo, &win, sizeof(int));
    }
    { /* lowPass's filter: its two calls with its arguments */
        const float transition = float(STOPBAND - PASSBAND) / SAMPLING_FREQUENCY, cutoff = float(PASSBAND + STOPBAND) / SAMPLING_FREQUENCY;
        int order;
        float beta;
        kaiserPara(RIPPLE, transition, order, beta);
        float *taps = new float[order + 1];
        kaiserLowPass(taps, order, beta, cutoff);
        put(fo, &order, sizeof(int));
        put(fo, taps, sizeof(float) * (order + 1));
    }
    for (int c = 0; c < NUMBER_CHANNEL; c++) put(fo, hOut[c], sizeof(float) * sigLength);
    for (int c = 0; c < NUMBER_CHANNEL; c++) put(fo, hEv[c], sizeof(float) * sigLength);
    for (int f = 0; f < numFrame; f++) put(fo, corrHc[f].acf, sizeof corrHc[f].acf);
    for (int f = 0; f < numFrame; f++) put(fo, corrEv[f].acf, sizeof corrEv[f].acf);
    for (int f = 0; f < numFrame; f++) put(fo, corrHc[f].cross, sizeof corrHc[f].cross);
    for (int f = 0; f < numFrame; f++) put(fo, corrEv[f].cross, sizeof corrEv[f].cross);
    for (int f = 0; f < numFrame; f++) put(fo, corrHc[f].pRatio, sizeof corrHc[f].pRatio);
    for (int f = 0; f < numFrame; f++) put(fo, Grp[f].mark, sizeof Grp[f].mark);
    put(fo, Pitch, sizeof(int) * numFrame);
    fclose(fo);
    return 0;
}
"""


def harmonic(L, amp, f0, nharm, noise, seed):
    """silence (or the noise alone) for the first third, then sum over h <= nharm of (amp / h) sin (2 pi f0 h n / 8000)"""
    n = np.arange(L, dtype=np.float64)
    x = np.zeros(L, np.float64)
    for h in range(1, nharm + 1):
        x += (amp / h) * np.sin(2 * np.pi * f0 * h * n / 8000.0)
    x[n < L // 3] = 0.0
    if noise:
        x += np.random.default_rng(seed).uniform(-noise, noise, L)
    return x.astype(np.float32)


def inputs():
    a = harmonic(L_FULL, 30.0, 150.0, 3, 0.0, 0)
    return {"a": a,
            "b": harmonic(L_FULL, 300.0, 110.0, 8, 0.3, 20141106),
            "c": harmonic(L_FULL, 3000.0, 100.0, 30, 0.0, 0),
            "d": a[:80].copy()}


def build(ref_root, tmp):
    src = os.path.join(ref_root, REL, "HuWang.cpp")
    if not os.path.exists(src):
        raise SystemExit(f"{src} is missing: this tool runs only where the reference tree exists")
    inc = os.path.join(tmp, "inc")
    os.makedirs(inc)
    with open(os.path.join(inc, "..\\aurora_etsi\\NoiseSupExports.h"), "w") as fh:
        fh.write(HEADER)
    with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "hw25_ref")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-w", "-I", inc, "-I", os.path.join(ref_root, REL),
                           os.path.join(tmp, "driver.cpp"), src, "-o", exe])
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


def planes(a):
    """float32 [shape] -> uint8 [4][shape], plane k = byte k of every value (little endian)"""
    return np.ascontiguousarray(np.moveaxis(a.astype("<f4").view(np.uint8).reshape(a.shape + (4,)), -1, 0))


def outcomes(r):
    """cells labelled 1 / failing only the cross test / only the energy test / both (createIBM:76)"""
    cross = r["cross_hc"].astype(np.float64) > 0.985
    energy = r["acf_hc"][:, :, 0] > np.float32(2500)
    return np.array([(cross & energy).sum(), (~cross & energy).sum(), (cross & ~energy).sum(), (~cross & ~energy).sum()])


# loudnessLevelInPhons's refusal of a frequency outside its table (:191-192): the centre frequencies are constants inside it
UNREACHABLE = {191: "loudnessLevelInPhons: every centre frequency lies inside 20..12500 Hz", 192: "the same refusal's exit"}


def assert_lines_executed(bank, signals):
    """every executable line of the front half's functions (HuWang.cpp:117-465; createIBM above them is not called by the
    driver) but UNREACHABLE ran on the fixture's inputs, on the instrumented build of `make -C oracle hwcov`"""
    sys.path.insert(0, ROOT)
    from tools import hw_oracle_coverage as C
    executable, missed = C.front_lines_missed(bank, signals, 117, 465)
    print(f"HuWang.cpp:117-465: {executable} executable lines, never executed: " + ", ".join(f"{n} ({UNREACHABLE.get(n, '?')})" for n in missed))
    assert executable > 150 and set(missed) == set(UNREACHABLE), f"expected exactly the unreachable lines {sorted(UNREACHABLE)}, got {missed}"


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    data, total = {}, np.zeros(4, np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp)
        for k, x in inputs().items():
            r = run(exe, tmp, x)
            for name in ("cf", "bw", "midEarCoeff", "winsize", "lp"):
                if name in data:
                    assert np.array_equal(data[name], r[name])
                data[name] = r.pop(name)
            assert np.array_equal(r["mark"] == 1, (r["cross_hc"].astype(np.float64) > 0.985) & (r["acf_hc"][:, :, 0] > np.float32(2500)))
            data[f"x_{k}"] = x
            for name, v in r.items():
                data[f"{name}_{k}"] = planes(v) if name in ("hOut", "hEv", "acf_hc", "acf_ev") else v
            o = outcomes(r)
            print(f"input {k}: L {len(x)}, frames {len(x) // HOP}, labelled 1 / cross fails / energy fails / both: {o.tolist()}, "
                  f"pitches {sorted(set(r['pitch'].tolist()))}")
            if k in "abc":
                total += o
    assert len(data["lp"]) == 91 and (data["winsize"][:3] > 200).all()
    assert_lines_executed("hw25", inputs().values())
    assert (total >= 5).all(), f"the labelling's four outcomes over (a)-(c) are {total.tolist()}: each needs 5 cells"
    np.savez_compressed(PATH, **data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
