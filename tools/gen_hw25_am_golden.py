#!/usr/bin/env python3
"""tools/gen_hw25_am_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw25_am_golden.npz: what THE REFERENCE ITSELF makes of a few signals in computeAM, finalSeg and the final
binarisation (function/20141106_speech_enhancement/aurora_etsi_test/HuWang.cpp:1146-1494, :99-106, with the tools of
:1553-1677): data only, no reference source.  Runs only where the reference tree exists:

    python tools/gen_hw25_am_golden.py <reference tree>

The reference's HuWang.cpp is compiled UNMODIFIED (g++ -O2 -ffp-contract=off -fPIC) in a temporary directory outside the
repository, with a two-line header of our own for `struct mask`, into a shared library.  A driver of our own is linked
against it and DEFINES functions with the names and signatures of some of the reference's (amPatt, hilbert, computeAMRate,
sinModel, reSegmentation, develope, initGroup).  The dynamic linker resolves the library's own calls of those names to the
driver's definitions, each of which records what goes in or comes out and calls the library's function of that name (looked
up with dlsym (RTLD_NEXT, ..)).  So the driver only CALLS the reference -- createIBM, finalSeg, computeAM themselves -- and
everything it dumps is what passed through those calls:

  * audio cases (tests/hw25_am_model.py::audio_inputs): one call of createIBM.  At the first amPatt the driver dumps Pitch, Grp
    (pitchDtm's), corrEv's cross, corrHc's pRatio and gOut; after each amPatt its output; at each computeAMRate its input (the
    normalised pattern); each sinModel's result, from which error / sEng follows with a window energy summed by the driver; at
    the first reSegmentation AmCrn; Grp at the second and third reSegmentation, at both developes and after the second (the
    state after each of finalSeg's five steps); N as hilbert receives it; the mask as createIBM returns it.  The tool checks
    that AmCrn is `ratio > THETAE ? 0 : 1` wherever sinModel ran.  initGroup's stand-in counts the segments first with the
    reference's segmentation and refuses an input with none or more than 400 (exit 3);
  * hand-made cases (tests/hw25_am_model.py::HAND_CASES): Grp, AmCrn, corrEv.cross and corrHc.pRatio as arrays, one call of
    finalSeg, the same five states; the mask is Grp > 0;
  * constants: N at L = 2^7 .. 2^17 as computeAM itself hands it to hilbert (on zeros; hilbert's stand-in does not transform
    them), kaiserPara's beta, and the twiddles of fft's stages with period 1 .. 512 in both directions, read off the reference's
    own fft: the transform of a unit impulse at sample 1 with N = n leaves stage n's u values in the first half of its output.

createIBM ends with `delete gOut[chan]` at chan == 25, one past the array; the driver replaces operator delete by one that
keeps the memory, so that the call returns.

Per audio case k: x_k; pitch_k [F] int32, grp_k [F][25] int8, cross_ev_k and pratio_k [F][25] float32 (finalSeg's inputs);
gout_crc_k, ampatt_crc_k, am_crc_k uint32 [25] (CRC32 per channel) and gout_s_k, ampatt_s_k, am_s_k (the values at
hw25_am_model.sample_index (L)); seng_k, ratio_k float32 and amcrn_k int8 [F][25]; the five stages and grp_final_k int8, mask_k.
Hand-made case k: the stages, grp_final_k and mask_k.  ratio_tol: twice the largest relative difference between the numpy
model's ratio (cosf, sinf, atanf taken as the double function rounded to float) and the reference's over all units where
sinModel runs; ratio_band_units: the number of such units whose reference ratio lies within ratio_tol (relative) of THETAE,
asserted to be 0, so that the labels compare exactly.

A second build with --coverage runs every input; gcov must show every executable line of HuWang.cpp:1146-1494 executed, and in
:1553-1677 exactly the lines that the constants make unreachable (UNREACHABLE below) not executed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hw25_am_model as AM  # noqa: E402
from tests import hw25_model as M  # noqa: E402
from tools import gen_hw25_pitch_golden as GP  # noqa: E402

PATH = AM.GOLDEN
NCH, HOP = 25, 80
# delta = 0.01 gives a = 40: kaiserPara's third beta branch (a > 50, :1561) is never taken (its first, `beta = 0`, shares line
# 1559 with the test itself); beta = 3.395 < 3.75 and sqrt (1 - k * k) <= 1 keep bessi0 in its polynomial branch (:1617-1618)
UNREACHABLE = {1561: "kaiserPara: a = 40 is not above 50", 1617: "bessi0: |x| <= beta < 3.75", 1618: "bessi0: |x| <= beta < 3.75"}

DRIVER = r"""
#include <dlfcn.h>
#include <new>
#include "HuWang.h"
extern long sigLength;
extern float *gOut[];
extern int numFrame;
extern corrLgm *corrHc, *corrEv;
extern int *Pitch;
extern int *Unit[2];
extern mask *AmCrn;

/* createIBM deletes one pointer past gOut[]: keep every block instead */
void operator delete(void *) noexcept {}
void operator delete(void *, std::size_t) noexcept {}
void operator delete[](void *) noexcept {}
void operator delete[](void *, std::size_t) noexcept {}

static FILE *fo;
static char mode;
static mask *theGrp;
static float *keptPatt, *keptAm, *keptEnergy, *keptRatio;
static const float *rateInput;
static int rateChan, pattCalls, segCalls, devCalls, seenN = -1;

static void put(const void *p, size_t n) { if (fwrite(p, 1, n, fo) != n) exit(2); }
static void putRows(const mask *g) { for (int f = 0; f < numFrame; f++) put(g[f].mark, sizeof g[f].mark); }
template <typename F> static F library(const char *name)
{
    void *p = dlsym(RTLD_NEXT, name);
    if (!p) exit(5);
    return reinterpret_cast<F>(p);
}

/* ---- stand-ins: the library's calls of these names arrive here; each passes the call on to the library's own function ---- */
void initGroup(mask *grp)
{
    mask *copy = new mask[numFrame + 1];
    int *marks = new int[long(numFrame + 1) * NUMBER_CHANNEL];
    memcpy(copy, grp, sizeof(mask) * numFrame);
    const int found = segmentation(copy, numFrame, Unit, marks);
    if (found < 1 || found > MAX_NUMBER_SEGMENT) exit(3);
    library<void (*)(mask *)>("_Z9initGroupP4mask")(grp);
}

void amPatt(float *input, float *output, long length, int *pitch)
{
    if (mode == 'a' && pattCalls == 0) {
        put(pitch, sizeof(int) * numFrame);
        putRows(theGrp);
        for (int f = 0; f < numFrame; f++) put(corrEv[f].cross, sizeof corrEv[f].cross);
        for (int f = 0; f < numFrame; f++) put(corrHc[f].pRatio, sizeof corrHc[f].pRatio);
        for (int c = 0; c < NUMBER_CHANNEL; c++) put(gOut[c], sizeof(float) * length);
        keptPatt = new float[length * NUMBER_CHANNEL];
        keptAm = new float[length * NUMBER_CHANNEL];
        keptEnergy = new float[long(numFrame + 1) * NUMBER_CHANNEL];
        keptRatio = new float[long(numFrame + 1) * NUMBER_CHANNEL];
    }
    library<void (*)(float *, float *, long, int *)>("_Z6amPattPfS_lPi")(input, output, length, pitch);
    if (mode == 'a') memcpy(keptPatt + pattCalls * length, output, sizeof(float) * length);
    pattCalls++;
}

void hilbert(float *re, float *im, int N)
{
    seenN = N;
    if (mode != 'c') library<void (*)(float *, float *, int)>("_Z7hilbertPfS_i")(re, im, N);
}

float sinModel(float *sig, float a, float freq)
{
    const float err = library<float (*)(float *, float, float)>("_Z8sinModelPfff")(sig, a, freq);
    if (rateInput) keptRatio[((sig - rateInput) / OFFSET + 1) * NUMBER_CHANNEL + rateChan] = err;
    return err;
}

static float windowEnergy(const float *p)
{
    float total = 0;
    for (int i = 0; i < WINDOW; i++) total += p[i] * p[i];
    return total;
}

void computeAMRate(float *input, int chan, int *pitch, int frames, mask *labels)
{
    if (mode == 'a') {
        memcpy(keptAm + chan * sigLength, input, sizeof(float) * sigLength);
        for (int f = 0; f < frames; f++) keptRatio[f * NUMBER_CHANNEL + chan] = -1; /* sinModel's result is never negative */
        rateInput = input;
        rateChan = chan;
    }
    library<void (*)(float *, int, int *, int, mask *)>("_Z13computeAMRatePfiPiiP4mask")(input, chan, pitch, frames, labels);
    rateInput = 0;
    if (mode != 'a') return;
    for (int f = 0; f < frames; f++) {
        const bool interior = f >= 1 && f + 1 < frames;
        const float energy = interior ? windowEnergy(input + (f - 1) * OFFSET) : 0;
        float &r = keptRatio[f * NUMBER_CHANNEL + chan];
        keptEnergy[f * NUMBER_CHANNEL + chan] = energy;
        r = r < 0 ? 0 : r / energy;
    }
}

void reSegmentation(mask *m)
{
    if (segCalls == 0 && mode == 'a') putRows(AmCrn);
    if (segCalls > 0) putRows(theGrp); /* Grp after finalSeg's first and second step */
    segCalls++;
    library<void (*)(mask *)>("_Z14reSegmentationP4mask")(m);
}

void develope(mask *m, int v, mask *grp)
{
    putRows(grp); /* Grp after the third and the fourth step */
    library<void (*)(mask *, int, mask *)>("_Z8developeP4maskiS0_")(m, v, grp);
    if (devCalls == 1) putRows(grp); /* and after the fifth */
    devCalls++;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *fi = fopen(argv[1], "rb");
    fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    mode = argv[3][0];
    if (mode == 'c') { /* constants */
        for (int k = 7; k <= 17; k++) {
            sigLength = 1L << k;
            numFrame = sigLength / OFFSET;
            for (int c = 0; c < NUMBER_CHANNEL; c++) gOut[c] = new float[sigLength]();
            Pitch = new int[numFrame + 1]();
            AmCrn = new mask[numFrame + 1];
            computeAM();
            put(&seenN, sizeof seenN);
        }
        int fLength;
        float beta;
        kaiserPara(0.01, 0.1, fLength, beta);
        put(&beta, sizeof beta);
        for (int dir = 1; dir >= -1; dir -= 2)
            for (int n = 1; n <= 10; n++) {
                long points = 1L << n;
                float *re = new float[points](), *im = new float[points]();
                re[1] = 1;
                fft(re, im, n, dir);
                for (long j = 0; j < points / 2; j++) {
                    put(&re[j], sizeof(float));
                    put(&im[j], sizeof(float));
                }
            }
        fclose(fo);
        return 0;
    }
    if (mode == 'h') { /* hand-made arrays straight into finalSeg */
        if (fread(&numFrame, sizeof(int), 1, fi) != 1) return 2;
        theGrp = new mask[numFrame + 1];
        AmCrn = new mask[numFrame + 1];
        corrHc = new corrLgm[numFrame + 1]();
        corrEv = new corrLgm[numFrame + 1]();
        for (int f = 0; f < numFrame; f++) if (fread(theGrp[f].mark, sizeof theGrp[f].mark, 1, fi) != 1) return 2;
        for (int f = 0; f < numFrame; f++) if (fread(AmCrn[f].mark, sizeof AmCrn[f].mark, 1, fi) != 1) return 2;
        for (int f = 0; f < numFrame; f++) if (fread(corrEv[f].cross, sizeof corrEv[f].cross, 1, fi) != 1) return 2;
        for (int f = 0; f < numFrame; f++) if (fread(corrHc[f].pRatio, sizeof corrHc[f].pRatio, 1, fi) != 1) return 2;
        Unit[0] = new int[long(numFrame + 1) * NUMBER_CHANNEL];
        Unit[1] = new int[long(numFrame + 1) * NUMBER_CHANNEL];
        finalSeg(theGrp);
        putRows(theGrp);
        fclose(fo);
        return 0;
    }
    static float x[MAX_SIG_LENGTH];
    const long len = (long)fread(x, sizeof(float), MAX_SIG_LENGTH, fi);
    theGrp = new mask[len / OFFSET + 1];
    createIBM(x, (int)len, theGrp);
    put(&seenN, sizeof seenN);
    put(keptPatt, sizeof(float) * len * NUMBER_CHANNEL);
    put(keptAm, sizeof(float) * len * NUMBER_CHANNEL);
    put(keptEnergy, sizeof(float) * numFrame * NUMBER_CHANNEL);
    put(keptRatio, sizeof(float) * numFrame * NUMBER_CHANNEL);
    putRows(theGrp);
    fclose(fo);
    return 0;
}
"""


def build(ref_root, tmp, name, extra):
    """HuWang.cpp unmodified into a shared library, the driver linked against it -> the driver's path"""
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
    exe = os.path.join(work, "hw25_am_ref")
    flags = ["g++", "-O2", "-ffp-contract=off", "-fPIC", "-w", *extra, "-I", inc, "-I", os.path.join(ref_root, GP.REL)]
    subprocess.check_call(flags + ["-c", src, "-o", os.path.join(work, "HuWang.o")], cwd=work)
    subprocess.check_call(["g++", "-shared", *extra, os.path.join(work, "HuWang.o"), "-o", os.path.join(work, "libhuwang.so")], cwd=work)
    subprocess.check_call(flags + ["-c", os.path.join(work, "driver.cpp"), "-o", os.path.join(work, "driver.o")], cwd=work)
    subprocess.check_call(["g++", "-rdynamic", *extra, os.path.join(work, "driver.o"), "-L", work, "-lhuwang", "-ldl",
                           "-Wl,-rpath," + work, "-o", exe], cwd=work)
    return exe


class Reader:
    def __init__(self, path):
        self.raw, self.pos = np.fromfile(path, np.uint8), 0

    def take(self, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert self.pos + n <= len(self.raw), "the driver wrote less than expected"
        out = self.raw[self.pos:self.pos + n].view(dtype).reshape(shape).copy()
        self.pos += n
        return out

    def done(self):
        assert self.pos == len(self.raw), "the driver wrote more than was read"


def call(exe, tmp, mode, payload):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(payload)
    rc = subprocess.call([exe, fin, fout, mode], stdout=subprocess.DEVNULL, cwd=os.path.dirname(exe))
    if rc:
        raise SystemExit(f"the driver failed with {rc} (3: no segment, or more than 400; 5: a library function was not found)")
    return Reader(fout)


def marks(r, nfr, values):
    g = r.take(np.float32, nfr, NCH)
    assert np.isin(g, values).all()
    return g.astype(np.int8)


def final_part(r, nfr):
    return {name: marks(r, nfr, (-2, -1, 0, 1, 2, 3)) for name in AM.FINAL_STAGES}


def run_audio(exe, tmp, x):
    L, nfr = len(x), len(x) // HOP
    r = call(exe, tmp, "a", x.tobytes())
    out = dict(pitch=r.take(np.int32, nfr), grp=marks(r, nfr, (-1, 0, 1)), cross_ev=r.take(np.float32, nfr, NCH),
               pratio=r.take(np.float32, nfr, NCH), gout=r.take(np.float32, NCH, L), amcrn=marks(r, nfr, (0, 1)))
    out.update(final_part(r, nfr))
    out.update(N=int(r.take(np.int32, 1)[0]), ampatt=r.take(np.float32, NCH, L), am=r.take(np.float32, NCH, L),
               seng=r.take(np.float32, nfr, NCH), ratio=r.take(np.float32, nfr, NCH), mask=marks(r, nfr, (0, 1)))
    r.done()
    out["grp_final"] = out[AM.FINAL_STAGES[-1]]
    assert np.isin(out["grp_final"], (-1, 0, 1)).all() and np.array_equal(out["mask"], (out["grp_final"] > 0).astype(np.int8))
    # the label is the float ratio against the double THETAE wherever sinModel ran (a voiced frame with energy in its window)
    ran = (out["pitch"] > 0)[:, None] & (out["seng"] > 0)
    assert np.array_equal(out["ratio"] != 0, ran), "sinModel did not run where it was expected to"
    assert np.array_equal(out["amcrn"] == 1, ran & ~(out["ratio"].astype(np.float64) > AM.THETAE)), "AmCrn is not ratio > THETAE ? 0 : 1"
    return out


def run_hand(exe, tmp, c):
    nfr = c["grp"].shape[0]
    r = call(exe, tmp, "h", np.int32(nfr).tobytes() + b"".join(c[k].astype(np.float32).tobytes() for k in ("grp", "amcrn", "cross_ev", "pratio")))
    out = final_part(r, nfr)
    out["grp_final"] = marks(r, nfr, (-1, 0, 1))
    r.done()
    assert np.array_equal(out["grp_final"], out[AM.FINAL_STAGES[-1]])
    out["mask"] = (out["grp_final"] > 0).astype(np.int8)
    return out


def run_constants(exe, tmp):
    r = call(exe, tmp, "c", b"")
    out = dict(n_at_pow2=r.take(np.int32, 11), beta=r.take(np.float32, 1)[0])
    for name in ("tw_fwd", "tw_inv"):
        out[name] = np.concatenate([r.take(np.float32, 1 << (n - 1), 2) for n in range(1, 11)])
    r.done()
    return out


def uncovered(work, first, last):
    GP.FIRST_LINE, GP.LAST_LINE = first, last
    return GP.uncovered(work)


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/gen_hw25_am_golden.py <reference tree>")
    ref_root = sys.argv[1]
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref_root, tmp, "plain", [])
        cov = build(ref_root, tmp, "cov", ["--coverage"])
        for k, v in run_constants(exe, tmp).items():
            data[k] = v
        run_constants(cov, tmp)
        print(f"N at 2^7..2^17: {data['n_at_pow2'].tolist()}, beta {data['beta']!r}")
        t = M.tables()
        worst, refs = 0.0, []
        for k, x in AM.audio_inputs().items():
            r = run_audio(exe, tmp, x)
            c = run_audio(cov, tmp, x)
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
            # the numpy model on the same input: exact up to sEng, ratio to be measured
            g = AM.gout(x, t)
            assert M.same_bits(g, r["gout"]), f"{k}: the model's gOut differs"
            m = AM.am_stage(g, r["pitch"])
            for name in ("ampatt", "am", "seng"):
                assert M.same_bits(m[name], r[name]), f"{k}: the model's {name} differs from the reference's"
            run = r["ratio"] != 0
            rel = np.abs(m["ratio"][run].astype(np.float64) - r["ratio"][run]) / r["ratio"][run]
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            refs.append(r["ratio"][run].astype(np.float64))
            print(f"input {k}: L {L}, N {r['N']}, frames {L // HOP}, voiced {int((r['pitch'] > 0).sum())}, sinModel units {int(run.sum())}, "
                  f"AM labels {int(r['amcrn'].sum())}, mask units {int(r['mask'].sum())}, model ratio rel. diff {float(rel.max()) if rel.size else 0:.3g}, "
                  f"labels equal {np.array_equal(m['amcrn'], r['amcrn'].astype(np.float32))}")
        tol = 2 * worst
        refs = np.concatenate(refs)
        band = int((np.abs(refs - AM.THETAE) <= tol * AM.THETAE).sum())
        print(f"ratio_tol {tol:.3g}; units within it of THETAE: {band}; nearest {np.abs(refs - AM.THETAE).min():.3g}")
        assert band == 0, "a fixture unit lies within the tolerance band of THETAE: change the input"
        data["ratio_tol"] = np.float64(tol)
        data["ratio_band_units"] = np.int32(band)
        for k, make in AM.HAND_CASES.items():
            c = make()
            r = run_hand(exe, tmp, c)
            rc = run_hand(cov, tmp, c)
            assert all(np.array_equal(rc[n], r[n]) for n in r)
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: mask units {int(r['mask'].sum())}, -1 units {int((r['grp_final'] < 0).sum())}")
        executable, missed = uncovered(os.path.dirname(cov), 1146, 1494)
        print(f"HuWang.cpp:1146-1494: {executable} executable lines, {len(missed)} never executed")
        assert not missed, f"lines never executed by the fixture's inputs: {missed}"
        executable, missed = uncovered(os.path.dirname(cov), 1553, 1677)
        print(f"HuWang.cpp:1553-1677: {executable} executable lines, never executed: " + ", ".join(f"{n} ({UNREACHABLE.get(n, '?')})" for n in missed))
        assert set(missed) == set(UNREACHABLE), f"expected exactly the unreachable lines {sorted(UNREACHABLE)}, got {missed}"
    GP.save(PATH, data)
    assert os.path.getsize(PATH) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
