"""The contract of the long-recording denoiser without a GPU: the numpy model (tests/recordings_model.py)
against a plain-C restatement of the reference's level, BufferDenoise and band-pass loops, compiled here and linked to the
oracle's etsi_denoise; the model's cast and chunk table; the chunk plan and stitch map of csrc/recording_plan.h, through a
sanitized driver and through the library's calls (host arithmetic, no device), against the model."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import recordings_cases as C
from tests import recordings_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
# (S, B): the issue's lengths at chunk 1600, the smallest chunk, one that no length reaches, R = 0 at several T, the tool's own
PLAN_CASES = [(S, C.CHUNK) for S in C.LENGTHS if S >= 320] + [(5000, C.CHUNK), (2400, C.CHUNK), (3000, C.CHUNK)] + \
             [(320, 320), (321, 320), (640, 320), (4434, 320), (16057, 4000), (16057, 16080), (8000, 4000), (1440000 * 2 + 1007, 1440000)]

# aurora_speech_enhancement.cpp:25-80 and :171-215 in plain C.  Ours: `work` is zeroed before every etsi_denoise (the reference
# reuses it, so the len % 80 samples etsi_denoise never writes hold stale data there), the level is a parameter, and the FIR --
# IPP's in the reference -- is the in-order float sum of the contract.
RESTATEMENT = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int ora_etsi_denoise(const short *in, short *out, long n);
static const int etsi_offset_points = 320;

static void denoise(short *src, short *work, int n)
{
    memset(work, 0, (size_t)n * sizeof(short));
    ora_etsi_denoise(src, work, n);
}

static void BufferDenoise(short *src_wave, short *des_wave, int samples, int batch_length, short *work)
{
    int batch_times = samples / batch_length;
    int batch_left = samples % batch_length;
    int i;
    if (batch_times == 0) {
        denoise(src_wave, work, samples);
        memcpy(des_wave, work + etsi_offset_points, (size_t)(samples - etsi_offset_points) * sizeof(short));
        memset(des_wave + samples - etsi_offset_points, 0, etsi_offset_points * sizeof(short));
    } else {
        denoise(src_wave, work, batch_length);
        memcpy(des_wave, work + etsi_offset_points, (size_t)(batch_length - etsi_offset_points) * sizeof(short));
        for (i = 1; i < batch_times; i++) {
            denoise(src_wave + i * batch_length - etsi_offset_points, work, batch_length + etsi_offset_points);
            memcpy(des_wave + i * batch_length - etsi_offset_points, work + etsi_offset_points, (size_t)batch_length * sizeof(short));
        }
        denoise(src_wave + batch_times * batch_length - etsi_offset_points, work, batch_left + etsi_offset_points);
        memcpy(des_wave + batch_times * batch_length - etsi_offset_points, work + etsi_offset_points, (size_t)batch_left * sizeof(short));
        memset(des_wave + samples - etsi_offset_points, 0, etsi_offset_points * sizeof(short));
    }
}

int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    int ncase, c;
    if (!fi || !fo || fread(&ncase, 4, 1, fi) != 1) return 2;
    for (c = 0; c < ncase; c++) {
        int hdr[3], samples, K, t, k, status = 0;
        float level;
        double factor = 1.0;
        short *p_data, *des, *work;
        float *taps, *flt;
        if (fread(hdr, 4, 3, fi) != 3 || fread(&level, 4, 1, fi) != 1) return 2;
        samples = hdr[0], K = hdr[2];
        p_data = calloc(samples + 1, sizeof(short)), des = calloc(samples + 1, sizeof(short));
        work = calloc(hdr[1] + samples + 321, sizeof(short));
        taps = calloc(K + 1, sizeof(float)), flt = calloc(samples + 1, sizeof(float));
        if (fread(p_data, 2, samples, fi) != (size_t)samples || fread(taps, 4, K, fi) != (size_t)K) return 2;
        if (samples < etsi_offset_points) {
            status = 1, factor = 0.0;
        } else {
            if (level > 0) {
                double energy = 0.0f;
                for (t = 0; t < samples; t++) energy += p_data[t] * p_data[t];
                energy /= samples;
                energy = sqrt(energy);
                factor = level / energy;
                for (t = 0; t < samples; t++) p_data[t] = (short)((float)p_data[t] * factor);
            }
            BufferDenoise(p_data, des, samples, hdr[1], work);
            if (K) {
                for (t = 0; t < samples; t++) flt[t] = (float)des[t];
                for (t = 0; t < samples; t++) {
                    float acc = 0.0f;
                    for (k = 0; k < K && k <= t; k++) acc = acc + taps[k] * flt[t - k];
                    des[t] = (short)acc;
                }
            }
        }
        fwrite(&factor, 8, 1, fo), fwrite(&status, 4, 1, fo), fwrite(des, 2, samples, fo);
        free(p_data), free(des), free(work), free(taps), free(flt);
    }
    fclose(fo);
    return 0;
}
"""


def test_model_equals_the_c_restatement(tmp_path, oracle):
    from oracle import oracle as O
    (tmp_path / "rec.c").write_text(RESTATEMENT)
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(tmp_path / "rec.c"), O.ORACLE_SO,
                    "-Wl,-rpath," + os.path.dirname(O.ORACLE_SO), "-lm"], check=True)
    xs, taps = C.recordings(), C.tap_sets()
    cases = [(x, C.CHUNK, C.LEVEL, "33") for x in xs] + [(x, C.CHUNK, 0.0, "none") for x in xs]
    cases += [(xs[C.LONGEST], C.CHUNK, C.LEVEL, "300"), (xs[C.LONGEST], 4000, C.LEVEL, "one"), (xs[5], 320, C.LEVEL, "none")]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for x, B, level, name in cases:
            t = taps[name] if taps[name] is not None else np.zeros(0, np.float32)
            f.write(struct.pack("<iiif", x.size, B, t.size, level))
            f.write(x.tobytes())
            f.write(t.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    raw = open(tmp_path / "out.bin", "rb").read()
    den = M.oracle_denoise(oracle)
    pos, wrapped, nonfinite = 0, 0, 0
    for k, (x, B, level, name) in enumerate(cases):
        factor, status = struct.unpack_from("<di", raw, pos)
        got = np.frombuffer(raw, np.int16, x.size, pos + 12)
        pos += 12 + 2 * x.size
        want, wf, ws = M.denoise_recording(x, B, level, taps[name], den)
        assert status == ws and np.array_equal(got, want), f"case {k}: {x.size} samples, chunk {B}, level {level}, taps {name}"
        assert factor == wf or (np.isinf(factor) and np.isinf(wf)), f"case {k}: factor {factor!r} against {wf!r}"
        nonfinite += int(np.isinf(wf))
        if level > 0 and status == 0 and np.isfinite(wf):
            wrapped += int((np.abs(x.astype(np.float64) * wf) >= 32768).any())
    assert pos == len(raw)
    assert nonfinite >= 1 and wrapped >= 1, "the cases no longer reach the infinite factor or the wrapping product"


def test_x86_cast_model():
    p = np.array([0.9, -0.9, 32767.9, 32768.0, -32769.5, 65536.0 + 5.2, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.5,
                  np.nan, np.inf, -np.inf, 1e300])
    want = np.array([0, 0, 32767, -32768, 32767, 5, -1, 0, 0, 0, 0, 0, 0, 0], np.int16)
    assert np.array_equal(M.x86_short(p), want)
    p32 = p[[0, 1, 3, 5, 7, 8, 10, 11]].astype(np.float32)  # 2147483647 rounds to 2^31 in float
    assert np.array_equal(M.x86_short(p32), np.array([0, 0, -32768, 5, 0, 0, 0, 0], np.int16))


def test_chunk_table_covers_the_recording():
    for S in (320, 1000, 1600, 1640, 4434, 4800, 16057):
        ch = M.chunks(S, C.CHUNK)
        assert sum(n for _, n in ch) == S + 320 * (S // C.CHUNK)
        assert all(s % 80 == 0 for s, _ in ch) and ch[-1][0] + ch[-1][1] == S


def test_fir_model_is_the_in_order_float_sum():
    """the vectorised model against the scalar loop of the contract, taps longer than the signal included"""
    rng = np.random.default_rng(3)
    des = rng.integers(-20000, 20000, 97).astype(np.int16)
    for K in (1, 5, 33, 200):
        taps = (rng.standard_normal(K) / 3).astype(np.float32)
        want = np.zeros(des.size, np.float32)
        for t in range(des.size):
            acc = np.float32(0)
            for k in range(min(K, t + 1)):
                acc = np.float32(acc + np.float32(taps[k] * np.float32(des[t - k])))
            want[t] = acc
        assert np.array_equal(M.fir(des, taps), M.x86_short(want)), K
    assert np.array_equal(M.fir(des, np.ones(1, np.float32)), des)


def test_the_cases_reach_every_branch_of_the_contract():
    xs = C.recordings()
    model = C.stitched()
    assert [s for _, _, s in model].count(1) == 1 and sum(np.isinf(f) for _, f, _ in model) == 1
    shapes = {(x.size // C.CHUNK == 0, x.size % C.CHUNK == 0, 0 < x.size % C.CHUNK < 80, x.size % 80 != 0) for x in xs if x.size >= 320}
    assert {(True, False, False, True), (False, True, False, False), (False, False, True, True)} <= shapes
    lead = xs[len(C.LENGTHS)]
    assert not lead[:2000].any() and not model[len(C.LENGTHS)][0][:C.CHUNK - 320].any(), "a whole zero chunk gives zeros"
    assert model[len(C.LENGTHS)][0].any()
    for des, _, _ in model:
        assert not des[-320:].any()


def _model_plan(S, B):
    """chunk table, layout and stitch map from the model's chunks () alone"""
    ch = M.chunks(S, B)
    off = np.concatenate(([0], np.cumsum([(n + 7) // 8 * 8 for _, n in ch])))
    idx = np.full(S, -1, np.int64)
    for i, (s, n) in enumerate(ch):  # des[...] = work[320 : ...] of BufferDenoise, chunk by chunk
        lo, hi = (0, min(B, S) - 320) if i == 0 else (s, s + n - 320)
        idx[lo:hi] = off[i] + 320 + np.arange(hi - lo)
    idx[S - 320:] = -1
    return ch, off, idx


def test_plan_header_equals_the_model_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/recording_plan_driver.cpp"
    exe = str(tmp_path / "recording_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "recording_plan_driver.cpp"), "-o", exe])
    small = [c for c in PLAN_CASES if c[0] < 100000]
    bad = [(100, 1600), (5000, 1000), (5000, 240), (5000, 0)]
    stdin = "".join(f"{S} {B}\n" for S, B in small + bad)
    run = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    blocks = run.stdout.split("case ")[1:]
    assert len(blocks) == len(small) + len(bad)
    for (S, B), block in zip(small, blocks):
        lines = block.split("\n")
        ch, off, idx = _model_plan(S, B)
        n, layout = map(int, lines[0].split())
        assert n == len(ch) and layout == off[-1], (S, B)
        got = [tuple(map(int, l.split())) for l in lines[1:1 + n]]
        assert got == [(s, ln, int(o)) for (s, ln), o in zip(ch, off)], (S, B)
        assert all(o % 8 == 0 and s % 80 == 0 for s, _, o in got)
        stitch = np.array(lines[1 + n].split(), np.int64)
        assert stitch[0] == -1 and stitch[-1] == -1 and np.array_equal(stitch[1:-1], idx), (S, B)
    assert all(b.startswith("-1 0") for b in blocks[len(small):])


@pytest.mark.parametrize("S,B", PLAN_CASES)
def test_library_plan_and_stitch_map(S, B):
    import speech_enhancement_amd as sea
    p = sea.recording_plan(S, B)
    ch = M.chunks(S, B)
    assert list(zip(p["src"].tolist(), p["len"].tolist())) == ch
    assert p["layout"] == S + 320 * (S // B) + (-(ch[-1][1]) % 8)
    if S < 100000:
        assert np.array_equal(sea.recording_stitch_map(S, B), _model_plan(S, B)[2])
    else:  # a window across the stitch boundary of the last chunk (des[2B - 320]), and the tail
        t = np.arange(2 * B - 700, 2 * B - 200)
        assert np.array_equal(sea.recording_stitch_map(S, B, int(t[0]), t.size), t + 320 + 320 * ((t + 320) // B))
        assert (sea.recording_stitch_map(S, B, S - 321, 321) == np.concatenate(([S - 321 + 320 + 640], np.full(320, -1)))).all()


def test_stitch_map_applied_to_the_oracles_chunks_is_buffer_denoise(oracle):
    """what a caller does with the plan: every chunk through etsi_denoise into the zeroed layout, then the map"""
    import speech_enhancement_amd as sea
    den = M.oracle_denoise(oracle)
    for x in C.recordings():
        if x.size < 320:
            assert sea.recording_plan(x.size, C.CHUNK)["layout"] == 0 and len(sea.recording_plan(x.size, C.CHUNK)["src"]) == 0
            continue
        p = sea.recording_plan(x.size, C.CHUNK)
        work = np.zeros(p["layout"], np.int16)
        for s, n, o in zip(p["src"], p["len"], p["off"]):
            work[o:o + n] = den(x[s:s + n])
        idx = sea.recording_stitch_map(x.size, C.CHUNK)
        des = np.where(idx >= 0, work[np.maximum(idx, 0)], 0).astype(np.int16)
        assert np.array_equal(des, M.buffer_denoise(x, C.CHUNK, den)), x.size


@pytest.mark.parametrize("chunk", [1000, 240, 0, -1600])
def test_a_bad_chunk_is_rejected(chunk):
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    assert lib.sea_recording_plan(5000, chunk, None, None, None, 0) == -1 and b"chunk" in lib.sea_last_error()
    idx = np.full(10, 7, np.int64)
    assert lib.sea_recording_stitch_map(5000, chunk, 0, 10, idx.ctypes.data) != 0 and (idx == 7).all()
    with pytest.raises(sea.SeaError):
        sea.recording_plan(5000, chunk)
    with pytest.raises(sea.SeaError):
        sea.recording_stitch_map(5000, 1600, 4995, 10)  # past the end


def test_prototypes_are_bound_and_take_no_stream():
    from speech_enhancement_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sea_recording_plan", "sea_recording_layout_samples", "sea_recording_stitch_map"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "sea_mi355x.h")).read()
    assert "void *stream" not in header[header.index("long long sea_recording_plan"):header.index("int sea_recording_stitch_map") + 120]
