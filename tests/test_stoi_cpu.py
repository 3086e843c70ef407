"""STOI without a GPU: the committed tables against their generator, known answers and the fall with
the SNR on the plain-C statement of the contract (tests/stoi_model_driver.c), that statement against an independent float64
model (tests/stoi_float64_model.py), the same program under the sanitizers, the conditions the inputs of
tests/test_gpu_stoi.py must meet, and the new symbols and their refusals."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import stoi_float64_model as D
from tests import stoi_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
TABLES = os.path.join(ROOT, "speech_enhancement_amd", "csrc", "stoi_tables.inc")
NEW_SYMBOLS = ("sea_stoi_utterances", "sea_stoi_last_chunks", "sea_stoi_last_stage_ms")
SNRS = (20, 10, 0, -10)

# The float32 contract against the float64 model over the inputs of test_c_model_against_the_float64_model (the speech-like
# signal clean and at four SNRs, and the chunk list, at both rates).  Measured: |stoi_C - stoi_64| at most 1.58e-8, |d_C - d_64|
# at most 5.01e-7.  Float rounding varies with the input and the inputs are few: the bounds are four times the measured values.
MEASURED_STOI, MEASURED_D = 1.58e-8, 5.01e-7
BOUND_STOI, BOUND_D = 4 * MEASURED_STOI, 4 * MEASURED_D


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def test_committed_tables_are_the_generators_output_bit_for_bit():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_stoi_tables.py"), "--print"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout == open(TABLES).read()
    text = run.stdout
    assert "#define SEA_STOI_BAND_LO 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219\n" in text
    # the float nearest 1 + 10^(15 / 20) = 6.62341325...
    clip = re.search(r"#define SEA_STOI_CLIP (\S+)f ", text).group(1)
    assert float.fromhex(clip) == float(np.float32(1.0 + 10.0 ** 0.75)) and clip == "0x1.a7e600p+2"
    for name, n in (("W", 256), ("CS", 512), ("H16", 161), ("H8", 101)):
        assert f"#define SEA_STOI_{name}_N {n}\n" in text


def test_tables_against_numpy_and_the_band_edges_against_the_paper():
    def table(name):
        body = open(TABLES).read().split(f"#define SEA_STOI_{name}_VALUES")[1].split("#define")[0]
        return np.array([float.fromhex(t[:-1]) for t in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+f", body)])

    w, cs, h16, h8 = table("W"), table("CS"), table("H16"), table("H8")
    assert (w.size, cs.size, h16.size, h8.size) == (256, 512, 161, 101)
    assert np.abs(w - np.hanning(258)[1:-1]).max() <= 2.0 ** -24  # one rounding to float of a value below 1
    assert np.abs(cs - np.cos(2 * np.pi * np.arange(512) / 512)).max() <= 2.0 ** -24
    for h, big in ((h16, 8), (h8, 5)):
        t = np.arange(-10 * big, 10 * big + 1)
        assert np.abs(h - 5 * np.sinc(t / big) / big * np.kaiser(t.size, 5.0)).max() <= 2.0 ** -24
        assert abs(h.sum() - 5.0) <= 0.02  # gain p over the upsampled signal, not renormalised
    A = D.third_octave_matrix()
    lo = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]
    for j in range(15):
        assert np.flatnonzero(A[j]).tolist() == list(range(lo[j], lo[j + 1]))


# ---- known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", M.RATES)
def test_known_answers(rate):
    ref = M.to_i16(M.speech_like(rate))
    same, silent_est, silent_ref = M.driver_stoi([ref, ref, np.zeros(ref.size, np.int16)], [ref.copy(), np.zeros(ref.size, np.int16), ref], rate)
    assert same["terms"] > 0 and abs(same["stoi"] - 1.0) <= 1e-6
    assert silent_est["terms"] == same["terms"] and silent_est["kept"] == same["kept"]
    assert np.all(silent_est["d"].view(np.uint32) == 0) and silent_est["stoi_sum"] == 0.0 and silent_est["stoi"] == 0.0
    assert silent_ref["frames"] == same["frames"] and silent_ref["kept"] == 0 and silent_ref["terms"] == 0
    assert math.isnan(silent_ref["stoi"])


@pytest.mark.parametrize("rate", M.RATES)
def test_stoi_falls_strictly_with_the_snr(rate):
    x = M.speech_like(rate)
    ref = M.to_i16(x)
    ests = [ref.copy()] + [M.to_i16(M.with_noise(x, snr, 5)) for snr in SNRS]
    got = [r["stoi"] for r in M.driver_stoi([ref] * len(ests), ests, rate)]
    print(f"rate {rate}: stoi clean and at {SNRS} dB: {[round(v, 4) for v in got]}")
    assert all(a > b for a, b in zip(got, got[1:]))
    assert got[1] > 0.99 and got[-1] < 0.75


# ---- the float32 contract against float64 -------------------------------------------------------------------------------------------
def test_c_model_against_the_float64_model():
    worst_stoi = worst_d = 0.0
    for rate in M.RATES:
        x = M.speech_like(rate)
        ref = M.to_i16(x)
        refs = [ref] * 5
        ests = [ref.copy()] + [M.to_i16(M.with_noise(x, snr, 5)) for snr in SNRS]
        cr, ce = M.chunk_list(rate)
        refs, ests = refs + cr, ests + ce
        for r, e, c in zip(refs, ests, M.driver_stoi(refs, ests, rate)):
            f = D.stoi(r, e, rate)
            # both precisions keep the same frames, and no term is decided by a zero denominator
            assert np.abs(f["ratio"] - 1.0).min() > 1e-3 and f["den_min"] > 0
            assert (c["frames"], c["kept"]) == (f["frames"], f["kept"]) and c["d"].shape == f["d"].shape
            worst_stoi = max(worst_stoi, abs(c["stoi"] - f["stoi"]))
            worst_d = max(worst_d, float(np.abs(c["d"] - f["d"]).max()))
    print(f"C model against float64: |stoi| {worst_stoi:.3g} (bound {BOUND_STOI:.3g}), |d| {worst_d:.3g} (bound {BOUND_D:.3g})")
    assert worst_stoi <= BOUND_STOI and worst_d <= BOUND_D


def test_c_model_is_clean_under_the_sanitizers():
    """the same driver at -O1 with -fsanitize=address,undefined, a stand-alone program, on test inputs: the same bits"""
    for rate in M.RATES:
        cases = M.removal_cases(rate)
        refs, ests = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
        sr, se = M.short_cases(rate)
        tr, te = M.tile_cases(rate)
        refs, ests = refs + sr + tr[:12], ests + se + te[:12]
        for a, b in zip(M.driver_stoi(refs, ests, rate), M.driver_stoi(refs, ests, rate, sanitize=True)):
            assert M.same_result(a, b) == 0


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", M.RATES)
def test_tile_and_short_cases_have_the_frames_their_names_say(rate):
    refs, ests, want = M.cached("tile", rate, lambda: M.tile_cases(rate))
    expect = [F for F in M.TILE_F for _ in M.TILE_R]
    assert [w["frames"] for w in want] == expect and [w["kept"] for w in want] == expect  # no frame is removed
    for L, F, r in zip(M.tile_lengths(rate), expect, [r for _ in M.TILE_F for r in M.TILE_R]):
        assert abs(M.l10_of(L, rate) - (128 * (F + 1) + r)) <= (0 if rate == 16000 else 1) and M.frames_of(L, rate) == F
    assert [M.frames_of(L, rate) for L in M.short_lengths(rate)] == [0, 0, 0, 1]
    assert M.short_lengths(rate)[:2] == [0, 1] and M.l10_of(M.short_lengths(rate)[2], rate) < 256 <= M.l10_of(M.short_lengths(rate)[3], rate)


@pytest.mark.parametrize("rate", M.RATES)
def test_random_gpu_inputs_remove_frames_and_clip_terms(rate):
    """between 10 % and 90 % of the frames removed; at least 5 % of the (segment, band, frame) values on the clipped branch"""
    refs, ests, want = M.cached("chunk", rate, lambda: M.chunk_list(rate))
    frames, kept = sum(w["frames"] for w in want), sum(w["kept"] for w in want)
    values = clipped = 0.0
    for r, e, w in zip(refs, ests, want):
        f = D.stoi(r, e, rate)
        values += 30 * w["terms"]
        clipped += f["clipped"] * 30 * w["terms"]
    print(f"rate {rate}: {frames - kept} of {frames} frames removed, {clipped / values:.3f} of the values clipped")
    assert 0.10 * frames <= frames - kept <= 0.90 * frames
    assert clipped >= 0.05 * values
    if rate == 16000:  # what test_gpu_stoi.py's chunking case counts on
        sizes = {M.chunk_bytes(r.size, rate) for r in refs}
        assert len(sizes) == 1 and 2 * max(sizes) <= 2 ** 20 < 3 * max(sizes)
    for refs, ests in M.placement_lists(rate)[2:]:
        got = M.driver_stoi(refs, ests, rate)
        assert got[len(refs) // 2]["frames"] == 0
        assert sum(1 for g in got if 0 < g["kept"] < 30) >= 2 and sum(1 for g in got if g["terms"] > 0) >= 30


@pytest.mark.parametrize("rate", M.RATES)
def test_removal_cases_are_what_their_names_say(rate):
    refs, ests, want = M.cached("removal", rate, lambda: tuple(map(list, zip(*M.removal_cases(rate).values()))))
    got = dict(zip(M.removal_cases(rate), want))
    F = got["identical"]["frames"]
    assert got["identical"]["kept"] == F > 64 and abs(got["identical"]["stoi"] - 1.0) <= 1e-6
    assert 30 < got["leading and trailing silence"]["kept"] < F - 40
    gap = got["a gap across the tile edge"]
    assert F - 12 <= gap["kept"] < F - 3 and gap["kept"] > 64
    assert got["every second frame"]["kept"] == (F + 1) // 2  # the float64 model keeps exactly the even frames
    every_second = D.stoi(*M.removal_cases(rate)["every second frame"], rate)
    assert np.flatnonzero(every_second["ratio"] > 1).tolist() == list(range(0, F, 2))
    assert np.abs(np.log10(every_second["ratio"])).min() > 1.0  # no decision within 10 dB of the threshold
    assert got["silent reference"]["kept"] == 0 and got["silent reference"]["terms"] == 0
    assert got["silent estimate"]["terms"] > 0 and np.all(got["silent estimate"]["d"] == 0)
    assert got["extremes"]["kept"] > 0 and got["extremes, alternating"]["kept"] > 0


# ---- symbols and refusals ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_bound_and_built_and_none_takes_a_stream():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    from tests import stream_cases as S
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
        assert not re.search(name + r"\([^;]*\bstream\b[^;]*\);", header), f"{name} takes a stream"
    assert len(S.stream_prototypes()) == 44
    blob = open(sea.LIB_PATH, "rb").read()
    for kernel in (b"stoi_basis_kernel", b"stoi_resample_kernel", b"stoi_energy_kernel", b"stoi_compact_kernel", b"stoi_band_kernel",
                   b"stoi_segment_kernel", b"stoi_finish_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    for name in ("stoi_utterances", "stoi_last_chunks", "stoi_frames"):
        assert callable(getattr(sea, name))
    makefile = open(os.path.join(ROOT, "speech_enhancement_amd", "csrc", "Makefile")).read()
    for name in ("stoi_kernel.hip", "stoi_capi.hip", "stoi_kernels.h", "stoi_tables.inc"):
        assert name in makefile
    assert [sea.stoi_frames(L, r) for r in M.RATES for L in M.short_lengths(r)] == [0, 0, 0, 1] * 2
    assert sea.stoi_frames(32000) == M.frames_of(32000, 16000) == 155


def _ptrs(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a is not None else None for a in arrays])


def test_refusals_come_before_any_device_call():
    """every refusal names its reason in sea_last_error; none of the messages is a HIP error (this test runs without a device)"""
    import speech_enhancement_amd as sea
    lib = sea.load()
    x = np.zeros(400, np.int16)
    s, t, fk = np.zeros(1, np.float64), np.zeros(1, np.int64), np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lens = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731

    def stoi(ref=_ptrs([x]), est=_ptrs([x]), lengths=lens(400), n=1, rate=16000, a=vp(s), b=vp(t), c=vp(fk)):
        return lib.sea_stoi_utterances(ref, est, lengths, n, rate, a, b, c, None)

    cases = {
        "n_utt": lambda: stoi(n=-1), "rate": lambda: stoi(rate=10000), "rate ": lambda: stoi(rate=0, n=0), "n_utt ": lambda: stoi(n=-1, rate=0),
        "NULL": lambda: stoi(ref=None), "NULL ": lambda: stoi(est=None), "NULL  ": lambda: stoi(lengths=None), "NULL   ": lambda: stoi(a=None),
        "NULL    ": lambda: stoi(b=None), "NULL     ": lambda: stoi(c=None),
        "samples": lambda: stoi(lengths=lens(-1)), "samples ": lambda: stoi(lengths=lens(2 ** 31)),
        "NULL buffer": lambda: stoi(est=_ptrs([None])), "NULL buffer ": lambda: stoi(ref=_ptrs([None])),
    }
    for what, call in cases.items():
        assert call() != 0, f"{what.strip()} was accepted"
        msg = lib.sea_last_error().decode()
        assert what.strip() in msg and "hip" not in msg, (what, msg)
    # an empty list is no error, whatever the pointers; nothing is written
    assert lib.sea_stoi_utterances(None, None, None, 0, 8000, None, None, None, None) == 0
    assert lib.sea_stoi_last_stage_ms(99) == -1.0 and lib.sea_stoi_last_stage_ms(-1) == -1.0
    with pytest.raises(ValueError):
        sea.stoi_utterances([x], [x[:-1]])
    with pytest.raises(ValueError):
        sea.stoi_utterances([x, x], [x])
