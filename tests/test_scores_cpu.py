"""The objective scores without a GPU: the numpy model against the plain-C statement of the contract
(tests/score_model_driver.c) bit for bit, known answers, sea_lnf on the part of its range that only the scores reach, the derived
figures against math.log10 on exact integers, the conditions the inputs of tests/test_gpu_scores.py must meet, and the new
symbols and their refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import score_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_score_utterances", "sea_mask_score_utterances", "sea_score_last_chunks", "sea_score_last_stage_ms")
HOPS = (80, 160)


def _agree(refs, ests, hop, sanitize=False):
    model, driver = M.scores(refs, ests, hop), M.driver_scores(refs, ests, hop, sanitize)
    for u, (a, b) in enumerate(zip(model, driver)):
        assert M.same_scores(a, b), f"hop {hop}, utterance {u} of {len(refs[u])} samples: the numpy model and the C model differ"
    return model


# ---- the two statements of the contract -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_numpy_model_equals_the_c_model_bit_for_bit(hop):
    _agree(*M.length_cases(hop), hop)
    for name, (ref, est) in M.special_cases(hop).items():
        _agree([ref], [est], hop)
    for refs, ests in M.placement_lists(hop)[:2]:
        _agree(refs, ests, hop)


def test_c_model_is_clean_under_the_sanitizers():
    """the same driver at -O1 with -fsanitize=address,undefined, a stand-alone program, on the test inputs: the same bits"""
    for hop in HOPS:
        cases = M.special_cases(hop)
        refs, ests = [c[0] for c in cases.values()], [c[1] for c in cases.values()]
        lr, le = M.length_cases(hop)
        refs, ests = refs + lr[:12], ests + le[:12]
        for a, b in zip(M.driver_scores(refs, ests, hop), M.driver_scores(refs, ests, hop, sanitize=True)):
            assert M.same_scores(a, b)
    for t in M.MASK_THRESHOLDS:
        est, ideal = M.mask_cases(t, t)
        assert np.array_equal(M.driver_mask_counts(est, ideal, t, t), M.driver_mask_counts(est, ideal, t, t, sanitize=True))


@pytest.mark.parametrize("t_est,t_ideal", [(t, t) for t in M.MASK_THRESHOLDS] + [(0.5, M.MASK_THRESHOLDS[2])])
def test_mask_model_equals_the_c_model_and_its_inputs_fill_every_class(t_est, t_ideal):
    est, ideal = M.mask_cases(t_est, t_ideal)
    counts = M.mask_counts(est, ideal, t_est, t_ideal)
    assert np.array_equal(counts, M.driver_mask_counts(est, ideal, t_est, t_ideal))
    assert counts.sum(axis=1).tolist() == [64 * r for r in M.MASK_ROWS]
    share = counts.sum(axis=0) / counts.sum()
    print(f"thresholds {t_est}, {t_ideal}: n11, n10, n01, n00 = {counts.sum(axis=0).tolist()}, shares {np.round(share, 3).tolist()}")
    assert share.min() >= 0.10
    # the special values: equal to the threshold is off, the next float and +Inf are on, +-0 (no threshold here is negative),
    # -Inf and NaN off
    t = np.float32(t_est)
    row = np.float32([t, np.nextafter(t, np.float32(2)), 0.0, -0.0, np.inf, -np.inf, np.nan]).reshape(1, -1)
    pad = np.full((1, 64 - row.size), -np.inf, np.float32)
    one = M.mask_counts([np.concatenate([row, pad], axis=1)], [np.full((1, 64), np.inf, np.float32)], t_est, 0.0)[0]
    assert one.tolist() == [2, 0, 62, 0]


# ---- known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_known_answers(hop):
    import speech_enhancement_amd.scores as S
    L = hop * 71 + 5
    ref = np.random.default_rng(3).integers(-9000, 9001, L).astype(np.int16)
    ref[:2] = (1234, -4321)  # no frame is silent
    # est == ref: no noise at all; every frame at the upper clamp
    same = _agree([ref], [ref.copy()], hop)[0]
    srr = int(same["sums"][0])
    assert same["sums"].tolist() == [srr, srr, srr] and same["seg_frames"] == 70
    assert np.all(same["frame_db"] == 35.0) and same["seg_sum"] == 35.0 * 70
    assert S.snr_db(*same["sums"]) == math.inf and S.si_sdr_db(*same["sums"]) == math.inf
    # est == 0: the noise is the reference; d is ln (srr + 1) - ln (srr + 1), exactly 0, and the SNR 0 dB
    zero = _agree([ref], [np.zeros(L, np.int16)], hop)[0]
    assert zero["sums"].tolist() == [srr, 0, 0] and np.all(zero["frame_db"] == 0.0) and zero["seg_sum"] == 0.0
    assert S.snr_db(*zero["sums"]) == 0.0 and math.isnan(S.si_sdr_db(*zero["sums"]))
    # est = ref / 2 on even samples: N = Srr / 4 exactly, 20 log10 2
    even = (ref // 2 * 2).astype(np.int16)
    half = _agree([even], [(even // 2).astype(np.int16)], hop)[0]
    s = [int(v) for v in half["sums"]]
    assert s[0] == 4 * s[1] == 2 * s[2] and s[0] - 2 * s[2] + s[1] == s[1]
    assert abs(S.snr_db(*s) - 20 * math.log10(2)) <= 1e-12 and S.si_sdr_db(*s) == math.inf
    assert np.abs(half["frame_db"] - 20 * math.log10(2)).max() <= 1e-4  # the + 1 of both arguments is below 1e-9 here
    assert abs(half["seg_sum"] / half["seg_frames"] - 20 * math.log10(2)) <= 1e-4


@pytest.mark.parametrize("hop", HOPS)
def test_the_int16_extremes_against_python_integers(hop):
    """ref = -32768 and est = 32767 everywhere: one product is 2^30, three of them overflow a signed 32-bit accumulator, and a
    frame's n = 2 hop 65535^2 is the largest argument the second logarithm can meet (above 2^40 at hop 160)"""
    L = hop * 71 + 5
    got = _agree([np.full(L, -32768, np.int16)], [np.full(L, 32767, np.int16)], hop)[0]
    assert got["sums"].tolist() == [L * 2 ** 30, L * 32767 ** 2, -L * 32768 * 32767]
    srr, see, sre, n = M.frame_energies(np.full(L, -32768, np.int16), np.full(L, 32767, np.int16), hop)
    assert set(srr.tolist()) == {2 * hop * 2 ** 30} and set(n.tolist()) == {2 * hop * 65535 ** 2}
    assert 2 * hop * 65535 ** 2 < 2 ** 41 and (hop == 80 or 2 * hop * 65535 ** 2 > 2 ** 40)
    want = 10 * math.log10((2 * hop * 2 ** 30 + 1) / (2 * hop * 65535 ** 2 + 1))  # -6.0204 dB
    assert got["seg_frames"] == 70 and np.abs(got["frame_db"] - want).max() <= 1e-4


# ---- sea_lnf beyond the cochleagram's range -------------------------------------------------------------------------------------------
def test_lnf_is_within_two_ulps_on_the_range_only_the_scores_reach():
    """tests/test_dnn_cpu.py measures sea_lnf on [1, 2^39]; n + 1 reaches 2^41.  Every float of (2^39, 2^41], 2 x 2^23 of them,
    against the double log.  Measured: 0.513 ulps, at 0x1.69b04ep+39."""
    r = M.lnf_sweep()
    print(f"sea_lnf: {r['n']} arguments, largest error {r['max_ulp']:.6f} ulps at {r['at']}")
    assert r["n"] == 2 * 2 ** 23
    assert r["max_ulp"] <= 2.0


def test_the_constant_is_the_float_nearest_ten_over_ln_ten():
    assert M.C_DB == np.float32(10.0 / math.log(10.0)) and float(M.C_DB).hex() == "0x1.15f2ce0000000p+2"


# ---- the derived figures ------------------------------------------------------------------------------------------------------------
def test_derived_figures_against_log10_of_exact_integers():
    """10 log10 (a / b) here is one correctly rounded quotient of two ints, its logarithm and a product; the yardstick is
    10 (log10 a - log10 b) with math.log10 on the exact ints.  Both are a few rounded operations on values below 200 dB
    (|log10| <= 38 for ints below 2^126): within 1e-12 dB."""
    import speech_enhancement_amd.scores as S
    rng = np.random.default_rng(9)
    worst = 0.0
    for _ in range(2000):
        L = int(rng.integers(1, 2 ** 31))
        a, b = int(rng.integers(1, 2 ** 30)), int(rng.integers(0, 2 ** 30))
        srr, see = L * a, L * b + int(rng.integers(0, 1000))
        lim = math.isqrt(srr * see)
        sre = int(rng.integers(-lim, lim + 1))
        n, t = srr - 2 * sre + see, sre * sre
        dd = srr * see - t
        assert n >= 0 and dd >= 0
        if n > 0:
            worst = max(worst, abs(S.snr_db(srr, see, sre) - 10 * (math.log10(srr) - math.log10(n))))
        if t > 0 and dd > 0:
            worst = max(worst, abs(S.si_sdr_db(srr, see, sre) - 10 * (math.log10(t) - math.log10(dd))))
    print(f"derived figures: largest difference {worst:.3g} dB")
    assert worst <= 1e-12
    # the written rule for zero denominators
    assert S.snr_db(5, 5, 5) == math.inf and S.snr_db(0, 7, 0) == -math.inf and math.isnan(S.snr_db(0, 0, 0))
    assert S.si_sdr_db(4, 9, 6) == math.inf and S.si_sdr_db(4, 9, 0) == -math.inf and math.isnan(S.si_sdr_db(4, 0, 0))
    assert S.hit_fa(3, 1, 1, 3) == (0.75, 0.25, 0.5)
    assert math.isnan(S.hit_fa(0, 1, 0, 3)[0]) and math.isnan(S.hit_fa(1, 0, 1, 0)[1]) and math.isnan(S.hit_fa(0, 0, 0, 0)[2])
    assert S.score_frames(319) == 0 and S.score_frames(320) == 1 and S.score_frames(479) == 1 and S.score_frames(160, 80) == 1


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_random_gpu_cases_rarely_clamp_or_skip(hop):
    lists = [M.length_cases(hop)] + M.placement_lists(hop) + ([M.chunk_list(hop)] if hop == 160 else [])
    for which, (refs, ests) in enumerate(lists):
        frames = off = 0
        for m in M.scores(refs, ests, hop):
            db = m["frame_db"]
            frames += db.size
            off += int(np.count_nonzero(np.isnan(db) | (db == -10.0) | (db == 35.0)))
        print(f"hop {hop}, list {which}: {off} of {frames} frames clamped or skipped")
        assert frames > 0 and off <= 0.10 * frames
    assert M.edge_lengths(hop)[:7] == [0, 1, hop - 1, 2 * hop - 1, 2 * hop, 2 * hop + 1, 3 * hop]
    assert {M.frames_of(L, hop) for L in M.edge_lengths(hop)[7:]} == {62, 63, 64, 126, 127, 252, 253, 505}


@pytest.mark.parametrize("hop", HOPS)
def test_special_gpu_cases_are_what_their_names_say(hop):
    got = {name: M.scores([r], [e], hop)[0] for name, (r, e) in M.special_cases(hop).items()}
    assert got["silent reference"]["seg_frames"] == 0 and np.isnan(got["silent reference"]["frame_db"]).all()
    gaps = got["silent frames between loud ones"]
    assert np.flatnonzero(np.isnan(gaps["frame_db"])).tolist() == [0, 9, 10, 30, 62, 63, 69] and gaps["seg_frames"] == 63
    assert np.all(got["all clamped low"]["frame_db"] == -10.0) and np.all(got["all clamped high"]["frame_db"] == 35.0)
    assert got["all clamped high"]["sums"][0] != got["all clamped high"]["sums"][1]  # clamped, not noiseless
    assert np.all(got["identical"]["frame_db"] == 35.0)


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
    for kernel in (b"score_frames_kernelILi80E", b"score_frames_kernelILi160E", b"score_finish_kernel", b"mask_score_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    for name in ("score_utterances", "mask_scores", "dnn_score_utterances", "score_last_chunks", "score_frames"):
        assert callable(getattr(sea, name))
    makefile = open(os.path.join(ROOT, "speech_enhancement_amd", "csrc", "Makefile")).read()
    assert "score_kernel.hip" in makefile and "score_capi.hip" in makefile and "score_kernels.h" in makefile


def _ptrs(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data if a is not None else None for a in arrays])


def test_refusals_come_before_any_device_call():
    """every refusal names its reason in sea_last_error; none of the messages is a HIP error (this test runs without a device)"""
    import speech_enhancement_amd as sea
    lib = sea.load()
    x = np.zeros(400, np.int16)
    sums, seg, used = np.zeros(3, np.int64), np.zeros(1, np.float64), np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lens = lambda *v: (ctypes.c_long * len(v))(*v)  # noqa: E731

    def score(ref=_ptrs([x]), est=_ptrs([x]), lengths=lens(400), n=1, hop=160, s=vp(sums), g=vp(seg), k=vp(used)):
        return lib.sea_score_utterances(ref, est, lengths, n, hop, s, g, k, None)

    cases = {
        "n_utt": lambda: score(n=-1), "hop": lambda: score(hop=100), "hop ": lambda: score(hop=0, n=0),
        "NULL": lambda: score(ref=None), "NULL ": lambda: score(s=None), "NULL  ": lambda: score(g=None), "NULL   ": lambda: score(k=None),
        "samples": lambda: score(lengths=lens(-1)), "samples ": lambda: score(lengths=lens(2 ** 31)),
        "NULL buffer": lambda: score(est=_ptrs([None])),
    }
    m = np.zeros((2, 64), np.float32)
    counts = np.zeros(4, np.int64)
    rows = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def mask(est=_ptrs([m]), ideal=_ptrs([m]), n_rows=rows(2), n=1, te=0.5, ti=0.5, c=vp(counts)):
        return lib.sea_mask_score_utterances(est, ideal, n_rows, n, te, ti, c)

    cases.update({
        "n_utt ": lambda: mask(n=-1), "not finite": lambda: mask(te=math.nan), "not finite ": lambda: mask(ti=math.inf),
        "not finite  ": lambda: mask(te=-math.inf, n=0), "NULL    ": lambda: mask(ideal=None), "NULL     ": lambda: mask(c=None),
        "rows": lambda: mask(n_rows=rows(-1)), "NULL buffer ": lambda: mask(est=_ptrs([None])),
    })
    for what, call in cases.items():
        assert call() != 0, f"{what.strip()} was accepted"
        msg = lib.sea_last_error().decode()
        assert what.strip() in msg and "hip" not in msg, (what, msg)
    # an empty list is no error, whatever the pointers; nothing is written
    assert lib.sea_score_utterances(None, None, None, 0, 160, None, None, None, None) == 0
    assert lib.sea_mask_score_utterances(None, None, None, 0, 0.5, 0.5, None) == 0
    assert lib.sea_score_last_stage_ms(99) == -1.0
    with pytest.raises(ValueError):
        sea.score_utterances([x], [x[:-1]])
    with pytest.raises(ValueError):
        sea.mask_scores([m], [m[:1]])
