"""The numpy model of the Hu-Wang AM labels and final grouping at 16 kHz on the 64-channel bank (tests/hw64_am_model.py: the
25-band model's functions at the 64-band constants, no literal rate or channel count) against what the reference's own
computeAM / finalSeg / createIBM produced when compiled against resyth_64sub_IBM/cpp/HuWang.h (tests/golden/hw64_am_golden.npz,
written by tools/gen_hw64_am_golden.py): gOut, the AM pattern before and after its normalisation and sEng bit for bit, ratio
within the fixture's ratio_tol, the labels, every stage of finalSeg and the mask equal; the tap bound the engine's buffers are
sized from; N at the powers of two; what each input and each hand-made case is there for; then the new symbols, prototypes
and exports, and what the C ABI settles before it touches a device.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import hw64_am_model as AM
from tests import hw64_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH, HOP = 64, 160
NEW_SYMBOLS = ("sea_hw64_am_scratch_bytes", "sea_hw64_am_batch", "sea_hw64_finalseg_scratch_bytes", "sea_hw64_finalseg_batch",
               "sea_hw64_ibm_scratch_bytes", "sea_hw64_ibm_batch", "sea_hw64_ibm")
KERNELS = (b"hw64_am_prepare_kernel", b"hw64_am_patt_kernel", b"hw64_am_fft_head_kernel", b"hw64_am_fft_stage_kernel",
           b"hw64_am_norm_kernel", b"hw64_am_rate_kernel", b"hw64_finalseg_kernel")


@pytest.fixture(scope="module")
def golden():
    return AM.load_golden()


@pytest.fixture(scope="module")
def inputs():
    return AM.audio_inputs()


@pytest.fixture(scope="module")
def stages(golden, inputs):
    """the AM stage of every audio input from the model, fed the reference's pitch; computed once"""
    t = M.tables()
    out = {}
    for k, x in inputs.items():
        g = AM.gout(x, t)
        out[k] = dict(AM.am_stage(g, golden[f"pitch_{k}"]), gout=g)
    return out


def _blocks(pitch, L):
    return [AM.block_mean_pitch(pitch, f) for f in range(2, L // HOP, 5)]


def test_the_inputs_are_the_fixtures_and_reach_what_they_are_for(golden, inputs):
    assert tuple(inputs) == AM.AUDIO_CASES
    for k, x in inputs.items():
        assert M.same_bits(x, golden[f"x_{k}"]), k
        assert len(x) <= 12000 and (golden[f"pitch_{k}"] > 0).sum() >= 9
        p = golden[f"pitch_{k}"]
        assert ((p == 0) | ((p >= 32) & (p <= 200))).all(), k
    L = {k: len(x) for k, x in inputs.items()}
    # N <= 12 keeps the FFT in LDS, N >= 13 does not; a length that is a power of two
    assert AM.fft_log2(L["p11900"]) == 14 and all(AM.fft_log2(L[k]) == 12 for k in ("w4096", "lo", "hi", "t16"))
    assert L["w4096"] == 4096
    # at least nine blocks of five frames; neither a multiple of five frames nor of the hop
    bl = _blocks(golden["pitch_p11900"], L["p11900"])
    assert len(bl) == 15 and (L["p11900"] // HOP) % 5 == 4 and L["p11900"] % HOP == 60
    assert bl[0] is None and bl[-1] is None and any(b is not None for b in bl), "no block without a voiced frame at either end"
    # the longest filters, whose window leaves the utterance at both ends, and the shortest
    lo = _blocks(golden["pitch_lo"], L["lo"])
    assert min(lo) > 195 and AM.filter_length(lo[0]) >= 1100 and AM.filter_length(lo[0]) // 2 > 0
    last = len(lo) - 1
    assert last * 5 * HOP + 5 * HOP + AM.filter_length(lo[last]) // 2 > L["lo"]
    hi = _blocks(golden["pitch_hi"], L["hi"])
    assert max(hi) <= 36 and min(hi) >= 32 and AM.filter_length(min(hi)) <= 190
    # AM labels in the channels above 40, and mask units there that only develope (m, 1) adds
    assert sum(int(golden[f"amcrn_{k}"][:, 40:].sum()) for k in inputs) > 500
    late = (golden["final_dev_plus_t16"][:, 40:] == 1) & (golden["final_dev_minus_t16"][:, 40:] == 0)
    assert late.any() and (golden["mask_t16"][:, 40:][late] == 1).all()


def test_linear_estimate_leaves_no_unvoiced_block_between_voiced_ones(golden):
    """why the fixture's audio has no such block (tests/hw64_am_model.py::audio_inputs), and that gap_pitch makes one"""
    for k in AM.AUDIO_CASES:
        p = golden[f"pitch_{k}"]
        v = np.flatnonzero(p > 0)
        inner = p[v[0]:v[-1] + 1]
        assert (inner > 0).all() or v[0] == 0, f"{k}: an unvoiced frame between voiced ones"
    bl = _blocks(AM.gap_pitch(40), 40 * HOP)
    assert bl[0] == 200 and bl[1] is None and bl[2] == 32 and bl[3] == 77 and bl[-1] is not None


@pytest.mark.parametrize("k", AM.AUDIO_CASES)
def test_exact_arrays_equal_the_reference(golden, stages, k):
    got = stages[k]
    L = got["gout"].shape[1]
    idx = AM.sample_index(L)
    assert got["gout"].shape[0] == NCH and len(idx) == AM.SAMPLES and idx[-1] == NCH * L - 1
    for name in ("gout", "ampatt", "am"):
        bad = np.flatnonzero(got[name].ravel()[idx].view(np.uint32) != golden[f"{name}_s_{k}"].view(np.uint32))
        assert not len(bad), f"{k}: {name} differs first at flat index {idx[bad[0]]}"
        assert np.array_equal(AM.channel_crcs(got[name]), golden[f"{name}_crc_{k}"]), f"{k}: {name} CRCs"
    assert M.same_bits(got["seng"], golden[f"seng_{k}"]), f"{k}: sEng"
    assert got["status"] == 0 and np.abs(got["ampatt"]).max() > 0


@pytest.mark.parametrize("k", AM.AUDIO_CASES)
def test_ratio_within_tolerance_and_labels_equal(golden, stages, k):
    got, ref = stages[k], golden[f"ratio_{k}"]
    tol = float(golden["ratio_tol"])
    run = ref != 0
    assert run.sum() >= 900 and np.array_equal(got["ratio"] != 0, run)
    rel = np.abs(got["ratio"][run].astype(np.float64) - ref[run]) / ref[run]
    print(f"{k}: largest relative difference of ratio {rel.max():.3g}, tolerance {tol:.3g}")
    assert rel.max() <= tol
    assert np.array_equal(got["amcrn"], golden[f"amcrn_{k}"].astype(np.float32)), f"{k}: AmCrn"


def test_ratio_tol_is_twice_the_models_largest_difference_and_no_unit_lies_in_its_band(golden, stages):
    tol = float(golden["ratio_tol"])
    worst = 0.0
    for k in AM.AUDIO_CASES:
        ref = golden[f"ratio_{k}"].astype(np.float64)
        run = ref != 0
        worst = max(worst, float((np.abs(stages[k]["ratio"][run].astype(np.float64) - ref[run]) / ref[run]).max()))
        assert not (np.abs(ref[run] - AM.THETAE) <= tol * AM.THETAE).any(), k
    assert tol == 2 * worst and 0 < tol < 1e-3 and int(golden["ratio_band_units"]) == 0


def test_tap_bound_holds_for_every_reachable_mean_pitch(golden):
    """SEA_HW64_AM_MAXTAPS and the 800 + fLength sample window are sized from kaiserPara's float arithmetic at mp = 200"""
    mps = AM.reachable_mean_pitches()
    assert mps[0] == 32 and mps[-1] == 200 and len(mps) > 1500
    lengths = [AM.filter_length(mp) for mp in mps]
    assert lengths == sorted(lengths), "fLength does not grow with mp"
    assert max(lengths) == AM.filter_length(200) == 1118 and all(n % 2 == 0 for n in lengths)
    assert max(lengths) + 1 == int(golden["max_taps"]) == 1119 <= AM.MAX_TAPS
    tables = open(os.path.join(ROOT, "speech_enhancement_amd", "csrc", "sea_tables.h")).read()
    assert f"SEA_HW64_AM_MAXTAPS = {AM.MAX_TAPS}" in tables
    assert (AM.MAX_TAPS + 5 * HOP + AM.MAX_TAPS) * 4 == 12160, "the pattern kernel's LDS"


def _compare_final(got, golden, k):
    assert got["status"] == 0
    for name in AM.FINAL_STAGES + ("grp_final", "mask"):
        assert got[name].shape[1] == NCH and np.array_equal(got[name], golden[f"{name}_{k}"].astype(np.float32)), f"{k}: {name}"


@pytest.mark.parametrize("k", AM.AUDIO_CASES)
def test_final_grouping_equals_the_reference_on_audio(golden, k):
    got = AM.final_seg(golden[f"grp_{k}"], golden[f"amcrn_{k}"], golden[f"cross_ev_{k}"], golden[f"pratio_{k}"])
    _compare_final(got, golden, k)
    assert got["mask"].sum() > 100


@pytest.mark.parametrize("k", tuple(AM.HAND_CASES))
def test_final_grouping_equals_the_reference_on_handmade_arrays(golden, k):
    _compare_final(AM.final_seg(**AM.HAND_CASES[k]()), golden, k)


def test_handmade_cases_do_what_they_are_for(golden):
    assert all(make()["grp"].shape[1] == NCH for make in AM.HAND_CASES.values())
    # prune: each reSegmentation keeps its component of exactly 5 frames and drops the one of 4
    g1, g2, g3 = (golden[f"{n}_prune"] for n in AM.FINAL_STAGES[:3])
    assert (g1[1:6, 2] == 2).all() and (g1[8:12, 2] == 0).all() and (g1[:, 4] == 0).all()
    assert (g2[2:7, 8] == 1).all() and (g2[9:13, 8] == -2).all()
    assert (g3[3:8, 14] == -1).all() and (g3[10:14, 14] == -2).all()
    # sweeps: both developes need more than two sweeps, forwards and backwards, and the closure is the sweep's fixpoint
    c = AM.hand_sweeps()
    g3, g4 = golden["final_reseg3_sweeps"].astype(np.int32), golden["final_dev_minus_sweeps"].astype(np.int32)
    for m, v, g in ((g3 == -2, -1, g3), ((c["amcrn"] == 1) & (g4 == 0), 1, g4)):
        a, b, d = g.copy(), g.copy(), g.copy()
        assert AM.develope(m, v, a) > 2 and AM.closure(m, v, b) > 2 and AM.closure(m, v, d, reverse=True) > 2
        assert np.array_equal(a, b) and np.array_equal(a, d), "develope's fixpoint depends on the sweep order"
    assert (golden["final_reseg3_sweeps"][2, 34:64] == -2).all() and (golden["final_dev_minus_sweeps"][2, 33:64] == -1).all()
    assert (golden["final_dev_minus_sweeps"][2, 1:31] == 0).all() and (golden["mask_sweeps"][2, 1:31] == 1).all()
    # minus2: units become -2 from both sides and then 1
    g2, g3, g5 = (golden[f"{n}_minus2"] for n in ("final_reseg2", "final_reseg3", "final_dev_plus"))
    assert (g2[1:4, 5] == -2).all() and (g3[2:6, 9] == -2).all() and (g5[1:4, 5] == 1).all() and (g5[2:6, 9] == 1).all()
    assert g3[5, 21] == -2 and g5[5, 21] == -1 and (g5[3:9, 20] == -1).all()
    assert not golden["mask_empty"].any()
    # wide: growth across channel 31 / 32 up to channel 63 and down from it, in both developes
    g3, g4, g5 = (golden[f"{n}_wide"] for n in ("final_reseg3", "final_dev_minus", "final_dev_plus"))
    assert (g4[3, 1:64] == 0).all() and (g5[3, :] == 1).all() and (g4[9, 0:63] == 0).all() and (g5[9, :] == 1).all()
    assert (g3[16, 0:62] == -2).all() and (g4[16, :] == -1).all() and (golden["mask_wide"][16] == 0).all()
    assert golden["mask_wide"][3].sum() == 64 and golden["mask_wide"][9].sum() == 64


def test_closure_form_of_develope_gives_the_same_final_grouping(golden):
    for k in AM.AUDIO_CASES[1:4] + ("sweeps", "wide"):
        c = AM.HAND_CASES[k]() if k in AM.HAND_CASES else {n: golden[f"{n}_{k}"] for n in ("grp", "amcrn", "cross_ev", "pratio")}
        got = AM.final_seg(**c, grow=AM.closure)
        _compare_final(got, golden, k)


def test_constants(golden):
    """N at the powers of two is what the 64-band build handed to hilbert; the twiddles and SEA_HW25_N_AT_POW2 depend on
    neither rate nor bank"""
    from tests import hw25_am_model as A25
    assert np.array_equal(AM.n_at_pow2(), golden["n_at_pow2"])
    assert np.array_equal(golden["n_at_pow2"], np.arange(7, 18)), "the engine's SEA_HW25_N_AT_POW2 carries these"
    a, beta = AM.kaiser_constants()
    assert a == np.float32(40) and M.same_bits(np.float32(beta), np.float32(golden["beta"]))
    g25 = A25.load_golden()
    for name in ("tw_fwd", "tw_inv", "n_at_pow2", "beta"):
        assert M.same_bits(np.asarray(golden[name]), np.asarray(g25[name])), f"{name} differs between the two builds"


def test_defined_behaviour():
    t = M.tables()
    z = AM.am_stage(np.zeros((NCH, 150001), np.float32), np.zeros(937, np.int32))
    assert z["status"] == AM.AM_TOO_LONG and not z["amcrn"].any()
    x = (3000 * np.sin(2 * np.pi * 125 * np.arange(480) / 16000)).astype(np.float32)
    s = AM.am_stage(AM.gout(x[:320], t), np.array([50, 50], np.int32))
    assert s["status"] == 0 and not s["ampatt"].any() and not s["amcrn"].any()
    g = AM.gout(x, t)
    assert AM.am_stage(g, np.array([0, 201, 0], np.int32))["status"] == AM.AM_BAD_PITCH
    ok = AM.am_stage(g, np.array([0, 200, 0], np.int32))
    assert ok["status"] == 0 and ok["ampatt"].any()
    got = AM.final_seg(**AM.many_final_segments_case())
    assert got["status"] == AM.FINAL_TOO_MANY_SEGMENTS and not got["mask"].any() and not got["final_reseg1"].any()
    assert got["mask"].shape[1] == NCH
    two = {k: v[:2] for k, v in AM.hand_minus2().items()}
    assert not AM.final_seg(**two)["mask"].any()


def test_the_new_symbols_are_declared_exported_and_built_for_gfx950():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "sea_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace("hw64", "hw25")], f"{name} does not mirror its 25-band namesake"
    blob = open(sea.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert k in blob, f"no code object for {k.decode()}"
    for name in ("hw64_am_batch", "hw64_finalseg_batch", "hw64_ibm_batch", "hw64_ibm"):
        assert callable(getattr(sea, name))
    assert issubclass(sea.Hw64AmResult, sea.Hw25AmResult) and issubclass(sea.Hw64MaskResult, sea.Hw25MaskResult)
    assert sea.Hw64AmResult.NCHAN == sea.Hw64MaskResult.NCHAN == 64 and sea.Hw25MaskResult.NCHAN == sea.Hw25AmResult.NCHAN == 25
    assert "computeAM onwards" not in header and "only resynthesis() is NOT built at 16 kHz" in header


def test_what_needs_no_device():
    """the scratch sizes and the size rule, an empty batch, null pointers and outputs that are inputs: all settled before
    anything touches a device"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    size = lambda total, n, chunk: up(4 * n) + 2 * up(total * NCH * 4 + 64) + 2 * up(total * 2 * chunk * 8 + 64)  # noqa: E731
    # 2048 bytes per padded sample: the rule cuts at 131 072, whatever the number of utterances
    for n in (1, 7):
        assert lib.sea_hw64_am_scratch_bytes(131072, n) == size(131072, n, 64)
        assert lib.sea_hw64_am_scratch_bytes(131073, n) == size(131073, n, 8)
    assert lib.sea_hw64_am_scratch_bytes(150000, 1) == size(150000, 1, 8), "a single long utterance takes the grouped path"
    assert lib.sea_hw64_finalseg_scratch_bytes(10, 2) == 4 * 10 * 6 * NCH + 64 and lib.sea_hw64_finalseg_scratch_bytes(-3, 1) == 64
    assert lib.sea_hw64_ibm_scratch_bytes(8000, 50, 1) > lib.sea_hw64_am_scratch_bytes(8000, 1) + 51 * NCH * 201 * 4
    assert lib.sea_hw64_am_batch(*([None] * 12), 0, None, 0, None) == 0
    assert lib.sea_hw64_finalseg_batch(*([None] * 12), 0, None) == 0
    assert lib.sea_hw64_ibm_batch(*([None] * 9), 0, 0, None, 0, None) == 0

    def refused(rc, word):
        msg = lib.sea_last_error().decode(errors="replace")
        assert rc != 0 and word in msg, msg

    buf = [np.zeros(64, np.float32) for _ in range(12)]
    p = [b.ctypes.data_as(ctypes.c_void_p) for b in buf]
    # sea_hw64_am_batch: gout, pitch, offsets, lengths, row_offsets, amcrn, ratio, seng, ampatt, am, status, scratch, total, order, n, stream
    args = [p[0], p[1], p[2], p[3], p[4], p[5], None, None, None, None, p[6], p[7], 64, None, 1, None]
    for i in (0, 1, 2, 3, 4, 5, 10, 11):
        a = list(args)
        a[i] = None
        refused(lib.sea_hw64_am_batch(*a), "null")
    for out, other in ((5, 0), (5, 1), (6, 5), (8, 0), (9, 8), (10, 5), (7, 6)):
        a = list(args)
        a[out] = p[8] if a[out] is None else a[out]
        a[other] = p[9] if a[other] is None else a[other]
        a[out] = a[other]
        refused(lib.sea_hw64_am_batch(*a), "must not be")
    a = list(args)
    a[12] = 0
    refused(lib.sea_hw64_am_batch(*a), "total_padded_samples")
    # sea_hw64_finalseg_batch: grp, amcrn, cross_ev, pratio, lengths, row_offsets, mask, grp_final, status, stages, scratch, order, n, stream
    args = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, p[7], None, p[8], None, 1, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 10):
        a = list(args)
        a[i] = None
        refused(lib.sea_hw64_finalseg_batch(*a), "null")
    for out, other in ((6, 0), (6, 1), (6, 2), (6, 3), (8, 6), (7, 6), (9, 8)):
        a = list(args)
        a[out] = a[other]
        refused(lib.sea_hw64_finalseg_batch(*a), "must not be")
    # sea_hw64_ibm_batch: in, offsets, lengths, row_offsets, mask, pitch, status, stages, scratch, total, rows, order, n, stream
    args = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], None, p[7], 64, 1, None, 1, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        a = list(args)
        a[i] = None
        refused(lib.sea_hw64_ibm_batch(*a), "null")
    for out, other in ((4, 0), (5, 4), (6, 4), (6, 5), (7, 4), (7, 6)):
        a = list(args)
        a[out] = a[other]
        refused(lib.sea_hw64_ibm_batch(*a), "must not be")
    a = list(args)
    a[9] = 0
    refused(lib.sea_hw64_ibm_batch(*a), "total_padded_samples")
    word = np.zeros(1, np.int32)
    refused(lib.sea_hw64_ibm(p[0], -1, None, None, word.ctypes.data_as(ctypes.c_void_p)), "L=-1")
    refused(lib.sea_hw64_ibm(None, 160, None, None, word.ctypes.data_as(ctypes.c_void_p)), "null")
    refused(lib.sea_hw64_ibm(p[0], 160, None, None, None), "null")
    word[0] = 99
    assert lib.sea_hw64_ibm(None, 0, None, None, word.ctypes.data_as(ctypes.c_void_p)) == 0 and word[0] == 0, "L = 0 is no work"
