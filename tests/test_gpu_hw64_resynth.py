"""The Hu-Wang resynthesis at 16 kHz on the 64-channel bank on the GPU (csrc/hw64_resynth_kernel.hip) against what the
reference's own resynthesis(), compiled against the 64-band header, produced (tests/golden/hw64_resynth_golden.npz) and, at the
shapes the fixture does not hold, against the numpy model that the CPU tests pin to that fixture (tests/hw64_resynth_model.py).
Every comparison is on the bits.

The library's calls take host memory.  The list forms are called through ctypes on output buffers that are filled with a
sentinel and one element longer than the utterance: the element past the end must keep the sentinel, every sample must be
written and the inputs must be unchanged.  No input is longer than 11900 samples."""
import ctypes

import numpy as np
import pytest

from tests import hw64_am_model as AM
from tests import hw64_model as M
from tests import hw64_resynth_model as RM

pytestmark = pytest.mark.gpu

NCH, HOP = 64, 160
SENT, SENT16 = np.float32(-7777.25), np.int16(-7777)
LENGTHS_A = (0, 159, 160, 161, 319, 320, 321, 3203)
LENGTHS_B = (1, 7, 63, 64, 65, 127, 128, 129)


def _lib():
    from speech_enhancement_amd import _lib
    return _lib, _lib.load()


def _ptrs(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays]) if arrays is not None else None


def _lens(xs):
    return (ctypes.c_long * max(len(xs), 1))(*[x.size for x in xs])


def _sentinel_outputs(xs, f32, i16):
    outs = [np.full(x.size + 1, SENT, np.float32) for x in xs] if f32 else None
    outs16 = [np.full(x.size + 1, SENT16, np.int16) for x in xs] if i16 else None
    return outs, outs16


def _checked(xs, outs, outs16):
    """the outputs without their last element, after it was found to hold the sentinel and every float sample to be written"""
    res = []
    for name, arrs, sent in (("f32", outs, SENT), ("i16", outs16, SENT16)):
        if arrs is None:
            res.append([None] * len(xs))
            continue
        for x, o in zip(xs, arrs):
            assert o[-1] == sent, f"{name}: the element past an utterance of {x.size} samples was written"
            if name == "f32":
                assert not (o[:-1] == sent).any(), f"a sample of an utterance of {x.size} samples was not written"
        res.append([o[:-1].copy() for o in arrs])
    return res


def resynth_list(xs, masks, threshold=0.0, f32=True, i16=False):
    """sea_hw64_resynth_utterances -> (floats, shorts, chunks) per utterance"""
    lib_mod, lib = _lib()
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    masks = [np.ascontiguousarray(m, np.float32).reshape(-1, NCH) for m in masks]
    assert [m.shape[0] for m in masks] == [x.size // HOP for x in xs]
    before = [a.copy() for a in xs + masks]
    outs, outs16 = _sentinel_outputs(xs, f32, i16)
    rc = lib.sea_hw64_resynth_utterances(_ptrs(xs), _lens(xs), _ptrs(masks), float(threshold), _ptrs(outs), _ptrs(outs16), len(xs))
    lib_mod.check(rc, "sea_hw64_resynth_utterances")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(xs + masks, before)), "an input changed"
    got, got16 = _checked(xs, outs, outs16)
    return got, got16, int(lib.sea_hw64_enhance_last_chunks())


def enhance_list(xs, i16=False):
    """sea_hw64_enhance_utterances -> dict of per-utterance lists, and chunks"""
    lib_mod, lib = _lib()
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    before = [a.copy() for a in xs]
    outs, outs16 = _sentinel_outputs(xs, True, i16)
    masks = [np.full((x.size // HOP, NCH), SENT, np.float32) for x in xs]
    pitch = [np.full(x.size // HOP, -7, np.int32) for x in xs]
    status = np.full(len(xs), -7, np.int32)
    rc = lib.sea_hw64_enhance_utterances(_ptrs(xs), _lens(xs), len(xs), _ptrs(outs), _ptrs(outs16), _ptrs(masks), _ptrs(pitch),
                                         status.ctypes.data_as(ctypes.c_void_p))
    lib_mod.check(rc, "sea_hw64_enhance_utterances")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(xs, before)), "an input changed"
    got, got16 = _checked(xs, outs, outs16)
    return dict(audio=got, shorts=got16, mask=masks, pitch=pitch, status=[int(v) for v in status],
                chunks=int(lib.sea_hw64_enhance_last_chunks()))


# ---- the fixture's cases -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fix():
    g = RM.load_golden()
    cases = RM.reference_cases(AM.load_golden())
    assert len(cases) == 19 and max(len(x) for x, _ in cases.values()) == 11900
    return dict(g=g, cases=cases)


@pytest.fixture(scope="module")
def ibm():
    """hw64_ibm on the five audio inputs, computed once"""
    import speech_enhancement_amd as sea
    xs = AM.audio_inputs()
    return {k: sea.hw64_ibm(xs[k]) for k in RM.AUDIO_CASES}


def test_every_fixture_case_through_the_single_form(fix):
    import speech_enhancement_amd as sea
    for k, (x, mask) in fix["cases"].items():
        got = sea.hw64_resynth(x, fix["g"][f"mask_{k}"].astype(np.float32))
        assert got.shape == x.shape and M.same_bits(got, fix["g"][f"out_{k}"]), f"{k}: not the reference's resynthesis"


def test_every_fixture_case_together_through_the_list_form(fix):
    keys = list(fix["cases"])
    xs = [fix["cases"][k][0] for k in keys]
    masks = [fix["g"][f"mask_{k}"].astype(np.float32) for k in keys]
    got, got16, chunks = resynth_list(xs, masks, i16=True)
    assert chunks == 1 and 0 < _lib()[1].sea_hw64_enhance_last_resynth_ms() < 1000, "the device time of the resynthesis launch"
    for u, k in enumerate(keys):
        assert M.same_bits(got[u], fix["g"][f"out_{k}"]), f"{k}: not the reference's resynthesis"
        assert np.array_equal(got16[u], RM.to_short(fix["g"][f"out_{k}"])), f"{k}: int16"
    import speech_enhancement_amd as sea
    res = sea.hw64_resynth_utterances(xs, masks, int16=True)
    assert res["chunks"] == 1 and all(M.same_bits(a, b) for a, b in zip(res["audio"], got))
    assert all(np.array_equal(a, b) for a, b in zip(res["shorts"], got16))


def test_enhance_equals_the_reference_end_to_end(fix, ibm, monkeypatch):
    import speech_enhancement_amd as sea
    g, am = fix["g"], AM.load_golden()
    xs = [AM.audio_inputs()[k] for k in RM.AUDIO_CASES]
    res = enhance_list(xs, i16=True)
    assert res["chunks"] == 1
    for u, k in enumerate(RM.AUDIO_CASES):
        one = sea.hw64_enhance(xs[u])
        for name, r in (("list", {n: res[n][u] for n in ("audio", "mask", "pitch", "status")}), ("single", one)):
            assert M.same_bits(r["audio"], g[f"out_a_{k}"]), f"{k}, {name}: audio in, enhanced audio out is not the reference's"
            assert np.array_equal(r["mask"], ibm[k]["mask"]) and np.array_equal(r["pitch"], ibm[k]["pitch"]), f"{k}, {name}"
            assert r["status"] == ibm[k]["status"] and r["status"] >> 16 == 0, f"{k}, {name}"
        assert np.array_equal(ibm[k]["mask"], am[f"mask_{k}"].astype(np.float32)), f"{k}: the mask is not createIBM's"
        assert np.array_equal(res["shorts"][u], RM.to_short(g[f"out_a_{k}"])), k
    # one utterance per chunk: the same bits
    monkeypatch.setenv("SEA_HW64_ENHANCE_SCRATCH_MB", "0")
    cut = enhance_list(xs)
    assert cut["chunks"] == 5 == len(sea.hw64_enhance_plan([len(x) for x in xs], 0)) - 1
    for u, k in enumerate(RM.AUDIO_CASES):
        assert M.same_bits(cut["audio"][u], res["audio"][u]) and np.array_equal(cut["mask"][u], res["mask"][u]), k
        assert np.array_equal(cut["pitch"][u], res["pitch"][u]) and cut["status"][u] == res["status"][u], k
    py = sea.hw64_enhance_utterances(xs[:2], int16=True)
    assert py["chunks"] == 2 and M.same_bits(py["audio"][1], res["audio"][1]) and np.array_equal(py["shorts"][0], res["shorts"][0])
    assert np.array_equal(py["mask"][0], res["mask"][0]) and np.array_equal(py["pitch"][1], res["pitch"][1]) and py["status"] == res["status"][:2]


# ---- mixed lengths against the model: random masks whose last row is set --------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """slices of p11900 at LENGTHS_A and LENGTHS_B with random 0 / 1 masks whose last row has units set, the model's result for
    each (computed once)"""
    rng = np.random.default_rng(11)
    p = AM.audio_inputs()["p11900"]
    t = M.tables()
    lengths = LENGTHS_A + LENGTHS_B
    xs = [np.ascontiguousarray(p[2000 + 37 * i:2000 + 37 * i + L]) for i, L in enumerate(lengths)]
    masks = [(rng.random((L // HOP, NCH)) < 0.5).astype(np.float32) for L in lengths]
    for m in masks:
        if len(m):
            m[-1, ::2] = 1
            m[-1, 63] = 1
    want = [RM.resynth(AM.gout(x, t), m, 0.0, t) if len(x) else np.zeros(0, np.float32) for x, m in zip(xs, masks)]
    assert any(len(w) and np.abs(w).max() > 40 for w in want), "the cases carry no signal"
    return dict(lengths=lengths, xs=xs, masks=masks, want=want)


def test_every_length_through_the_single_form(mixed):
    import speech_enhancement_amd as sea
    for L, x, m, want in zip(mixed["lengths"], mixed["xs"], mixed["masks"], mixed["want"]):
        got = sea.hw64_resynth(x, m)
        assert got.shape == (L,) and M.same_bits(got, want), f"L = {L}: not the model's resynthesis"
        if L < HOP:
            assert not got.any(), f"L = {L}: an utterance without a frame must give zeros"


def test_mixed_list_against_the_model_in_one_chunk_and_in_several(mixed, monkeypatch):
    import speech_enhancement_amd as sea
    lengths, xs, masks, want = (mixed[k] for k in ("lengths", "xs", "masks", "want"))
    got, got16, chunks = resynth_list(xs, masks, i16=True)
    assert chunks == 1
    for u, L in enumerate(lengths):
        assert got[u].shape == (L,) and M.same_bits(got[u], want[u]), f"L = {L}: not the model's resynthesis"
        assert np.array_equal(got16[u], RM.to_short(want[u])), f"L = {L}: int16"
    only16 = resynth_list(xs, masks, f32=False, i16=True)[1]
    assert all(np.array_equal(a, RM.to_short(w)) for a, w in zip(only16, want))
    # the same list under a budget of 1 MiB: several chunks, the same bits
    monkeypatch.setenv("SEA_HW64_ENHANCE_SCRATCH_MB", "1")
    cut, cut16, chunks = resynth_list(xs, masks, i16=True)
    assert chunks > 1 and chunks == len(sea.hw64_enhance_plan(lengths, 1 << 20, resynth_only=True)) - 1
    for u, L in enumerate(lengths):
        assert M.same_bits(cut[u], got[u]) and np.array_equal(cut16[u], got16[u]), f"L = {L}: the result depends on the cut"
    monkeypatch.setenv("SEA_HW64_ENHANCE_SCRATCH_MB", "0")
    each, _, chunks = resynth_list(xs, masks)
    assert chunks == len(lengths) and all(M.same_bits(a, b) for a, b in zip(each, got))


# ---- thresholds and mask values ------------------------------------------------------------------------------------------------
def test_thresholds_on_soft_masks(fix):
    xs = [RM.hand_input(i) for i in RM.HAND_INPUTS]
    masks = [RM.hand_mask("soft", len(x) // HOP) for x in xs]
    at0 = resynth_list(xs, masks, threshold=0.0)[0]
    at05 = resynth_list(xs, masks, threshold=0.5)[0]
    for u, i in enumerate(RM.HAND_INPUTS):
        assert M.same_bits(at0[u], fix["g"][f"out_h_{i}_soft"]), f"{i}: threshold 0 is the reference's mark > 0"
        assert M.same_bits(at05[u], RM.resynth_input(i, masks[u], 0.5)), f"{i}: threshold 0.5"
        assert M.same_bits(at05[u], RM.resynth_input(i, (masks[u] == np.float32(0.7)).astype(np.float32))), i
        assert not M.same_bits(at0[u], at05[u])


def test_nan_negative_zero_and_negative_marks_count_as_not_set():
    rng = np.random.default_rng(5)
    xs = [RM.hand_input(i) for i in RM.HAND_INPUTS]
    masks, cleaned = [], []
    for x in xs:
        m = (rng.random((len(x) // HOP, NCH)) < 0.4).astype(np.float32)
        odd = rng.integers(0, 4, m.shape)
        m[odd == 1] = np.nan
        m[odd == 2] = -0.0
        m[(odd == 3) & (m == 0)] = -1.0
        masks.append(m)
        with np.errstate(invalid="ignore"):
            cleaned.append((m > 0).astype(np.float32))
    got = resynth_list(xs, masks)[0]
    for u, i in enumerate(RM.HAND_INPUTS):
        assert np.isnan(masks[u]).sum() > 50 and (np.signbit(masks[u]) & (masks[u] == 0)).sum() > 50 and (masks[u] == -1).sum() > 50
        assert np.isnan(masks[u][:, 32:]).sum() > 20, "marks that are not set in the upper half of the ballot"
        assert M.same_bits(got[u], RM.resynth_input(i, masks[u])), f"{i}: NaN / -0.0 / negative marks"
        assert M.same_bits(got[u], RM.resynth_input(i, cleaned[u])), i
        assert np.isfinite(got[u]).all()


def test_a_single_inf_sample_against_the_model(fix):
    """Inf enters the filter state for good: every later gOut is NaN, and so is all of the second pass but the sample it starts
    from; a weight of zero does not hide it (0 * NaN), as in the reference's literal arithmetic"""
    x = RM.hand_input("w4096")[:2048].copy()
    x[1500] = np.inf
    t = M.tables()
    mask = RM.hand_mask("checker", len(x) // HOP)
    with np.errstate(all="ignore"):
        want = RM.resynth(AM.gout(x, t), mask, 0.0, t)
    got, got16, _ = resynth_list([x, RM.hand_input("t3200")], [mask, RM.hand_mask("checker", 20)], i16=True)
    assert np.isnan(want).sum() >= len(x) - 1 and M.same_bits(got[0], want)
    assert np.array_equal(got16[0], RM.to_short(want)) and not got16[0].any()
    assert M.same_bits(got[1], fix["g"]["out_h_t3200_checker"]), "the neighbour of the utterance with the Inf"


def test_int16_output_is_the_x86_conversion(fix):
    """t3200 under a mask of ones reaches 62477: samples beyond +-32767 wrap as the x86-64 (short) cast does"""
    want = [fix["g"]["out_h_t3200_ones"], fix["g"]["out_h_w4096_single"]]
    xs = [RM.hand_input("t3200"), RM.hand_input("w4096")]
    masks = [RM.hand_mask("ones", 20), RM.hand_mask("single", 25)]
    got, got16, _ = resynth_list(xs, masks, i16=True)
    for u in range(2):
        assert M.same_bits(got[u], want[u]) and got16[u].dtype == np.int16
        assert np.array_equal(got16[u], RM.to_short(want[u])), "int16 is not the x86 conversion of the float output"
    wrapped = np.abs(want[0]) > 32768
    assert wrapped.sum() == 76 and np.abs(want[1]).max() < 32767, "the reference's own floats: 76 samples of the fixture wrap"
    assert not np.array_equal(got16[0][wrapped], np.clip(np.trunc(want[0][wrapped]), -32768, 32767).astype(np.int16)), "saturated"


# ---- the single forms, the Python layer, refusals --------------------------------------------------------------------------------
def test_single_forms_equal_the_list_forms_of_one_utterance(fix, ibm):
    import speech_enhancement_amd as sea
    x = RM.hand_input("t3200")
    soft = RM.hand_mask("soft", 20)
    for thr in (0.0, 0.5):
        assert M.same_bits(sea.hw64_resynth(x, soft, threshold=thr), resynth_list([x], [soft], threshold=thr)[0][0]), thr
    xa = AM.audio_inputs()["lo"]
    one, lst = sea.hw64_enhance(xa), enhance_list([xa])
    assert M.same_bits(one["audio"], lst["audio"][0]) and np.array_equal(one["mask"], lst["mask"][0])
    assert np.array_equal(one["pitch"], lst["pitch"][0]) and one["status"] == lst["status"][0] and lst["chunks"] == 1
    # silence, short and empty inputs
    z = sea.hw64_enhance(np.zeros(3200, np.float32))
    assert z["audio"].shape == (3200,) and not z["audio"].any(), "gOut of silence is zero, whatever the mask"
    assert z["mask"].shape == (20, NCH) and np.array_equal(z["mask"], sea.hw64_ibm(np.zeros(3200, np.float32))["mask"])
    short = sea.hw64_enhance(xa[:159])
    assert short["audio"].shape == (159,) and not short["audio"].any() and short["mask"].shape == (0, NCH)
    assert not sea.hw64_resynth(xa[:159], np.zeros((0, NCH), np.float32)).any()
    empty = sea.hw64_enhance(np.zeros(0, np.float32))
    assert empty["audio"].shape == (0,) and empty["status"] == 0
    assert sea.hw64_resynth(np.zeros(0, np.float32), np.zeros((0, NCH), np.float32)).shape == (0,)
    lst = enhance_list([xa[:159], np.zeros(0, np.float32), xa])
    assert not lst["audio"][0].any() and lst["status"][:2] == [0, 0] and M.same_bits(lst["audio"][2], one["audio"])
    assert np.array_equal(lst["mask"][2], one["mask"])
    none = sea.hw64_enhance_utterances([])
    assert none["audio"] == [] and none["chunks"] == 0
    with pytest.raises(sea.SeaError):
        sea.hw64_resynth(x, soft[:19])


def test_null_buffers_are_refused():
    _, lib = _lib()
    x = RM.hand_input("t3200")
    m = RM.hand_mask("ones", 20)
    out = np.zeros(x.size, np.float32)
    lens = _lens([x])
    assert lib.sea_hw64_resynth_utterances(_ptrs([x]), lens, _ptrs([m]), 0.0, None, None, 1) != 0, "no output at all"
    assert lib.sea_hw64_resynth_utterances(None, lens, _ptrs([m]), 0.0, _ptrs([out]), None, 1) != 0
    assert lib.sea_hw64_resynth_utterances(_ptrs([x]), lens, None, 0.0, _ptrs([out]), None, 1) != 0, "frames without a mask"
    assert lib.sea_hw64_resynth_utterances(_ptrs([x]), (ctypes.c_long * 1)(-1), _ptrs([m]), 0.0, _ptrs([out]), None, 1) != 0
    assert lib.sea_hw64_resynth_utterances(None, None, None, 0.0, None, None, 0) == 0, "n_utt <= 0 is no work"
    status = np.zeros(1, np.int32)
    sp = status.ctypes.data_as(ctypes.c_void_p)
    assert lib.sea_hw64_enhance_utterances(_ptrs([x]), lens, 1, None, None, None, None, sp) != 0
    assert lib.sea_hw64_enhance_utterances(_ptrs([x]), lens, 1, _ptrs([out]), None, None, None, None) != 0, "no status"
    assert lib.sea_hw64_enhance_utterances(_ptrs([x]), lens, 1, _ptrs([out]), None, None, None, sp) == 0, "masks and pitch are optional"
    import speech_enhancement_amd as sea
    whole = sea.hw64_enhance(x)
    assert M.same_bits(out, whole["audio"]) and status[0] == whole["status"]


# ---- the edge set ------------------------------------------------------------------------------------------------------------
def test_edge_set_through_resynthesis_and_the_host_forms():
    """The edge set's audio (tests/test_hw_edge_coverage_cpu.py: edc, and ewhole with units in its last frame) against
    tests/golden/hw64_edge_golden.npz, bit for bit: resynthesis of the expected mask in one batch after a fixture input, then
    once end to end through the host forms (sea_hw64_ibm, sea_hw64_enhance_utterances), whose mask and pitch are createIBM's
    and whose audio is the resynthesis of that mask.  At this bank the reference finds a segment in edc and the fixture holds
    all of its arrays; tests/hw_edge.source would take the models' where it did not, as at 25 bands."""
    import speech_enhancement_amd as sea
    from tests import hw_edge as E
    e, am = E.load("hw64"), AM.load_golden()
    keys = list(E.AUDIO)
    src = [E.source("hw64", k) for k in keys]
    assert keys == ["edc", "ewhole"] and ("status_edc" in src[0]) == False and "status_ewhole" not in src[1]
    assert e["mask_ewhole"][-1].any() and np.abs(e["out_ewhole"]).max() > 1000
    xs = [am["x_w4096"]] + [s[f"x_{k}"] for s, k in zip(src, keys)]
    masks = [am["mask_w4096"].astype(np.float32)] + [s[f"mask_{k}"].astype(np.float32) for s, k in zip(src, keys)]
    want = [RM.load_golden()["out_a_w4096"]] + [s[f"out_{k}"] for s, k in zip(src, keys)]
    got = resynth_list(xs, masks)[0]
    tally = E.Tally("hw64 resynthesis, edge audio in one batch")
    for u, w in enumerate(want):
        tally.add(got[u], w, f"utterance {u}")
    tally.done()
    tally = E.Tally("hw64 host forms, edge audio end to end")
    res = enhance_list(xs[1:])
    enhs = [{n: res[n][i] for n in ("audio", "mask", "pitch", "status")} for i in range(len(keys))]
    for k, s, x, enh in zip(keys, src, xs[1:], enhs):
        ibm = sea.hw64_ibm(x)
        for name, r in (("ibm", ibm), ("enhance", enh)):
            if f"status_{k}" in s:
                assert r["status"] == s[f"status_{k}"] == 0, f"{k} {name}: status {r['status']:#x}, expected no segment (0)"
            else:
                assert r["status"] >> 16 == 0 and r["status"] > 0, f"{k} {name}: status {r['status']:#x}"
            tally.add(r["mask"], s[f"mask_{k}"].astype(np.float32), f"{k} {name} mask")
            tally.add(r["pitch"], s[f"pitch_{k}"], f"{k} {name} pitch")
        tally.add(enh["audio"], s[f"out_{k}"], f"{k} enhanced audio")
    tally.done()
