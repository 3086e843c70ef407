"""The numpy model of the Hu-Wang AM labels and final grouping (tests/hw25_am_model.py) against what the reference's own
computeAM / finalSeg / createIBM produced (tests/golden/hw25_am_golden.npz, written by tools/gen_hw25_am_golden.py): gOut, the
AM pattern before and after its normalisation and sEng bit for bit, ratio within the fixture's ratio_tol, the labels, every
stage of finalSeg and the mask equal; the constants (N at powers of two, beta, the first twiddle stages); then the model's
defined behaviour where the reference has none.  No GPU."""
import numpy as np
import pytest

from tests import hw25_am_model as AM
from tests import hw25_model as M


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


def test_the_inputs_are_the_fixtures(golden, inputs):
    assert tuple(inputs) == AM.AUDIO_CASES
    for k, x in inputs.items():
        assert M.same_bits(x, golden[f"x_{k}"]), k
        assert (len(x) <= 4000 or k == "p12000") and (golden[f"pitch_{k}"] > 0).sum() >= 9
    assert len(inputs["w2048"]) == 2048 and len(inputs["w1600"]) == 1600


@pytest.mark.parametrize("k", AM.AUDIO_CASES)
def test_exact_arrays_equal_the_reference(golden, stages, k):
    got = stages[k]
    L = got["gout"].shape[1]
    idx = AM.sample_index(L)
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
    assert run.sum() >= 200 and np.array_equal(got["ratio"] != 0, run)
    rel = np.abs(got["ratio"][run].astype(np.float64) - ref[run]) / ref[run]
    print(f"{k}: largest relative difference of ratio {rel.max():.3g}, tolerance {tol:.3g}")
    assert rel.max() <= tol
    assert np.array_equal(got["amcrn"], golden[f"amcrn_{k}"].astype(np.float32)), f"{k}: AmCrn"


def test_no_fixture_unit_lies_in_the_tolerance_band(golden):
    tol = float(golden["ratio_tol"])
    assert 0 < tol < 1e-3 and int(golden["ratio_band_units"]) == 0
    for k in AM.AUDIO_CASES:
        r = golden[f"ratio_{k}"].astype(np.float64)
        assert not (np.abs(r[r != 0] - AM.THETAE) <= tol * AM.THETAE).any(), k


def _compare_final(got, golden, k):
    assert got["status"] == 0
    for name in AM.FINAL_STAGES + ("grp_final", "mask"):
        assert np.array_equal(got[name], golden[f"{name}_{k}"].astype(np.float32)), f"{k}: {name}"


@pytest.mark.parametrize("k", AM.AUDIO_CASES)
def test_final_grouping_equals_the_reference_on_audio(golden, k):
    got = AM.final_seg(golden[f"grp_{k}"], golden[f"amcrn_{k}"], golden[f"cross_ev_{k}"], golden[f"pratio_{k}"])
    _compare_final(got, golden, k)
    assert got["mask"].sum() > 100


@pytest.mark.parametrize("k", tuple(AM.HAND_CASES))
def test_final_grouping_equals_the_reference_on_handmade_arrays(golden, k):
    _compare_final(AM.final_seg(**AM.HAND_CASES[k]()), golden, k)


def test_handmade_cases_do_what_they_are_for(golden):
    # prune: each reSegmentation keeps its component of exactly 5 frames and drops the one of 4
    c = AM.hand_prune()
    g1, g2, g3 = (golden[f"{n}_prune"] for n in AM.FINAL_STAGES[:3])
    assert (g1[1:6, 2] == 2).all() and (g1[8:12, 2] == 0).all() and (g1[:, 4] == 0).all()
    assert (g2[2:7, 8] == 1).all() and (g2[9:13, 8] == -2).all()
    assert (g3[3:8, 14] == -1).all() and (g3[10:14, 14] == -2).all()
    assert c["grp"].shape[0] == 16
    # sweeps: both developes need more than two sweeps, forwards and backwards
    c = AM.hand_sweeps()
    assert 12 <= c["grp"].shape[0] <= 20
    g3, g4 = golden["final_reseg3_sweeps"].astype(np.int32), golden["final_dev_minus_sweeps"].astype(np.int32)
    for m, v, g in ((g3 == -2, -1, g3), ((c["amcrn"] == 1) & (g4 == 0), 1, g4)):
        a, b, d = g.copy(), g.copy(), g.copy()
        assert AM.develope(m, v, a) > 2 and AM.closure(m, v, b) > 2 and AM.closure(m, v, d, reverse=True) > 2
        assert np.array_equal(a, b) and np.array_equal(a, d), "develope's fixpoint depends on the sweep order"
    assert (golden["final_reseg3_sweeps"][2, 13:25] == -2).all() and (golden["final_dev_minus_sweeps"][2, 13:25] == -1).all()
    assert (golden["final_dev_minus_sweeps"][2, 1:12] == 0).all() and (golden["mask_sweeps"][2, 1:12] == 1).all()
    # minus2: units become -2 from both sides and then 1
    g2, g3, g5 = (golden[f"{n}_minus2"] for n in ("final_reseg2", "final_reseg3", "final_dev_plus"))
    assert (g2[1:4, 5] == -2).all() and (g3[2:6, 9] == -2).all() and (g5[1:4, 5] == 1).all() and (g5[2:6, 9] == 1).all()
    assert g3[5, 21] == -2 and g5[5, 21] == -1 and (g5[3:9, 20] == -1).all()
    assert not golden["mask_empty"].any()


def test_closure_form_of_develope_gives_the_same_final_grouping(golden):
    for k in AM.AUDIO_CASES[:3] + ("sweeps",):
        c = AM.HAND_CASES[k]() if k in AM.HAND_CASES else {n: golden[f"{n}_{k}"] for n in ("grp", "amcrn", "cross_ev", "pratio")}
        got = AM.final_seg(**c, grow=AM.closure)
        _compare_final(got, golden, k)


def test_constants(golden):
    assert np.array_equal(AM.n_at_pow2(), golden["n_at_pow2"])
    assert np.array_equal(golden["n_at_pow2"], np.arange(7, 18)), "the engine's SEA_HW25_N_AT_POW2 carries these"
    a, beta = AM.kaiser_constants()
    assert a == np.float32(40) and M.same_bits(np.float32(beta), np.float32(golden["beta"]))
    for name, direct in (("tw_fwd", 1), ("tw_inv", -1)):
        mine = np.concatenate([AM.twiddles(1 << (n - 1), direct) for n in range(1, 11)])
        assert M.same_bits(mine, golden[name]), name


def test_inverse_twiddles_are_the_conjugates(golden):
    assert np.array_equal(golden["tw_inv"][:, 0], golden["tw_fwd"][:, 0]) and np.array_equal(golden["tw_inv"][:, 1], -golden["tw_fwd"][:, 1])
    for n in (11, 14, 17):
        f, i = AM.twiddles(1 << n, 1), AM.twiddles(1 << n, -1)
        assert np.array_equal(f[:, 0], i[:, 0]) and np.array_equal(f[:, 1], -i[:, 1]), n


def test_fft_log2_away_from_powers_of_two():
    for k in range(8, 18):
        assert AM.fft_log2((1 << k) + 1) == k + 1 and AM.fft_log2((1 << k) - 1) == k
    assert AM.fft_log2(150000) == 18


def test_defined_behaviour():
    t = M.tables()
    z = AM.am_stage(np.zeros((25, 150001), np.float32), np.zeros(1875, np.int32))
    assert z["status"] == AM.AM_TOO_LONG and not z["amcrn"].any()
    x = (3000 * np.sin(2 * np.pi * 125 * np.arange(240) / 8000)).astype(np.float32)
    s = AM.am_stage(AM.gout(x[:160], t), np.array([50, 50], np.int32))
    assert s["status"] == 0 and not s["ampatt"].any() and not s["amcrn"].any()
    got = AM.final_seg(**AM.many_final_segments_case())
    assert got["status"] == AM.FINAL_TOO_MANY_SEGMENTS and not got["mask"].any() and not got["final_reseg1"].any()
    two = {k: v[:2] for k, v in AM.hand_minus2().items()}
    assert not AM.final_seg(**two)["mask"].any()
