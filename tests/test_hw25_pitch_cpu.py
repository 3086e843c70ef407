"""The numpy model of the Hu-Wang initial grouping and pitch tracking (tests/hw25_pitch_model.py) against what the reference's
own initGroup / pitchDtm produced (tests/golden/hw25_pitch_golden.npz, written by tools/gen_hw25_pitch_golden.py), array by
array and bit for bit; then the model's defined behaviour where the reference has none.  No GPU.

The audio cases go through the front-half model (tests/hw25_model.frontend, seconds per input): computed once per module."""
import numpy as np
import pytest

from tests import hw25_model as M
from tests import hw25_pitch_model as PM


@pytest.fixture(scope="module")
def golden():
    return PM.load_golden()


@pytest.fixture(scope="module")
def inputs():
    return PM.audio_inputs()


@pytest.fixture(scope="module")
def fronts(inputs):
    """the front half of every audio input, s included, from the model"""
    t = M.tables()
    return {k: M.frontend(x, t) for k, x in inputs.items()}


def _compare(got, golden, k):
    assert (got["status"] & 0xFFFF) == int(golden[f"nseg_{k}"]) and got["status"] >> 16 == 0, f"{k}: status {got['status']:#x}"
    for name in ("pitch",) + PM.PITCH_STAGES:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], golden[f"{name}_{k}"]), f"{k}: {name}"
    for name in ("grp",) + PM.GRP_STAGES:
        assert np.array_equal(got[name], golden[f"{name}_{k}"].astype(np.float32)), f"{k}: {name}"
    assert M.same_bits(got["pratio"], golden[f"pratio_{k}"]), f"{k}: pratio"


def test_the_inputs_are_the_fixtures(golden, inputs):
    for k in PM.AUDIO_CASES:
        assert M.same_bits(inputs[k], golden[f"x_{k}"]), k


@pytest.mark.parametrize("k", PM.AUDIO_CASES)
def test_model_equals_the_reference_on_audio(golden, fronts, k):
    fr = fronts[k]
    assert PM.crc32(fr["acf_hc"]) == int(golden[f"acfcrc_{k}"]), f"{k}: the FRONT half's ACF differs from the reference's"
    _compare(PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"]), golden, k)


def test_handmade_case(golden):
    got = PM.pitch_stage(*PM.handmade_case())
    _compare(got, golden, "h")
    want = np.zeros(36, np.int32)
    want[12], want[13:20], want[20] = 40, 70, 40
    assert got["status"] == 4 and np.array_equal(got["pitch"], want)
    _, _, mark = PM.handmade_case()
    plus = np.zeros_like(mark, dtype=bool)
    plus[13:20, 18:21] = True
    assert np.array_equal(got["grp"] > 0, plus) and np.array_equal(got["grp"] < 0, (mark > 0) & ~plus)


def _lr_after_the_vote(pitch):
    voiced = np.flatnonzero(pitch > 0)
    return [int(voiced[0]), int(voiced[-1])] if len(voiced) else [len(pitch), 0]


def test_lframe_is_taken_before_the_vote(golden):
    """v: frame 3 has + units, sumAuto finds delay 40 there and findPitch's vote zeroes it; lFrame is 3 all the same, so
    leftDevelope reaches frame 3 and gives it a pitch.  With lFrame from the frames that keep their pitch it would stay 0."""
    a = PM.hand_inputs("v")
    got = PM.pitch_stage(*a)
    _compare(got, golden, "v")
    assert golden["lrframe_v"].tolist() == [3, 12] and _lr_after_the_vote(golden["pitch_find2_v"]) == [4, 12]
    assert got["pitch_find2"][3] == 0 and got["pitch_left"][3] == 40 and got["pitch"][3] == 40 and got["pratio"][3].any()
    acf, _, _, _ = a
    pitch, lf, rf = PM.find_pitch(acf, got["grp_thetap"])
    assert [lf, rf] == [3, 12] and np.array_equal(pitch, golden["pitch_find2_v"])
    for k in PM.AUDIO_CASES + ("h", "x"):  # no other input separates the two: this one pins it
        assert golden[f"lrframe_{k}"].tolist() == _lr_after_the_vote(golden[f"pitch_find2_{k}"]), k


def test_cross_decides_a_bit(golden):
    """x: number2's forty-channel loop reads cross[5][20] as channel 25; with cross zero frame 5 stays unvoiced"""
    a = PM.hand_inputs("x")
    got = PM.pitch_stage(*a)
    _compare(got, golden, "x")
    assert got["pitch_check"][5] == 0 and got["pitch_left"][5] == 20
    assert PM.pitch_stage(*a[:3])["pitch_left"][5] == 0


def test_the_fixture_takes_the_branches_it_is_there_for(golden):
    """two voiced stretches in p with only the later one inside the longest segment's span; interpolated frames somewhere"""
    assert all(1 <= int(golden[f"nseg_{k}"]) <= PM.MAX_SEG for k in PM.AUDIO_CASES + tuple(PM.HAND_CASES))
    changed = [k for k in PM.AUDIO_CASES if not np.array_equal(golden[f"pitch_{k}"], golden[f"pitch_right_{k}"])]
    assert changed, "linearEstimate fills no frame on any input"
    assert any(not np.array_equal(golden[f"pitch_left_{k}"], golden[f"pitch_check_{k}"]) for k in PM.AUDIO_CASES)
    assert any(not np.array_equal(golden[f"pitch_right_{k}"], golden[f"pitch_left_{k}"]) for k in PM.AUDIO_CASES)


def _all_zero(got):
    return all(not got[name].any() for name in ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES)


def test_no_segment_gives_zeros(fronts):
    fr = fronts["s"]
    got = PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"])
    assert got["status"] == 0 and _all_zero(got) and got["pitch"].shape == (100,) and got["grp"].shape == (100, 25)


@pytest.mark.parametrize("rows", [0, 2, 3])
def test_few_rows(rows):
    """fewer than three rows hold no seed; three rows hold one per marked column"""
    acf = np.full((rows, 25, 101), 100, np.float32)
    acf[:, :, 45] = 700
    mark = np.ones((rows, 25), np.float32)
    got = PM.pitch_stage(acf, np.full((rows, 25), 0.99, np.float32), mark)
    assert got["pitch"].shape == (rows,) and got["grp"].shape == (rows, 25)
    if rows < 3:
        assert got["status"] == 0 and _all_zero(got)
    else:
        assert got["status"] == 1 and np.array_equal(got["pitch"], [45, 45, 45]) and (got["grp"] == 1).all()
        assert (got["pratio"] == 1).all()


def test_more_than_400_segments():
    acf, pratio, mark = PM.many_segments_case()
    units, seg_mark = PM.segmentation(mark)
    assert len(seg_mark) == 442 and len(units) == 442 * 3
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == (442 | PM.TOO_MANY_SEGMENTS) and _all_zero(got)
    mark[1 + 4 * 30:, :] = 0  # 30 blocks of 13 = 390 segments: within the reference's array
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == 390 and got["grp"].any()


def test_no_streak_reads_chan_mark_unset():
    got = PM.pitch_stage(*PM.no_streak_case())
    assert got["status"] == (1 | PM.CHANMARK_UNSET)
    assert got["pitch_find2"][1:11].tolist() == [30, 60] * 5 and not got["pitch_check"].any()
    assert not got["pitch_left"].any() and got["pitch_right"].any()
