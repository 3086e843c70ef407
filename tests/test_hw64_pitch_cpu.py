"""The numpy model of the Hu-Wang initial grouping and pitch tracking at 16 kHz on the 64-channel bank
(tests/hw64_pitch_model.py) against what the reference's own initGroup / pitchDtm produced when compiled against the 64-band
header (tests/golden/hw64_pitch_golden.npz, written by tools/gen_hw64_pitch_golden.py), array by array and bit for bit; the
forty-channel bound of the Developes against a bound of 64; the model's defined behaviour where the reference has none; the
new symbols.  No GPU.

The audio cases go through the front-half model (tests/hw64_model.frontend, about ten seconds per input): computed once per
module."""
import ctypes
import os

import numpy as np
import pytest

from tests import hw64_model as M
from tests import hw64_pitch_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sea_hw64_pitch_scratch_bytes", "sea_hw64_pitch_waves_per_utterance", "sea_hw64_pitch_batch", "sea_hw64_pitch")
KERNELS = (b"hw64_pitch_max_kernel", b"hw64_pitch_segment_kernel", b"hw64_pitch_frame_kernel", b"hw64_pitch_regroup_kernel",
           b"hw64_pitch_track_kernel")
ALL = ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES


@pytest.fixture(scope="module")
def golden():
    return PM.load_golden()


@pytest.fixture(scope="module")
def tables():
    return M.tables()


def _compare(got, golden, k):
    assert (got["status"] & 0xFFFF) == int(golden[f"nseg_{k}"]) and got["status"] >> 16 == 0, f"{k}: status {got['status']:#x}"
    for name in ("pitch",) + PM.PITCH_STAGES:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], golden[f"{name}_{k}"]), f"{k}: {name}"
    for name in ("grp",) + PM.GRP_STAGES:
        assert got[name].shape[1] == 64 and np.array_equal(got[name], golden[f"{name}_{k}"].astype(np.float32)), f"{k}: {name}"
    assert M.same_bits(got["pratio"], golden[f"pratio_{k}"]), f"{k}: pratio"


def test_the_inputs_are_the_fixtures(golden):
    xs = PM.audio_inputs()
    for k in PM.AUDIO_CASES:
        assert M.same_bits(xs[k], golden[f"x_{k}"]) and 50 <= len(xs[k]) // PM.HOP <= 90, k
    assert (PM.NCH, PM.NDEL, PM.MIN_DELAY, PM.HOP, PM.STAGE_WORDS) == (64, 201, 32, 160, 133)
    assert os.path.getsize(PM.GOLDEN) < 1 << 20


@pytest.mark.parametrize("k", PM.AUDIO_CASES)
def test_model_equals_the_reference_on_audio(golden, tables, k):
    fr = M.frontend(golden[f"x_{k}"], tables)
    assert PM.crc32(fr["acf_hc"]) == int(golden[f"acfcrc_{k}"]), f"{k}: the FRONT half's ACF differs from the reference's"
    _compare(PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"]), golden, k)


@pytest.mark.parametrize("k", sorted(PM.HAND_CASES))
def test_model_equals_the_reference_on_the_handmade_arrays(golden, k):
    acf, pratio, mark = PM.hand_inputs(k)
    assert acf.shape[1:] == (64, 201) and pratio.shape == mark.shape == acf.shape[:2]
    _compare(PM.pitch_stage(acf, pratio, mark), golden, k)


@pytest.mark.parametrize("bound", PM.BOUND_NAMES)
def test_forty_channels_not_sixty_four(golden, bound):
    """Each of the four `chan<40` of leftDevelope / rightDevelope has a hand-made case whose pitch changes when the model moves
    that bound, and no other, to 64: the fixture (the reference, at 40) holds one value, the moved model the other.  Moving all
    four changes it too, so a port with 64 throughout fails the comparison with the fixture."""
    k, frame, at40, at64 = PM.SEPARATES[bound]
    a = PM.hand_inputs(k)
    stage = "pitch_left" if bound.startswith("left") else "pitch_right"
    assert int(golden[f"{stage}_{k}"][frame]) == at40 == int(golden[f"pitch_{k}"][frame]) and at40 != at64
    moved = PM.pitch_stage(*a, bounds={bound: 64})
    assert int(moved[stage][frame]) == at64 == int(moved["pitch"][frame])
    assert not np.array_equal(moved[stage], golden[f"{stage}_{k}"])
    assert int(PM.pitch_stage(*a, bounds=PM.ALL_64)["pitch"][frame]) == at64
    for other in PM.BOUND_NAMES:  # the case separates its own bound alone
        if other != bound:
            assert np.array_equal(PM.pitch_stage(*a, bounds={other: 64})["pitch"], golden[f"pitch_{k}"]), other
    _compare(PM.pitch_stage(*a), golden, k)  # and the switch leaves nothing behind
    # the units that decide it lie in channels 40..63
    assert (golden[f"grp_thetap_{k}"][frame, 40:] > 0).any() and (golden[f"grp_thetap_{k}"][frame, :40] > 0).any()


def test_the_fixture_takes_the_branches_it_is_there_for(golden):
    cases = PM.AUDIO_CASES + tuple(PM.HAND_CASES)
    assert all(1 <= int(golden[f"nseg_{k}"]) <= PM.MAX_SEG for k in cases)
    assert any(not np.array_equal(golden[f"pitch_{k}"], golden[f"pitch_right_{k}"]) for k in PM.AUDIO_CASES), "linearEstimate"
    assert any(not np.array_equal(golden[f"pitch_left_{k}"], golden[f"pitch_check_{k}"]) for k in PM.AUDIO_CASES)
    assert any(not np.array_equal(golden[f"pitch_right_{k}"], golden[f"pitch_left_{k}"]) for k in PM.AUDIO_CASES)
    assert sum(int((golden[f"grp_{k}"][:, 40:] > 0).sum()) for k in PM.AUDIO_CASES) > 100
    top = max(int(golden[f"pitch_{k}"].max()) for k in PM.AUDIO_CASES)
    assert 129 <= top <= 200, "no pitch above 128: the Developes' k2 never reaches its clamp at 200"
    # v: lFrame is taken before findPitch's vote
    voiced = np.flatnonzero(golden["pitch_find2_v"] > 0)
    assert golden["lrframe_v"].tolist() == [3, 12] and [int(voiced[0]), int(voiced[-1])] == [4, 12]
    assert golden["pitch_find2_v"][3] == 0 and golden["pitch_left_v"][3] == 40


def _all_zero(got):
    return all(not got[name].any() for name in ALL)


def _flat(rows):
    acf = np.full((rows, 64, 201), 100, np.float32)
    acf[:, :, 90] = 700
    return acf, np.full((rows, 64), 0.99, np.float32), np.ones((rows, 64), np.float32)


def test_no_segment_gives_zeros():
    acf, pratio, mark = _flat(9)
    mark[:] = 0
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == 0 and _all_zero(got) and got["pitch"].shape == (9,) and got["grp"].shape == (9, 64)
    mark[0::2] = 1  # marked units, none with both time neighbours marked
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == 0 and _all_zero(got)


@pytest.mark.parametrize("rows", [0, 2, 3, 5])
def test_few_rows(rows):
    """fewer than three rows hold no seed; from three rows on the marked block is one segment"""
    got = PM.pitch_stage(*_flat(rows))
    assert got["pitch"].shape == (rows,) and got["grp"].shape == (rows, 64)
    if rows < 3:
        assert got["status"] == 0 and _all_zero(got)
    else:
        assert got["status"] == 1 and np.array_equal(got["pitch"], [90] * rows) and (got["grp"] == 1).all()
        assert (got["pratio"] == 1).all()


def test_more_than_400_segments():
    acf, pratio, mark = PM.many_segments_case()
    units, seg_mark = PM.segmentation(mark)
    assert len(seg_mark) == 34 * 32 and len(units) == 34 * 32 * 3
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == (1088 | PM.TOO_MANY_SEGMENTS) and _all_zero(got)
    mark[1 + 4 * 12:, :] = 0  # 12 blocks of 32 = 384 segments: within the reference's array
    got = PM.pitch_stage(acf, pratio, mark)
    assert got["status"] == 384 and got["grp"].any()


def test_no_streak_reads_chan_mark_unset():
    got = PM.pitch_stage(*PM.no_streak_case())
    assert got["status"] == (1 | PM.CHANMARK_UNSET)
    assert got["pitch_find2"][1:11].tolist() == [40, 80] * 5 and not got["pitch_check"].any()
    assert not got["pitch_left"].any() and got["pitch_right"].any()


def test_the_new_symbols_are_declared_exported_and_built_for_gfx950():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "sea_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
    assert "SEA_HW64_STAGE_WORDS = 133" in header
    # the 25-band call without its d_cross_hc
    assert len(_lib.PROTOTYPES["sea_hw64_pitch_batch"][1]) == len(_lib.PROTOTYPES["sea_hw25_pitch_batch"][1]) - 1 == 14
    assert _lib.PROTOTYPES["sea_hw64_pitch"] == _lib.PROTOTYPES["sea_hw25_pitch"]
    assert _lib.PROTOTYPES["sea_hw64_pitch_scratch_bytes"] == _lib.PROTOTYPES["sea_hw25_pitch_scratch_bytes"]
    blob = open(sea.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert k in blob, f"no code object for {k.decode()}"
    for name in ("hw64_pitch_batch", "hw64_pitch", "hw64_pitch_waves_per_utterance"):
        assert callable(getattr(sea, name))
    assert sea.HW64_STAGE_WORDS == PM.STAGE_WORDS and issubclass(sea.Hw64PitchResult, sea.Hw25PitchResult)
    assert sea.Hw64PitchResult.NCHAN == 64 and sea.Hw25PitchResult.NCHAN == 25 and sea.Hw25PitchResult.STAGE_WORDS == 55


def test_what_needs_no_device():
    """the scratch size, an empty batch, null pointers and outputs that are inputs: all settled before anything touches a device"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    assert lib.sea_hw64_pitch_scratch_bytes(10, 2) == 4 * (2 * 800 + 10 * 193)
    assert lib.sea_hw64_pitch_scratch_bytes(-1, -1) == 0
    assert lib.sea_hw64_pitch_waves_per_utterance(0) == 0 and lib.sea_hw64_pitch_waves_per_utterance(-2) == 0
    assert lib.sea_hw64_pitch_batch(*([None] * 12), 0, None) == 0

    def refused(rc, word):
        msg = lib.sea_last_error().decode(errors="replace")
        assert rc != 0 and word in msg, msg

    buf = [np.zeros(64, np.float32) for _ in range(11)]
    p = [b.ctypes.data_as(ctypes.c_void_p) for b in buf]
    args = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], None, p[9], None, 1, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):
        a = list(args)
        a[i] = None
        refused(lib.sea_hw64_pitch_batch(*a), "null")
    for out, other in ((6, 2), (7, 1), (6, 7), (5, 0), (9, 6), (10, 7), (8, 3)):  # grp is mark, pratio is pratio_in, grp is pratio, ...
        a = list(args)
        a[out] = args[other]
        refused(lib.sea_hw64_pitch_batch(*a), "of its own")
    refused(lib.sea_hw64_pitch(p[0], 0, None, None, None, p[1]), "L=0")
    refused(lib.sea_hw64_pitch(None, 160, None, None, None, p[1]), "null")
    refused(lib.sea_hw64_pitch(p[0], 160, None, None, None, None), "null")
