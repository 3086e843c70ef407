"""tests/launch_caps.py without a GPU: the parser finds every cap in csrc/capi.hip (a renamed constant fails here, not silently
in tests/test_gpu_launch_caps.py), and the helpers' arithmetic reproduces the launch code's formulas on hand-made cases."""
import numpy as np
import pytest

from tests import launch_caps as LC


@pytest.fixture(scope="module")
def caps():
    return LC.parse()


def test_parser_finds_every_cap(caps):
    assert caps == LC.Caps(cc_grid=16384, afe_grid=8192, frames_grid=8192, wb_cc_grid=16384, cc_slice_grid=16384, rfft_per_cu=16,
                           hw25_per_cu=8, hw25_clamp=1024, cc_tile=16, afe_tile=8, frames_tile=16)


def test_a_renamed_or_disagreeing_constant_is_an_error():
    with open(LC.CAPI) as f:
        text = f.read()
    for old, new in (("kCcGrid = 16384", "kCepsGrid = 16384"), ("ntile < 8192", "ntile < kFramesGrid"),
                     ("16LL * c->n_cu ? npair", "kWavesPerCu * c->n_cu ? npair"), ("per_utt > 1024 ? 1024", "per_utt > kMax ? kMax"),
                     ("(8 * c->n_cu + n_utt - 1)", "(kPerCu * c->n_cu + n_utt - 1)"),
                     ("nslot < 16384 ? nslot : 16384", "nslot < kGrid ? nslot : kGrid")):
        assert old in text, old
        with pytest.raises(LookupError):
            LC.parse(text.replace(old, new))
    # one of the four kAfeGrid definitions changed alone: they must agree
    assert text.count("kAfeGrid = 8192") == 4
    with pytest.raises(LookupError, match="disagree"):
        LC.parse(text.replace("kAfeGrid = 8192", "kAfeGrid = 4096", 1))
    with pytest.raises(LookupError, match="disagree"):
        LC.parse(text.replace("ntile < 8192 ? ntile : 8192", "ntile < 8192 ? ntile : 4096"))


def test_trips_of_a_grid_stride_loop():
    assert LC.trips(0, 1) == LC.Trips(1, 0, 0, 0, 0)
    assert LC.trips(5, 5) == LC.Trips(5, 5, 1, 0, 0)
    assert LC.trips(6, 5) == LC.Trips(5, 6, 2, 1, 0)
    assert LC.trips(13, 5) == LC.Trips(5, 13, 3, 5, 3)
    # items with holes (spare slots): 0, 1, 5, 6, 10 on a grid of 5 -> workgroup 0 three trips, workgroup 1 two
    assert LC.trips([0, 1, 5, 6, 10], 5) == LC.Trips(5, 5, 3, 2, 1)


def test_rfft_pairs_and_second_trip(caps):
    # npair = (n + 1) / 2, grid = min (npair, 16 n_cu)
    assert [LC.rfft_pairs(n) for n in (1, 2, 3, 256, 257)] == [1, 1, 2, 128, 129]
    assert LC.rfft_grid(257, 256, caps) == 129 and LC.rfft_grid(10 ** 6, 256, caps) == 4096 and LC.rfft_grid(10 ** 6, 4, caps) == 64
    for n_cu in (1, 4, 256, 304):
        n = LC.rfft_second_trip_frames(n_cu, caps)
        assert n == 32 * n_cu + 1
        assert LC.rfft_trips(n - 1, n_cu, caps).busiest == 1 and LC.rfft_trips(n, n_cu, caps) == LC.Trips(16 * n_cu, 16 * n_cu + 1, 2, 1, 0)
    # the size tests/test_gpu_launch_caps.py uses: 2 (2 * 16 n_cu) + 3 frames = 2 * cap + 2 pairs, the last one half empty
    t = LC.rfft_trips(2 * (2 * 16 * 256) + 3, 256, caps)
    assert t == LC.Trips(4096, 8194, 3, 4096, 2)


def test_compceps_frames_tiles(caps):
    assert [LC.frames_tiles(n, caps) for n in (1, 16, 17, 35)] == [1, 1, 2, 3]
    assert LC.frames_second_trip_frames(caps) == 16 * 8192 + 1
    assert LC.frames_trips(16 * 8192, caps) == LC.Trips(8192, 8192, 1, 0, 0)
    assert LC.frames_trips(16 * 8192 + 1, caps) == LC.Trips(8192, 8193, 2, 1, 0)
    assert LC.frames_trips(16 * (8192 + 100) + 5, caps) == LC.Trips(8192, 8293, 2, 101, 0)


def test_slot_arithmetic_by_hand():
    # capacities 0, 5, 16, 17, 40, 0 with T = 16: cum = 0 0 5 21 38 78 78; nslot = 78 / 16 + 6 = 10
    cum = np.array([0, 0, 5, 21, 38, 78, 78])
    assert LC.slot_count(cum, 16) == 78 // 16 + 6 == 10
    # base (u) = cum[u] / 16 + u
    assert LC.slot_base(cum, 16).tolist() == [0, 1, 2, 4, 6, 9, 10]
    slots, utt = LC.slot_tiles(cum, 16)
    # u1: one tile at slot 1; u2: one at 2 (slot 3 spare); u3: 17 rows = two tiles at 4, 5; u4: 40 rows = three at 6, 7, 8; slots 0, 9 spare
    assert slots.tolist() == [1, 2, 4, 5, 6, 7, 8] and utt.tolist() == [1, 2, 3, 3, 4, 4, 4]
    assert LC.slot_trips(cum, 16, 16384) == LC.Trips(10, 7, 1, 0, 0)
    assert LC.slot_trips(cum, 16, 4) == LC.Trips(4, 7, 2, 3, 0)  # workgroups 0: 4, 8; 1: 1, 5; 2: 2, 6; 3: 7
    assert LC.straddles(cum, 16, 5) == [3] and LC.straddles(cum, 16, 7) == [4] and LC.straddles(cum, 16, 6) == []
    # the same capacities with the feature chain's tile of 8: nslot = 78 / 8 + 6 = 15
    assert LC.slot_count(cum, 8) == 15 and LC.slot_base(cum, 8).tolist() == [0, 1, 2, 5, 8, 14, 15]
    assert LC.slot_tiles(cum, 8)[0].tolist() == [1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]
    assert LC.slot_second_trip_utterances(16384, 0, 16) == 16385 and LC.slot_second_trip_utterances(16384, 160, 16) == 16375


def test_slots_cover_every_row_once():
    rng = np.random.default_rng(5)
    for tile in (8, 16):
        cap = rng.integers(0, 70, 200)
        cap[::7] = 0
        cum = np.concatenate(([0], np.cumsum(cap)))
        slots, utt = LC.slot_tiles(cum, tile)
        assert len(set(slots.tolist())) == len(slots) and slots.max() < LC.slot_count(cum, tile)
        base = LC.slot_base(cum, tile)
        rows = np.minimum(cap[utt] - (slots - base[utt]) * tile, tile)
        assert (rows > 0).all() and np.array_equal(np.bincount(utt, weights=rows, minlength=len(cap)), cap)


def test_hw25_per_utt_formula(caps):
    # per_utt = ceil (8 n_cu / n_utt) clamped to 1 .. 1024
    assert LC.hw25_per_utt(1, 256, caps) == 1024 and LC.hw25_per_utt(2, 256, caps) == 1024 and LC.hw25_per_utt(3, 256, caps) == 683
    assert LC.hw25_per_utt(7, 256, caps) == 293 and LC.hw25_per_utt(1024, 256, caps) == 2 and LC.hw25_per_utt(2048, 256, caps) == 1
    assert LC.hw25_per_utt(2049, 256, caps) == 1 and LC.hw25_per_utt(65537, 256, caps) == 1 and LC.hw25_per_utt(2047, 256, caps) == 2
    assert LC.hw25_utterances_for(3, 256, caps) == 683 and LC.hw25_utterances_for(1, 256, caps) == 2048
    assert LC.hw25_utterances_for(3, 304, caps) == 811
    # 15 frames on three workgroups: five trips each; 8 frames: 3, 3, 2; one workgroup: all 15
    assert LC.hw25_trips([15, 8, 0, 1], 3) == LC.Trips(3, 24, 5, 6, 5)
    assert LC.hw25_trips([15], 1) == LC.Trips(1, 15, 15, 1, 1)
    assert LC.hw25_trips([2], 1024).busiest == 1
