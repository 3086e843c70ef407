"""The Hu-Wang resynthesis without a GPU: the numpy model (tests/hw25_resynth_model.py) against what the reference's own
resynthesis() produced (tests/golden/hw25_resynth_golden.npz, tools/gen_hw25_resynth_golden.py), bit for bit on every case; the
library's host tables against the model's; the text writer against the reference's file; the new symbols."""
import ctypes
import os
import zlib

import numpy as np
import pytest

from tests import hw25_am_model as AM
from tests import hw25_model as M
from tests import hw25_resynth_model as RM

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_hw25_resynth_tables_host", "sea_hw25_resynth_batch", "sea_hw25_enhance_batch", "sea_hw25_resynth",
               "sea_hw25_enhance", "sea_hw25_resynth_text_write")


@pytest.fixture(scope="module")
def golden():
    return RM.load_golden()


@pytest.fixture(scope="module")
def cases():
    return RM.reference_cases(AM.load_golden())


def test_the_cases_are_the_fixtures_and_stay_in_bounds(golden, cases):
    assert len(cases) == len(RM.AUDIO_CASES) + len(RM.HAND_INPUTS) * len(RM.HAND_MASKS) == 18
    for k, (x, mask) in cases.items():
        assert np.array_equal(golden[f"mask_{k}"], mask.astype(np.int8)), k
        assert golden[f"out_{k}"].shape == x.shape and golden[f"out_{k}"].dtype == np.float32, k
        assert RM.in_bounds(mask > 0, len(x)), f"{k}: the reference would write past weight[]"
    # t1640's last frame reaches exactly the last sample; m9 and r are out of the reference's bounds with createIBM's mask
    assert 80 * 19 + 119 == len(RM.hand_input("t1640")) - 1 and len(RM.hand_input("w2048")) % 80 == 48
    am = AM.load_golden()
    for k in RM.MODEL_ONLY_CASES:
        assert not RM.in_bounds(am[f"mask_{k}"] > 0, len(am[f"x_{k}"])), k
    assert set(RM.AUDIO_CASES) | set(RM.MODEL_ONLY_CASES) == set(AM.AUDIO_CASES)


def test_model_equals_the_reference_on_every_case(golden, cases):
    for k, (x, mask) in cases.items():
        got = RM.resynth_input(k.split("_")[1], mask)
        assert M.same_bits(got, golden[f"out_{k}"]), f"{k}: the model is not the reference's resynthesis"
        assert np.abs(got).max() > 100, k


def test_soft_mask_is_its_positive_part_at_threshold_zero(golden):
    for i in RM.HAND_INPUTS:
        soft = RM.hand_mask("soft", len(RM.hand_input(i)) // 80)
        assert set(np.unique(soft)) == {np.float32(0), np.float32(0.3), np.float32(0.7)}
        assert M.same_bits(RM.resynth_input(i, soft), golden[f"out_h_{i}_soft"])
        assert not M.same_bits(RM.resynth_input(i, soft, 0.5), golden[f"out_h_{i}_soft"])


def test_weights_follow_the_window_and_the_drop_rule():
    up, down = RM.ola_tables()
    assert up[0] == 0 and down[0] == 1 and down[80] < 1e-30 and down[119] > down[81] > 0, "the last 40 values rise again"
    # one set unit at frame 3 of 6: up on [160, 240), down on [240, 360)
    m = np.zeros((6, 25), bool)
    m[3, 5] = True
    w = RM.weights(m, 487)
    assert M.same_bits(w[5, 160:240], up.astype(np.float32)) and M.same_bits(w[5, 240:360], down.astype(np.float32))
    assert not w[5, :160].any() and not w[5, 360:].any() and not np.delete(w, 5, axis=0).any()
    # frame 0 has no rising half; the last frame's tail is cut at L
    m[:] = False
    m[0, 0] = m[5, 0] = True
    w = RM.weights(m, 487)
    assert M.same_bits(w[0, :120], down.astype(np.float32)) and M.same_bits(w[0, 400:487], down[:87].astype(np.float32))
    # three frames in a row: the sample 80 k + o sums down[80 + o], down[o], up[o] in that order, each sum rounded to float
    m[:] = False
    m[1:4, 2] = True
    w = RM.weights(m, 487)
    o = np.arange(40)
    want = (down[80 + o].astype(np.float32).astype(np.float64) + down[o]).astype(np.float32)
    want = (want.astype(np.float64) + up[o]).astype(np.float32)
    assert M.same_bits(w[2, 160:200], want)


def test_host_tables_equal_the_models():
    import speech_enhancement_amd as sea
    t = sea.hw25_resynth_tables()
    up, down = RM.ola_tables()
    assert M.same_bits(t["up"], up) and M.same_bits(t["down"], down)
    w = RM.weight_table()
    assert M.same_bits(t["w"], w), "the 640 weights"
    # bit 0 (frame k - 1) reaches only the first 40 positions of a hop
    assert np.array_equal(w[40:, 1::2], w[40:, 0::2]) and (w[:40, 1] > 0).sum() == 39 and not w[:, 0].any()
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    assert lib.sea_hw25_resynth_tables_host(None, None, None) == 0


def test_text_writer_gives_the_references_bytes(golden, tmp_path):
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    for k in RM.reference_cases(AM.load_golden()):
        out = golden[f"out_{k}"]
        path = tmp_path / f"{k}.txt"
        assert lib.sea_hw25_resynth_text_write(str(path).encode(), out.ctypes.data_as(ctypes.c_void_p), len(out)) == 0
        got = path.read_bytes()
        assert zlib.crc32(got) & 0xFFFFFFFF == int(golden[f"text_crc_{k}"]), k
        assert got == RM.text(out), k
        if k in RM.TEXT_CASES:
            assert got == golden[f"text_{k}"].tobytes(), k
    assert all(f"text_{k}" in golden for k in RM.TEXT_CASES)
    assert lib.sea_hw25_resynth_text_write(str(tmp_path / "no" / "such" / "dir.txt").encode(), None, 0) != 0
    assert lib.sea_hw25_resynth_text_write(str(tmp_path / "empty.txt").encode(), None, 0) == 0
    assert (tmp_path / "empty.txt").read_bytes() == b""


def test_short_conversion_is_the_x86_one():
    v = np.array([0.0, -0.0, 0.9, -0.9, 1.5, -1.5, 32767.4, 32768.0, -32768.9, -32769.0, 65536.0, 65537.9, 2147483520.0, 2147483648.0,
                  -2147483648.0, -2147483904.0, np.inf, -np.inf, np.nan, 1e20], np.float32)
    want = np.array([0, 0, 0, 0, 1, -1, 32767, -32768, -32768, 32767, 0, 1, -128, 0, 0, 0, 0, 0, 0, 0], np.int16)
    assert np.array_equal(RM.to_short(v), want)


def test_new_symbols_are_declared_and_exported():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
    assert b"hw25_resynth_kernel" in open(sea.LIB_PATH, "rb").read()
    assert "is not built" not in header
    for name in ("hw25_resynth_batch", "hw25_resynth", "hw25_enhance_batch", "hw25_enhance", "hw25_resynth_tables"):
        assert callable(getattr(sea, name))
