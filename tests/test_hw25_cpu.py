"""The Hu-Wang front half on the 25-channel 8 kHz bank without a GPU: the host tables and the numpy model against what the
reference's own functions produced (tests/golden/hw25_golden.npz, tools/gen_hw25_golden.py), the frame and scratch counts,
and the exported symbols."""
import ctypes
import os

import numpy as np
import pytest

from tests import hw25_model as M

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_hw25_tables_host", "sea_hw25_frames", "sea_hw25_scratch_bytes", "sea_hw25_periphery_batch",
               "sea_hw25_correlogram_batch", "sea_hw25_frontend_batch", "sea_hw25_frontend")
KERNELS = (b"hw25_periphery_kernel", b"hw25_lowpass_kernel", b"hw25_correlogram_kernel")
ARRAYS = ("hOut", "hEv", "acf_hc", "acf_ev", "cross_hc", "cross_ev", "pitch", "pRatio", "mark")


@pytest.fixture(scope="module")
def golden():
    return M.load_golden()


@pytest.fixture(scope="module")
def model_tables():
    return M.tables()


@pytest.fixture(scope="module")
def model_b(golden, model_tables):
    return M.frontend(golden["x_b"], model_tables)


def test_the_new_symbols_are_exported_declared_and_built_for_gfx950():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
    assert len(_lib.PROTOTYPES["sea_hw25_correlogram_batch"][1]) == 16 and len(_lib.PROTOTYPES["sea_hw25_frontend_batch"][1]) == 17
    blob = open(sea.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert k in blob, f"no code object for {k.decode()}"
    for name in ("hw25_tables", "hw25_periphery_batch", "hw25_frontend_batch", "hw25_frontend"):
        assert callable(getattr(sea, name))


def test_host_tables_equal_the_reference_bit_for_bit(golden):
    import speech_enhancement_amd as sea
    t = sea.hw25_tables()
    for name in ("cf", "bw", "midEarCoeff", "lp"):
        assert M.same_bits(t[name], golden[name]), name
    assert np.array_equal(t["winsize"], golden["winsize"])
    assert t["winsize"][:3].tolist() == [400, 276, 206] and (t["winsize"][3:] == 200).all() and int(t["winsize"].sum()) == 5282


def test_model_tables_equal_the_reference_and_the_library(golden, model_tables):
    import speech_enhancement_amd as sea
    for name in ("cf", "bw", "midEarCoeff", "lp"):
        assert M.same_bits(model_tables[name], golden[name]), name
    assert np.array_equal(model_tables["winsize"], golden["winsize"])
    t = sea.hw25_tables()
    for name in ("gain", "f1", "f2", "hair"):  # the fixture holds these only through hOut
        assert M.same_bits(model_tables[name], t[name]), name


@pytest.mark.parametrize("k", ["a", "b", "c", "d"])
def test_model_equals_every_array_of_the_fixture(golden, model_tables, model_b, k):
    got = model_b if k == "b" else M.frontend(golden[f"x_{k}"], model_tables)
    for name in ARRAYS:
        assert M.same_bits(got[name], golden[f"{name}_{k}"]), f"input {k}: {name}"


def test_fixture_covers_the_branches(golden):
    total = np.zeros(4, np.int64)
    pitches = set()
    for k in "abc":
        cross = golden[f"cross_hc_{k}"].astype(np.float64) > 0.985
        energy = golden[f"acf_hc_{k}"][:, :, 0] > np.float32(2500)
        total += [(cross & energy).sum(), (~cross & energy).sum(), (cross & ~energy).sum(), (~cross & ~energy).sum()]
        pitches |= set(golden[f"pitch_{k}"].tolist())
        assert len(golden[f"x_{k}"]) == 1210
    assert (total >= 5).all(), total
    assert {53, 73, 80} <= pitches
    # the first frames cut the 400-sample window at the start of the signal, the last one at its end: later delays see fewer terms
    assert len(golden["x_d"]) == 80 and golden["acf_hc_d"].shape == (1, 25, 101)


def test_a_silent_stream_takes_the_zero_rms_branch(model_tables):
    """No input makes hOut zero (the hair cell fires spontaneously), so the fixture cannot hold a zero ACF; the correlogram of
    streams that ARE zero must leave the RMS undivided and give 0 / 0 = NaN for pRatio (tests/test_gpu_hw25.py runs this case
    through the kernel)."""
    stream = np.zeros((25, 163), np.float32)
    stream[5] = np.linspace(1, 60, 163, dtype=np.float32)
    a = M.acf(stream, model_tables["winsize"])
    pitch = M.global_pitch(a)
    cross, ratio = M.cross_corr(a), M.p_ratio(a, pitch)
    assert not a[:, :5].any() and a[:, 5].any()
    assert not cross.any() and not np.isnan(cross).any()
    assert np.isnan(ratio[:, :5]).all() and np.isnan(ratio[:, 6:]).all() and not np.isnan(ratio[:, 5]).any()


def test_a_reordered_acf_sum_is_told_apart(golden, model_tables, model_b):
    """the same terms added oldest sample first: the comparison above must be able to see the order"""
    other = M.acf(model_b["hOut"], model_tables["winsize"], reverse_steps=True)
    assert other.shape == model_b["acf_hc"].shape
    assert not M.same_bits(other, golden["acf_hc_b"])
    assert np.allclose(other, golden["acf_hc_b"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("length,nframes", [(0, 0), (79, 0), (80, 1), (81, 1), (159, 1), (160, 2), (1210, 15)])
def test_frames_and_scratch(length, nframes):
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    assert lib.sea_hw25_frames(length) == nframes == M.frames(length)
    # the correlogram keeps a frame's ACFs in LDS: no scratch at any size
    assert lib.sea_hw25_scratch_bytes((length + 7) // 8 * 8, 1) == 0
    assert lib.sea_hw25_scratch_bytes((length + 7) // 8 * 8 * 3, 3) == 0
