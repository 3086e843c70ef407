"""The Hu-Wang front half at 16 kHz on the 64-channel bank without a GPU: the host tables and the numpy model against what the
reference's own functions produced (tests/golden/hw64_*.npz, tools/gen_hw64_golden.py), the frame counts, the exported
symbols and the refusals that need no device."""
import ctypes
import os

import numpy as np
import pytest

from tests import hw64_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_hw64_tables_host", "sea_hw64_frames", "sea_hw64_workgroups_per_utterance", "sea_hw64_periphery_batch",
               "sea_hw64_correlogram_batch", "sea_hw64_frontend_batch", "sea_hw64_frontend")
KERNELS = (b"hw64_periphery_kernel", b"hw64_lowpass_kernel", b"hw64_correlogram_kernel")
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
    # argument for argument the 25-band calls; the periphery takes the nullable d_gout of sea_hw25_periphery_gout_batch
    for name in ("tables_host", "frames", "correlogram_batch", "frontend_batch", "frontend"):
        assert _lib.PROTOTYPES[f"sea_hw64_{name}"] == _lib.PROTOTYPES[f"sea_hw25_{name}"], name
    assert _lib.PROTOTYPES["sea_hw64_periphery_batch"] == _lib.PROTOTYPES["sea_hw25_periphery_gout_batch"]
    assert len(_lib.PROTOTYPES["sea_hw64_correlogram_batch"][1]) == 16 and len(_lib.PROTOTYPES["sea_hw64_frontend_batch"][1]) == 17
    blob = open(sea.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert k in blob, f"no code object for {k.decode()}"
    for name in ("hw64_tables", "hw64_periphery_batch", "hw64_split", "hw64_correlogram_batch", "hw64_frontend_batch", "hw64_frontend"):
        assert callable(getattr(sea, name))
    assert (sea.hw64.HW64_NCHAN, sea.hw64.HW64_DELAYS, sea.hw64.HW64_HOP) == (M.NCH, M.NDEL, M.HOP)


def test_host_tables_equal_the_reference_bit_for_bit(golden):
    import speech_enhancement_amd as sea
    t = sea.hw64_tables()
    for name in ("cf", "bw", "midEarCoeff", "lp"):
        assert M.same_bits(t[name], golden[name]), name
    assert np.array_equal(t["winsize"], golden["winsize"])
    assert t["winsize"][:8].tolist() == [1280, 978, 784, 647, 547, 470, 410, 360] and (t["winsize"][8:] == 320).all()
    assert int(t["winsize"].sum()) == 23396 and t["lp"].shape == (181,)
    assert t["cf"][0] == np.float32(50) and t["cf"][63] == np.float32(7999.9995)


def test_model_tables_equal_the_reference_and_the_library(golden, model_tables):
    import speech_enhancement_amd as sea
    for name in ("cf", "bw", "midEarCoeff", "lp"):
        assert M.same_bits(model_tables[name], golden[name]), name
    assert np.array_equal(model_tables["winsize"], golden["winsize"])
    t = sea.hw64_tables()
    for name in ("gain", "f1", "f2", "hair"):  # the fixture holds these only through hOut
        assert M.same_bits(model_tables[name], t[name]), name


def test_the_25_band_tables_did_not_move():
    """both banks' tables come from one body on the sampling rate: the 25-band ones still equal their own fixture"""
    import speech_enhancement_amd as sea
    from tests import hw25_model as M25
    g, t = M25.load_golden(), sea.hw25_tables()
    for name in ("cf", "bw", "midEarCoeff", "lp"):
        assert M25.same_bits(t[name], g[name]), name
    m = M25.tables()
    for name in ("gain", "f1", "f2", "hair"):
        assert M25.same_bits(t[name], m[name]), name


@pytest.mark.parametrize("k", ["a", "b", "c", "d"])
def test_model_equals_every_array_and_digest_of_the_fixture(golden, model_tables, model_b, k):
    got = model_b if k == "b" else M.frontend(golden[f"x_{k}"], model_tables)
    for name in ARRAYS:
        assert M.equals_golden(got[name], golden, name, k), f"input {k}: {name}"
    for name in M.LARGE:  # the digests the fixture stores are those of the arrays it stores
        assert np.array_equal(M.digest(golden[f"{name}_{k}"]), golden[f"sha256_{name}_{k}"]), f"input {k}: digest of {name}"


def test_fixture_covers_the_branches(golden):
    total, pitches = np.zeros(4, np.int64), set()
    for k in "abc":
        cross = golden[f"cross_hc_{k}"].astype(np.float64) > 0.985
        loud = golden[f"acf_hc_{k}"][:, :, 0] > np.float32(2500)
        assert len(golden[f"x_{k}"]) == 1770 and golden[f"pitch_{k}"].shape == (11,) and not np.isnan(golden[f"pRatio_{k}"]).any()
        o = np.array([(cross & loud).sum(), (~cross & loud).sum(), (cross & ~loud).sum(), (~cross & ~loud).sum()])
        assert (o >= 5).all(), (k, o)
        total += o
        pitches |= set(golden[f"pitch_{k}"].tolist())
    assert total.tolist() == [797, 982, 275, 58]
    assert min(pitches) == 32 and max(pitches) == 160
    assert len(golden["x_d"]) == 160 and golden["acf_hc_d"].shape == (1, 64, 201)
    for path in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if path.startswith("hw64_"):
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", path)) < 1 << 20, path


def test_a_reordered_acf_sum_is_told_apart(golden, model_tables, model_b):
    """the same terms added oldest sample first: the comparison above must be able to see the order"""
    other = M.acf(model_b["hOut"], model_tables["winsize"], reverse_steps=True)
    assert not M.equals_golden(other, golden, "acf_hc", "b")
    assert np.allclose(other, model_b["acf_hc"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("length,nframes", [(0, 0), (-5, 0), (159, 0), (160, 1), (161, 1), (319, 1), (320, 2), (1770, 11)])
def test_frames(length, nframes):
    from speech_enhancement_amd import _lib
    assert _lib.load().sea_hw64_frames(length) == nframes == M.frames(length)


def test_refusals_that_need_no_device():
    """null pointers and outputs that are inputs are refused before anything touches a device; an empty batch is no error"""
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    buf = [np.zeros(64, np.float32) for _ in range(12)]
    p = [b.ctypes.data_as(ctypes.c_void_p) for b in buf]
    assert lib.sea_hw64_periphery_batch(None, None, None, None, None, None, None, 0, None) == 0
    assert lib.sea_hw64_correlogram_batch(*([None] * 14), 0, None) == 0
    assert lib.sea_hw64_frontend_batch(*([None] * 15), -1, None) == 0
    assert lib.sea_hw64_workgroups_per_utterance(0) == 0 and lib.sea_hw64_workgroups_per_utterance(-3) == 0

    def refused(rc, word):
        msg = lib.sea_last_error().decode(errors="replace")
        assert rc != 0 and word in msg, msg

    refused(lib.sea_hw64_periphery_batch(p[0], p[1], None, None, p[3], p[4], None, 1, None), "null")
    refused(lib.sea_hw64_periphery_batch(p[0], p[1], p[1], None, p[3], p[4], None, 1, None), "of its own")
    refused(lib.sea_hw64_periphery_batch(p[0], p[1], p[2], p[0], p[3], p[4], None, 1, None), "of its own")
    corr = [p[0], p[1], p[2], p[3], p[4], None, None, p[5], p[6], p[7], p[8], p[9], None, None, 1, None]
    for i in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11):
        args = list(corr)
        args[i] = None
        refused(lib.sea_hw64_correlogram_batch(*args), "null")
    args = list(corr)
    args[7] = p[0]  # cross_hc is hout
    refused(lib.sea_hw64_correlogram_batch(*args), "of its own")
    args = list(corr)
    args[6] = p[9]  # acf_ev is mark
    refused(lib.sea_hw64_correlogram_batch(*args), "of its own")
    front = [p[10]] + corr
    args = list(front)
    args[12] = None  # mark
    refused(lib.sea_hw64_frontend_batch(*args), "null")
    args = list(front)
    args[1] = p[10]  # hout is the input
    refused(lib.sea_hw64_frontend_batch(*args), "of its own")
    refused(lib.sea_hw64_frontend(p[0], 0, *([None] * 9)), "L=0")
    refused(lib.sea_hw64_frontend(None, 160, *([None] * 9)), "null")
