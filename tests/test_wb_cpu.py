"""CPU tests of the ETSI wideband (16 kHz) mode's host side: the tables the library computes against the reference's own
(read out of oracle/_ref/libetsi_ref.so at run time: no number is copied into a test), the committed fixture against a live
regeneration, and the no-fallback rule.  The header / export / prototype checks of tests/test_host_cpu.py pick the new
symbols up by themselves."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wb_golden.npz")

from tests import wb_reference as W  # noqa: E402


def _need_reference():
    if not W.available():
        pytest.skip("oracle/_ref/libetsi_ref.so not built (the reference's sources are not on this machine)")


def test_wb_symbols_are_declared_exported_and_prototyped():
    import ctypes
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    header = open(os.path.join(ROOT, "include", "sea_mi355x.h")).read()
    lib = ctypes.CDLL(sea.LIB_PATH)
    for name in ("sea_wb_denoise_batch", "sea_wb_scratch_bytes", "sea_wb_rows", "sea_wb_compceps_batch", "sea_wb_denoise",
                 "sea_wb_tables_host"):
        assert name + "(" in header.replace(" (", "(") and hasattr(lib, name) and name in _lib.PROTOTYPES, name
    blob = open(sea.LIB_PATH, "rb").read()
    for kernel in (b"wb_qmf_kernel", b"ns_denoise_pipe_wb_kernel", b"wb_hb_kernel", b"wb_specsub_kernel", b"compceps_wb_kernel"):
        assert kernel in blob, kernel


def test_qmf_tables_are_the_standards_integers_over_2_23():
    """Structure only, no reference: integer numerators over 2^23, symmetric low-pass, high-pass = the low-pass tap at the
    same index with the sign (-1)^(j+1)."""
    import speech_enhancement_amd as sea
    t = sea.wb_tables()
    lp, hp = t["qmfLp"].astype(np.float64), t["qmfHp"].astype(np.float64)
    num = lp * 2.0 ** 23
    assert np.array_equal(num, np.round(num)) and np.abs(num).max() < 2 ** 24
    assert np.array_equal(lp, lp[::-1])
    sign = np.where(np.arange(118) % 2 == 1, 1.0, -1.0)
    assert np.array_equal(hp, sign * lp)


def test_qmf_taps_equal_the_references_impulse_response():
    """Two unit impulses through the reference's own Do16kProcessing return all 118 taps of both filters."""
    _need_reference()
    import speech_enhancement_amd as sea
    lp, hp = W.qmf_taps()
    assert lp[0] * 2 ** 23 == 1584 and lp[58] * 2 ** 23 == 3562497 and np.array_equal(lp, lp[::-1])  # the driver read a filter
    t = sea.wb_tables()
    assert np.array_equal(t["qmfLp"].view(np.uint32), lp.view(np.uint32))
    assert np.array_equal(t["qmfHp"].view(np.uint32), hp.view(np.uint32))


def test_high_band_mel_filter_equals_the_references_windows():
    _need_reference()
    import speech_enhancement_amd as sea
    t = sea.wb_tables()
    wins = W.hp_mel_windows()
    assert len(wins) == 5
    for b in range(3):  # the two half bands at the ends are not used
        start, w = wins[b + 1]
        assert start == t["hpMelStart"][b] and len(w) == t["hpMelLen"][b]
        assert np.array_equal(w.view(np.uint32), t["hpMelW"][b][:len(w)].view(np.uint32))
        assert not t["hpMelW"][b][len(w):].any() and start + len(w) <= 65


def test_dct26_is_the_cosine_matrix():
    """InitDCTMatrix (13, 26) is private to the reference's CompCeps.c; against the formula, to float rounding (the GPU
    cepstra pin its bits)."""
    import speech_enhancement_amd as sea
    d = sea.wb_tables()["dct"]
    i, j = np.meshgrid(np.arange(1, 13), np.arange(26), indexing="ij")
    assert np.abs(d - np.cos(np.pi * i / 26.0 * (j + 0.5))).max() < 2e-7


def test_fixture_equals_a_live_regeneration():
    _need_reference()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_wb_golden as G
    live = G.generate()
    with np.load(GOLD) as z:
        assert sorted(z.files) == sorted(live)
        for k in z.files:
            a, b = z[k], np.asarray(live[k])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), k


def test_fixture_meets_the_high_band_vad_condition_and_fits():
    """Every wideband utterance of 3 s has the reference's high-band VAD in each of its three states for >= 5 % of its
    frames; the corpus utterances never leave 'idle'; the file stays below the largest older fixture and below 1 MiB."""
    with np.load(GOLD) as z:
        st = z["vad_states"]
        for u in (2, 3, 4):
            nfr = len(z[f"x{u}"]) // 160
            assert nfr >= 300 and (st[u] / nfr).min() >= 0.05, (u, st[u], nfr)
        for u in (0, 1):
            assert st[u][0] == 0 and st[u][1] == 0 and st[u][2] > 0
        assert len(z["x5"]) // 160 < 5 and z["first_out"][5] == -1
    assert os.path.getsize(GOLD) < min(1 << 20, os.path.getsize(os.path.join(ROOT, "tests", "golden", "ns_golden.npz")))


def test_wb_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import speech_enhancement_amd as sea
    with pytest.raises(sea.SeaError):
        sea.wb_denoise(np.ones(1600, np.int16))
