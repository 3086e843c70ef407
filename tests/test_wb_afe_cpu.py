"""CPU tests of the wideband (16 kHz) feature chain's host side: the new symbols, the committed fixture
(tests/golden/wb_afe_golden.npz) against a live regeneration through the reference's own functions
(tests/wb_afe_reference.py), the conditions that fixture is there for, and the no-fallback rule."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wb_afe_golden.npz")
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import wb_afe_reference as A  # noqa: E402
from tests import wb_reference as W  # noqa: E402


def _need_reference():
    if not A.available():
        pytest.skip("oracle/_ref/libetsi_ref.so not built (the reference's sources are not on this machine)")


def test_wb_afe_symbols_are_declared_exported_and_prototyped():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    header = open(os.path.join(ROOT, "include", "sea_mi355x.h")).read()
    lib = ctypes.CDLL(sea.LIB_PATH)
    for name in ("sea_wb_denoise_batch_fd", "sea_wb_afe_features_batch"):
        assert name + "(" in header.replace(" (", "(") and hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert callable(sea.wb_afe_features_batch)
    blob = open(sea.LIB_PATH, "rb").read()
    for kernel in (b"ns_denoise_pipe_wb_fd_kernel", b"afe_wb_ceps_kernel", b"afe_wb_vad_kernel"):
        assert kernel in blob, kernel


def test_fixture_equals_a_live_regeneration():
    _need_reference()
    import gen_wb_afe_golden as G
    live = G.generate()
    with np.load(GOLD) as z:
        assert sorted(z.files) == sorted(live)
        for k in z.files:
            a, b = z[k], np.asarray(live[k])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), k


def test_fixture_meets_the_coverage_conditions_and_fits():
    """The quiet utterance takes and skips WaveProc's bypass and has PostProc's weight below 0, in [0, 1] and above 1, each on
    >= 10 % of its cepstral frames; it and the three wideband utterances of 3 s have both VAD values on >= 10 % of their emitted
    frames; the counts the file stores are those of its own arrays and of the reference run they were recorded from."""
    import gen_wb_afe_golden as G
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    n_utt = len(g["counts"])
    assert n_utt == 7 and G.QUIET == 6
    shares = G.coverage(g)
    assert len(shares) == 5 + 2 * 4
    for what, share in shares:
        assert share >= G.MIN_SHARE, f"{what}: {share:.3f} of the frames"
    for u in range(n_utt):
        nfr, nceps, nemit, nnull, nflag1, nbypass = (int(v) for v in g["counts"][u])
        f15 = g[f"feat15_{u}"]
        assert nfr == len(g[f"x{u}"]) // 160 and nceps == len(g[f"feat_cc{u}"]) == len(g[f"feat_pp{u}"]) == len(g[f"bypass{u}"])
        assert nemit == len(f15) and nflag1 == int((f15[:, 14] == 1).sum()) and nbypass == int(g[f"bypass{u}"].sum())
        assert set(np.unique(f15[:, 14])) <= {0.0, 1.0}
        assert nnull == min(int(g["onset"][u]), nfr) and not f15[:nnull].any()
        fo = int(g["first_out"][u])
        assert len(g[f"flags{u}"]) == (nfr - fo if fo >= 0 else 0) and nceps == max(len(g[f"flags{u}"]) - 2, 0)
    # the figures of the reference run the fixture was designed on
    assert g["counts"][:6].tolist() == [[100, 94, 94, 0, 62, 0], [100, 92, 94, 2, 62, 0], [300, 294, 294, 0, 226, 0],
                                        [300, 294, 294, 0, 212, 0], [303, 294, 297, 3, 235, 0], [4, 0, 6, 0, 0, 0]]
    for u in range(6):
        assert (A.pp_weight(g[f"feat_cc{u}"][:, 13]) > 1).all(), f"utterance {u} leaves the loud branch of PostProc"
    assert g["counts"][6].tolist() == [200, 194, 194, 0, 110, 117]
    w = A.pp_weight(g["feat_cc6"][:, 13])
    assert [int((w < 0).sum()), int(((w >= 0) & (w <= 1)).sum()), int((w > 1).sum())] == [38, 38, 118]
    assert os.path.getsize(GOLD) < 1 << 20


def test_waveproc_changes_the_cepstra_of_the_frames_it_runs_on():
    """What tests/test_gpu_wb_afe.py's cross-check (d) relies on, shown on the reference alone: a cepstral frame that took
    WaveProc's bypass has the cepstrum the plain wideband CompCeps gives (tests/wb_reference.py::trace), bit for bit; of the
    others, on the wideband utterances of 3 s, at least half differ (here: every one)."""
    _need_reference()
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    for u in (2, 3, 4, 6):
        plain = W.trace(g[f"x{u}"])["ceps"]
        cc, bypass = g[f"feat_cc{u}"], g[f"bypass{u}"]
        assert plain.shape == cc.shape
        differ = (plain.view(np.uint32) != cc.view(np.uint32)).any(axis=1)
        assert not differ[bypass].any(), f"utterance {u}: a bypassed frame's cepstrum changed"
        assert 2 * int(differ[~bypass].sum()) >= int((~bypass).sum()) > 0, (u, int(differ[~bypass].sum()), int((~bypass).sum()))


def test_wb_afe_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import speech_enhancement_amd as sea
    lib = sea.load()
    buf = np.zeros(4096, np.float32)
    meta = np.array([0, 1600], np.int64)
    cum = np.array([0, 4], np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.sea_wb_denoise_batch_fd(p(buf), p(buf), p(buf), p(meta), p(meta[1:]), None, p(buf), p(buf), p(buf), p(buf), p(buf),
                                     p(buf), 1600, 1, None)
    assert rc != 0 and lib.sea_last_error()
    rc = lib.sea_wb_afe_features_batch(p(buf), p(buf), p(buf), p(buf), p(meta), p(meta[1:]), p(buf), p(buf), p(cum), 4, p(buf),
                                       None, p(cum), p(buf), p(buf), None, 1, None)
    assert rc != 0 and lib.sea_last_error()
    with pytest.raises(sea.SeaError):
        sea._lib.check(rc, "sea_wb_afe_features_batch")
