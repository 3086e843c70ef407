"""irm_target_kernel (csrc/irm_kernel.hip) against the float64 model of tests/irm_model.py on the hand-made streams of
tests/irm_cases.py, within irm_cases.IRM_TOL -- the tolerance tests/test_irm_cpu.py derives from what correct implementations make
of the same inputs, and the inputs that file shows able to see every misreading of the definition.

The [64][pitch] device layout is built here from the streams (no subband_batch); all cases of a window kind travel in one batch
through sea_irm_target_batch, on a sentinel-filled output with guard rows before and behind every utterance's rows, once with
zeros and once with 0x7fff in the padding columns L .. pitch-1.  NaN positions and the exact 0, 0.5 and 1 are exact; nothing but an
utterance's own rows is written; the inputs are not; an utterance shorter than a frame owns no row; the host form gives the batch
form's bits; a window kind outside 0..2 is refused before anything is written.

MEASURED on an MI355X, worst |device - model| per family (IRM_TOL 3.5e-6; the host restatement of the kernel's arithmetic
predicts 1.42e-7): tones 1.32e-7, ramped tones 1.42e-7, outside the band 1.32e-7, extremes 1.28e-7, real subbands 1.40e-7, silent 0;
host form 1.32e-7.  Against the float restatement: test_irm_target_vs_oracle 3.58e-7, test_trainset_batch_irm_vs_oracle 2.98e-7.
"""
import ctypes

import numpy as np
import pytest

from tests import irm_cases as C
from tests import irm_model as M

pytestmark = pytest.mark.gpu

SENT = -7777.25
GUARD = 3


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from speech_enhancement_amd import _lib
    return _lib, _lib.load()


def _launch(case_list, kind, pad_value=0):
    """sea_irm_target_batch on the packed cases -> (rc, [per utterance rows], the whole output with its guard rows, row offsets).
    Asserts that the inputs are unchanged and that every row outside the utterances' own still holds the sentinel."""
    import torch
    _, lib = _lib()
    pk = C.pack(case_list)
    pure, noise = pk["pure"].copy(), pk["noise"].copy()
    pure[pk["pad"]] = pad_value
    noise[pk["pad"]] = pad_value
    rows = pk["rows"]
    row_offsets = (GUARD + np.concatenate(([0], np.cumsum(rows + GUARD)[:-1]))).astype(np.int64)
    total = int(rows.sum()) + GUARD * (len(rows) + 1)
    dev = "cuda:0"
    d_pure, d_noise = torch.from_numpy(pure).to(dev), torch.from_numpy(noise).to(dev)
    d_off, d_len, d_row = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pk["offsets"], pk["lengths"], row_offsets))
    out = torch.full((total, 64), SENT, dtype=torch.float32, device=dev)
    rc = lib.sea_irm_target_batch(_ptr(d_pure), _ptr(d_noise), _ptr(d_off), _ptr(d_len), _ptr(d_row), _ptr(out), int(kind),
                                  len(case_list), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(d_pure.cpu().numpy(), pure) and np.array_equal(d_noise.cpu().numpy(), noise), "an input was written"
    assert np.array_equal(d_off.cpu().numpy(), pk["offsets"]) and np.array_equal(d_len.cpu().numpy(), pk["lengths"])
    assert np.array_equal(d_row.cpu().numpy(), row_offsets)
    own = np.zeros(total, bool)
    for o, r in zip(row_offsets, rows):
        own[o:o + r] = True
    assert np.all(host[~own] == np.float32(SENT)), f"rows {np.flatnonzero((host != np.float32(SENT)).any(axis=1) & ~own)[:8]} are no utterance's"
    return rc, [host[o:o + r] for o, r in zip(row_offsets, rows)], host, own


def _check(name, got, want, worst, fam):
    assert got.dtype == np.float32 and got.shape == want.shape, name
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN positions"
    assert not np.any(got == np.float32(SENT)), f"{name}: a row was not written"
    for sl, v in C.exact_values(name):
        if v is not None:
            assert np.all(got[:, sl] == np.float32(v)), f"{name}: not exactly {v}"
    if (~nan).any():
        d = float(np.abs(got[~nan].astype(np.float64) - want[~nan]).max())
        worst[fam] = max(worst.get(fam, 0.0), d)
        assert d <= C.IRM_TOL, f"{name}: |delta| {d:.3g} > IRM_TOL {C.IRM_TOL:.3g}"


@pytest.fixture(scope="module")
def case_list(oracle):
    return C.cases(oracle)


@pytest.fixture(scope="module")
def models(case_list):
    """computed once, shared, never changed"""
    return {name: M.irm(p, n, kind) for name, p, n, kind, _ in case_list}


@pytest.fixture(scope="module")
def batch_results(case_list):
    """name -> the batch form's rows, padding columns zero; every window kind in one batch of its own"""
    res = {}
    for kind in (0, 1, 2):
        mine = [c for c in case_list if c[3] == kind]
        rc, per_utt, _, _ = _launch(mine, kind)
        assert rc == 0
        res.update({c[0]: r for c, r in zip(mine, per_utt)})
    return res


def test_batch_form_is_the_model_within_irm_tol(case_list, models, batch_results):
    worst = {}
    assert len({c[3] for c in case_list}) == 3
    for name, _, _, _, fam in case_list:
        _check(name, batch_results[name], models[name], worst, fam)
    for fam, d in worst.items():
        print(f"IRM target, batch form, {fam}: worst |device - model| {d:.3g}   (IRM_TOL {C.IRM_TOL:.3g})")
    assert set(worst) >= {"tones", "ramped tones", "outside", "extremes", "real", C.SILENT}


def test_padding_columns_are_not_read(case_list, batch_results):
    """0x7fff in the columns L .. pitch-1 of every channel row: the same bits, guard rows and all"""
    for kind in (0, 1, 2):
        mine = [c for c in case_list if c[3] == kind]
        assert any(c[1].shape[1] % 8 for c in mine)
        rc, per_utt, _, _ = _launch(mine, kind, pad_value=0x7fff)
        assert rc == 0
        for c, r in zip(mine, per_utt):
            assert r.tobytes() == batch_results[c[0]].tobytes(), f"{c[0]}: the padding columns changed the result"


def test_utterances_shorter_than_a_frame_own_no_row(case_list, models, batch_results):
    """L = 319 and L = 0 between two normal utterances, at the C ABI: the call returns 0, both own zero rows, their neighbours'
    rows are the bits of before and no sentinel is lost (_launch asserts the guard rows)."""
    by = {c[0]: c for c in case_list}
    a, b = by["tones F=17 tail=5 w=1"], by["ramped tones F=65 tail=159 w=1"]
    short = ("L = 319", a[1][:, :319].copy(), a[2][:, :319].copy(), 1, "short")
    empty = ("L = 0", a[1][:, :0].copy(), a[2][:, :0].copy(), 1, "short")
    rc, per_utt, host, own = _launch([a, short, empty, b], 1, pad_value=0x7fff)
    assert rc == 0
    assert per_utt[1].shape == (0, 64) and per_utt[2].shape == (0, 64)
    assert int(own.sum()) == 17 + 65
    assert per_utt[0].tobytes() == batch_results[a[0]].tobytes() and per_utt[3].tobytes() == batch_results[b[0]].tobytes()
    worst = {}
    _check(a[0], per_utt[0], models[a[0]], worst, "short")
    _check(b[0], per_utt[3], models[b[0]], worst, "short")


def test_host_form_is_the_batch_form(case_list, models, batch_results):
    """sea.irm_target (its own device buffers, padding columns uninitialised) on F = 1, F = 17 with L % 8 != 0 and F = 65: the model
    within IRM_TOL and the batch form's bits -- both run one kernel"""
    import speech_enhancement_amd as sea
    by = {c[0]: c for c in case_list}
    worst = {}
    for name in ("tones F=1 tail=0 w=1", "tones F=17 tail=5 w=2", "ramped tones F=65 tail=159 w=0"):
        _, p, n, kind, _ = by[name]
        assert name != "tones F=17 tail=5 w=2" or p.shape[1] % 8
        p0, n0 = p.copy(), n.copy()
        got = sea.irm_target(p, n, kind)
        assert np.array_equal(p, p0) and np.array_equal(n, n0)
        _check(name, got, models[name], worst, "host form")
        assert got.tobytes() == batch_results[name].tobytes(), f"{name}: host form and batch form differ"
    print(f"IRM target, host form: worst |device - model| {worst['host form']:.3g}   (IRM_TOL {C.IRM_TOL:.3g})")


def test_window_kinds_outside_0_to_2_are_refused(case_list):
    lib_mod, lib = _lib()
    by = {c[0]: c for c in case_list}
    a = by["tones F=1 tail=5 w=1"]
    for kind in (3, -1):
        rc, _, host, _ = _launch([a], kind)
        assert rc != 0 and b"window" in lib.sea_last_error()
        assert np.all(host == np.float32(SENT)), f"window {kind}: the output was written"
        out = np.full((1, 64), SENT, np.float32)
        p, n = np.ascontiguousarray(a[1]), np.ascontiguousarray(a[2])
        rc = lib.sea_irm_target(p.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(ctypes.c_void_p), p.shape[1], kind,
                                out.ctypes.data_as(ctypes.c_void_p))
        assert rc != 0 and np.all(out == np.float32(SENT)), f"window {kind}: host form"
