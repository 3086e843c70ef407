"""GPU tests of the gammatone / resynthesis half against the independent float64 model (tests/gammatone_model.py).
Run on an MI355X with ``pytest -m gpu``.

Every other GPU test of this half asserts bit-identity with oracle/resynth_oracle.c, a restatement written from the same
reading of extractwav.cpp as the kernels.  Here the kernels are held to the model directly -- no oracle in that
comparison -- on the inputs and at the thresholds of tests/resynth_model_cases.py, which tests/test_resynth_model_cpu.py
measured on the CPU (restatement vs model) and proved able to see seven misreadings of the source.  On the same inputs
(lengths around the 16-sample tile and the 8-rows-in-flight boundaries, masks outside [0, 1), a channel sum that wraps
int16) the bit-identity with the restatement is asserted as well.  All cases of a mode travel in ONE batch, so the
LANE = CHANNEL tiles of neighbouring utterances sit side by side.
"""
import ctypes

import numpy as np
import pytest

from tests import gammatone_model as G
from tests import resynth_model_cases as C

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]       # (binary, frames_l_over_160)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _check_model_peak(name, model, silent):
    if silent:
        assert not np.any(model), name
    else:
        assert np.abs(model).max() >= C.MIN_PEAK, f"{name}: vacuous case, model peak {np.abs(model).max():.0f}"


def test_gammatone_filter_vs_model(oracle):
    """sea.gammaToneFilter, every channel, 16 000 samples of corpus / wideband / full-scale square / burst + silence"""
    import speech_enhancement_amd as sea
    _torch()
    cf, bw, me = oracle.resynth_channels()
    for name, x in C.stream_inputs().items():
        got = np.stack([sea.gammaToneFilter(x, c) for c in range(64)])
        model = G.gammatone_bank(x)
        _check_model_peak(name, model, False)
        fig = G.stream_figure(got, model)
        print(f"gammaToneFilter {name}: worst max|d| / channel peak {fig:.4g} (tolerance {C.STREAM_TOL:.3g})")
        assert fig <= C.STREAM_TOL, name
        want = np.stack([oracle.gammatone(x, cf[c], bw[c], me[c]) for c in range(64)])
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(-1))[0]
        assert bad.size == 0, f"{name}: channels {bad[:8]} differ from the restatement"


def test_subband_vs_model(oracle):
    """subband_batch (one batch: lengths 1, 15, 16, 17 next to long ones) and subbband() against the model's gammatone +
    float64 Meddis recursion + cast"""
    import speech_enhancement_amd as sea
    torch = _torch()
    cases, models = C.subband_cases(), C.subband_model()
    utts = [x for _, x, _ in cases]
    batch = sea.PackedBatch.from_arrays(utts)
    out = sea.subband_batch(batch)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for u, ((name, x, check_peak), model) in enumerate(zip(cases, models)):
        L = len(x)
        if check_peak:
            _check_model_peak(name, model, False)
        pitch = (L + 7) // 8 * 8
        off = int(batch.host_offsets[u]) * 64
        blk = np.ascontiguousarray(host[off: off + 64 * pitch].reshape(64, pitch)[:, :L])
        C.check_int16(blk, model, "subband", f"subband_batch {name}")
        one = sea.subbband(x)
        C.check_int16(one, model, "subband", f"subbband {name}")
        want = oracle.subband64(x)
        assert np.array_equal(blk, want) and np.array_equal(one, want), f"{name}: differs from the restatement"


def _wrap_exercised(name, model, binary):
    if name == C.WRAP_CASE and not binary:
        over = float(np.mean(np.abs(model) > 32767))
        print(f"{name}: model sum beyond int16 on {over * 100:.2f} % of the samples")
        assert over >= 0.01, "the (short) wrap must be exercised on the device"


@pytest.mark.parametrize("binary,alt", MODES)
def test_resynth_batch_vs_model(oracle, binary, alt):
    import speech_enhancement_amd as sea
    torch = _torch()
    fam = C.family(binary, alt)
    cases, models = C.resynth_cases(alt), C.resynth_model(alt, binary)
    batch = sea.PackedBatch.from_arrays([x for _, x, _, _ in cases])
    mb = sea.MaskBatch.from_arrays([m for _, _, m, _ in cases])
    out, _ = sea.resynth_batch(batch, mb, binary=binary, frames_l_over_160=alt)
    torch.cuda.synchronize()
    for ((name, x, mask, silent), model, got) in zip(cases, models, batch.split(out)):
        _check_model_peak(name, model, silent)
        _wrap_exercised(name, model, binary)
        C.check_int16(got, model, fam, f"resynth_batch {fam} {name}")
        want = oracle.resynth64(x, mask, binary=binary, frames_l_over_160=alt)
        assert np.array_equal(got, want), f"{fam} {name}: differs from the restatement"


@pytest.mark.parametrize("binary,alt", MODES)
def test_resynth_host_entry_vs_model(oracle, binary, alt):
    """sea.resynth (sea_resynth64, host pointers), one utterance per call"""
    import speech_enhancement_amd as sea
    _torch()
    fam = C.family(binary, alt)
    for (name, x, mask, silent), model in zip(C.resynth_cases(alt), C.resynth_model(alt, binary)):
        got = sea.resynth(x, mask, binary=binary, frames_l_over_160=alt)
        C.check_int16(got, model, fam, f"resynth {fam} {name}")
        assert np.array_equal(got, oracle.resynth64(x, mask, binary=binary, frames_l_over_160=alt)), f"{fam} {name}"


@pytest.mark.parametrize("binary,alt", MODES)
def test_resynth_utterances_vs_model(oracle, binary, alt):
    """sea_resynth_utterances (the host-buffer list entry the file driver uses) through ctypes, all cases in one call"""
    import speech_enhancement_amd as sea
    _torch()
    lib = sea.load()
    fam = C.family(binary, alt)
    cases, models = C.resynth_cases(alt), C.resynth_model(alt, binary)
    utts = [x for _, x, _, _ in cases]
    masks = [m for _, _, m, _ in cases]
    outs = [np.full_like(x, -7777) for x in utts]
    n = len(utts)
    pin = (ctypes.c_void_p * n)(*[x.ctypes.data for x in utts])
    pm = (ctypes.c_void_p * n)(*[m.ctypes.data for m in masks])
    po = (ctypes.c_void_p * n)(*[y.ctypes.data for y in outs])
    pl = (ctypes.c_long * n)(*[len(x) for x in utts])
    mode = int(binary) | (2 if alt else 0)
    assert lib.sea_resynth_utterances(pin, pl, pm, mode, po, n) == 0, lib.sea_last_error()
    for (name, x, mask, silent), model, got in zip(cases, models, outs):
        C.check_int16(got, model, fam, f"sea_resynth_utterances {fam} {name}")
        assert np.array_equal(got, oracle.resynth64(x, mask, binary=binary, frames_l_over_160=alt)), f"{fam} {name}"
