"""The plain CompCeps' time slices and the cepstrum host pipelines without a GPU: the built library exports the entry points,
``_lib.py`` declares them, the shared object holds gfx950 code for the slice kernels, every argument check is reached before the
device is touched, and the engine wrappers refuse a state tensor that cannot hold the state."""
import ctypes
import os

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")

NEW_SYMBOLS = ("sea_compceps_batch_slice", "sea_cc_slice_state_floats", "sea_wb_compceps_batch_slice",
               "sea_wb_cc_slice_state_floats", "sea_wb_denoise_ceps_utterances")
SLICE_KERNELS = (b"compceps_slice_kernel", b"compceps_wb_slice_kernel", b"compceps_carry_slice_kernel")
P = ctypes.c_void_p(4096)  # a pointer no refused call may follow


def test_library_exports_the_entry_points_and_lib_declares_them():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
    res, args = _lib.PROTOTYPES["sea_compceps_batch_slice"]
    assert res is ctypes.c_int and len(args) == 13 and args[5] is ctypes.c_longlong and args[9:12] == [ctypes.c_int] * 3
    res, args = _lib.PROTOTYPES["sea_wb_compceps_batch_slice"]
    assert res is ctypes.c_int and len(args) == 15 and args[7] is ctypes.c_longlong and args[11:14] == [ctypes.c_int] * 3
    assert len(_lib.PROTOTYPES["sea_cc_slice_state_floats"][1]) == 0 and len(_lib.PROTOTYPES["sea_wb_cc_slice_state_floats"][1]) == 0
    assert len(_lib.PROTOTYPES["sea_wb_denoise_ceps_utterances"][1]) == 6 and len(_lib.PROTOTYPES["sea_denoise_ceps_utterances"][1]) == 6
    for name in ("cc_slice_state", "wb_cc_slice_state", "compceps_batch_slice", "wb_compceps_batch_slice", "denoise_ceps_utterances",
                 "wb_denoise_ceps_utterances"):
        assert callable(getattr(sea, name))
    assert "run it once at the end" not in header


def test_library_contains_gfx950_code_for_the_slice_kernels():
    import speech_enhancement_amd as sea
    blob = open(sea.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for name in SLICE_KERNELS:
        assert name in blob, f"no kernel {name.decode()} in the library"


def test_state_sizes():
    """no device needed: the sizes are constants.  Two frames and a sample of the float stream; the wideband state adds two
    high-band rows of 3 and two code rows of 9.  The four existing states are as they were: the cepstrum's is a blob of its own."""
    import speech_enhancement_amd as sea
    lib = sea.load()
    assert lib.sea_cc_slice_state_floats() >= 161
    assert lib.sea_wb_cc_slice_state_floats() >= 161 + 6 + 18
    assert lib.sea_afe_slice_state_floats() >= 161 + 105 + 12 + 15 + 5
    assert lib.sea_ns_slice_state_floats() == 2 * 640 + 12 * 64 + 3 * 8 + 40
    assert lib.sea_wb_slice_state_floats() == lib.sea_ns_slice_state_floats() + 117 + 3 + 800 + 8
    assert lib.sea_wb_afe_slice_state_floats() >= lib.sea_afe_slice_state_floats() + 6 + 18


def _cc(lib, f32=P, offs=P, lens=P, first=P, cum=P, ceps=P, nc=P, state=P, frame_base=0, total=1):
    return lib.sea_compceps_batch_slice(f32, offs, lens, first, cum, total, ceps, nc, state, 1, frame_base, 0, None)


def _wbcc(lib, f32=P, offs=P, lens=P, first=P, hp=P, code=P, cum=P, ceps=P, nc=P, state=P, frame_base=0, total=1):
    return lib.sea_wb_compceps_batch_slice(f32, offs, lens, first, hp, code, cum, total, ceps, nc, state, 1, frame_base, 0, None)


_COMMON = [dict(state=None), dict(f32=None), dict(offs=None), dict(lens=None), dict(first=None), dict(cum=None), dict(ceps=None),
           dict(nc=None), dict(total=-1), dict(frame_base=-1)]


@pytest.mark.parametrize("call,name,kw", [(_cc, "sea_compceps_batch_slice", kw) for kw in _COMMON] +
                         [(_wbcc, "sea_wb_compceps_batch_slice", kw) for kw in _COMMON + [dict(hp=None), dict(code=None)]])
def test_refusals_are_reached_without_a_device(call, name, kw):
    """every pointer but the missing one is a dummy: a refusal that came after the first launch, or after the device context,
    would not return this message"""
    import speech_enhancement_amd as sea
    lib = sea.load()
    rc = call(lib, **kw)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and msg.startswith(name + ":"), f"{kw}: rc {rc}, message {msg!r}"


@pytest.mark.parametrize("fn,hop", [("sea_denoise_ceps_utterances", 80), ("sea_wb_denoise_ceps_utterances", 160)])
def test_host_pipelines_check_their_arguments_without_a_device(fn, hop):
    import speech_enhancement_amd as sea
    lib = sea.load()
    call = getattr(lib, fn)
    name = fn + ":"
    assert call(None, None, None, None, None, 0) == 0
    x = np.zeros(10 * hop, np.int16)
    o = np.full(10 * 80 * (hop // 80), 7, np.int16)
    c = np.zeros((4, 14), np.float32)
    ins, outs = (ctypes.c_void_p * 1)(x.ctypes.data), (ctypes.c_void_p * 1)(o.ctypes.data)
    ceps = (ctypes.c_void_p * 1)(c.ctypes.data)
    nc = (ctypes.c_int * 1)(-5)
    good = (ctypes.c_long * 1)(10 * hop)
    rc = call(ins, outs, ceps, nc, (ctypes.c_long * 1)(-1), 1)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and "negative length" in msg and msg.startswith(name), msg
    rc = call(ins, outs, (ctypes.c_void_p * 1)(None), nc, good, 1)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and "ceps[0]" in msg and msg.startswith(name), msg
    for args in ((None, outs, ceps, nc, good), (ins, outs, None, nc, good), (ins, outs, ceps, None, good), (ins, outs, ceps, nc, None)):
        rc = call(*args, 1)
        msg = lib.sea_last_error().decode()
        assert rc != 0 and msg.startswith(name), msg
    assert nc[0] == -5 and not c.any() and (o == 7).all(), "a refused call wrote something"


def test_engine_wrappers_reject_a_wrong_state():
    import torch
    import speech_enhancement_amd as sea
    lib = sea.load()
    b = sea.PackedBatch.from_arrays([np.zeros(320, np.int16), np.zeros(160, np.int16)], device="cpu")
    for fn, make, n in ((sea.compceps_batch_slice, sea.cc_slice_state, lib.sea_cc_slice_state_floats()),
                        (sea.wb_compceps_batch_slice, sea.wb_cc_slice_state, lib.sea_wb_cc_slice_state_floats())):
        for bad in (None, torch.zeros((2, n - 1)), torch.zeros((1, n)), torch.zeros((2, n), dtype=torch.float64),
                    torch.zeros((2, 2 * n))[:, ::2]):
            with pytest.raises(ValueError, match="cc_state"):
                fn(b, {}, bad, 0, False)
        assert tuple(make(3, "cpu").shape) == (3, n) and make(3, "cpu").dtype == torch.float32
