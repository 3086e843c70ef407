"""The wideband feature chain's time slices without a GPU: the built library exports the entry points, ``_lib.py`` declares them,
the shared object holds gfx950 code for the slice kernels, every argument check is reached before the device is touched, and
the engine wrappers refuse a state tensor that cannot hold the state."""
import ctypes
import os

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")

NEW_SYMBOLS = ("sea_wb_denoise_batch_slice_fd", "sea_wb_afe_features_batch_slice", "sea_wb_afe_slice_state_floats",
               "sea_wb_features_utterances")
SLICE_KERNELS = (b"ns_denoise_pipe_wb_fd_slice_kernel", b"afe_wb_ceps_slice_kernel", b"afe_wb_vad_slice_kernel")
P = ctypes.c_void_p(4096)  # a pointer no refused call may follow


def test_library_exports_the_entry_points_and_lib_declares_them():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
        assert name in header, f"{name} is not declared in include/sea_mi355x.h"
    res, args = _lib.PROTOTYPES["sea_wb_denoise_batch_slice_fd"]
    assert res is ctypes.c_int and len(args) == 18 and args[12] is ctypes.c_longlong and args[14:17] == [ctypes.c_int] * 3
    res, args = _lib.PROTOTYPES["sea_wb_afe_features_batch_slice"]
    assert res is ctypes.c_int and len(args) == 22 and args[10] is ctypes.c_longlong and args[18:21] == [ctypes.c_int] * 3
    assert len(_lib.PROTOTYPES["sea_wb_features_utterances"][1]) == 6
    for name in ("wb_afe_slice_state", "wb_afe_features_batch_slice", "wb_features_utterances"):
        assert callable(getattr(sea, name))


def test_library_contains_gfx950_code_for_the_slice_kernels():
    import speech_enhancement_amd as sea
    blob = open(sea.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for name in SLICE_KERNELS:
        assert name in blob, f"no kernel {name.decode()} in the library"


def test_state_holds_the_histories_and_the_vad():
    """no device needed: the sizes are constants.  Two frames and a sample of the float stream, two rows of 3 and of 9, the ring
    of 7 x 15, 12 weights, 15 buffered features, the counters; the denoiser's state is as it was."""
    import speech_enhancement_amd as sea
    lib = sea.load()
    assert lib.sea_wb_afe_slice_state_floats() >= 161 + 6 + 18 + 105 + 12 + 15 + 7
    assert lib.sea_wb_afe_slice_state_floats() > 0
    assert lib.sea_wb_slice_state_floats() == lib.sea_ns_slice_state_floats() + 117 + 3 + 800 + 8


def _fd(lib, flags=P, f32=P, state=P, first=P, onset=P, hp=P, code=P, frame_base=0):
    return lib.sea_wb_denoise_batch_slice_fd(P, P, f32, P, P, None, first, onset, flags, hp, code, P, 160, state, 1, frame_base, 0, None)


def _feat(lib, f32=P, flags=P, afe=P, cc=P, f15=P, nf=P, ccum=P, fcum=P, frame_base=0, total=1):
    return lib.sea_wb_afe_features_batch_slice(f32, flags, P, P, P, P, P, P, None, ccum, total, cc, None, fcum, f15, nf, None, afe,
                                               1, frame_base, 0, None)


@pytest.mark.parametrize("call,name,kw", [
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(flags=None)),
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(f32=None)),
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(first=None)),
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(hp=None)),
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(state=None)),
    (_fd, "sea_wb_denoise_batch_slice_fd", dict(frame_base=-1)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(afe=None)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(flags=None)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(frame_base=-1)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(f15=None)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(nf=None)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(cc=None)),
    (_feat, "sea_wb_afe_features_batch_slice", dict(total=-1)),
])
def test_refusals_are_reached_without_a_device(call, name, kw):
    """every pointer but the missing one is a dummy: a refusal that came after the first launch, or after the device context,
    would not return this message"""
    import speech_enhancement_amd as sea
    lib = sea.load()
    rc = call(lib, **kw)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and msg.startswith(name + ":"), f"{kw}: rc {rc}, message {msg!r}"


def test_host_pipeline_checks_its_arguments_without_a_device():
    import speech_enhancement_amd as sea
    lib = sea.load()
    assert lib.sea_wb_features_utterances(None, None, None, None, None, 0) == 0
    x = np.zeros(320, np.int16)
    f = np.zeros((8, 15), np.float32)
    ins = (ctypes.c_void_p * 1)(x.ctypes.data)
    feats = (ctypes.c_void_p * 1)(f.ctypes.data)
    nf = (ctypes.c_int * 1)(-5)
    rc = lib.sea_wb_features_utterances(ins, None, feats, nf, (ctypes.c_long * 1)(-1), 1)
    assert rc != 0 and "negative length" in lib.sea_last_error().decode() and "sea_wb_features_utterances" in lib.sea_last_error().decode()
    rc = lib.sea_wb_features_utterances(ins, None, None, nf, (ctypes.c_long * 1)(320), 1)
    assert rc != 0 and "sea_wb_features_utterances" in lib.sea_last_error().decode()
    rc = lib.sea_wb_features_utterances(ins, None, (ctypes.c_void_p * 1)(None), nf, (ctypes.c_long * 1)(320), 1)
    assert rc != 0 and "feats[0]" in lib.sea_last_error().decode()
    assert nf[0] == -5 and not f.any(), "a refused call wrote something"


def test_engine_wrappers_reject_a_wrong_state():
    import torch
    import speech_enhancement_amd as sea
    lib = sea.load()
    b = sea.PackedBatch.from_arrays([np.zeros(320, np.int16), np.zeros(160, np.int16)], device="cpu")
    n_afe, n_wb = lib.sea_wb_afe_slice_state_floats(), lib.sea_wb_slice_state_floats()
    for bad in (None, torch.zeros((2, n_afe - 1)), torch.zeros((1, n_afe)), torch.zeros((2, n_afe), dtype=torch.float64),
                torch.zeros((2, 2 * n_afe))[:, ::2]):
        with pytest.raises(ValueError, match="afe_state"):
            sea.wb_afe_features_batch_slice(b, {}, bad, 0, False)
    for bad in (None, torch.zeros((2, n_wb - 1)), torch.zeros((2, n_wb), dtype=torch.float16)):
        with pytest.raises(ValueError, match="state"):
            sea.wb_denoise_batch_slice(b, bad, 0, False, want_flags=True)
    assert tuple(sea.wb_afe_slice_state(3, device="cpu").shape) == (3, n_afe)
