"""The 8 kHz feature chain's time slices without a GPU: the built library exports the entry points, ``_lib.py`` declares them,
the shared object holds gfx950 code for the slice kernels, every argument check is reached before the device is touched, and
the engine wrappers refuse a state tensor that cannot hold the state."""
import ctypes
import os

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")

NEW_SYMBOLS = ("sea_ns_denoise_batch_slice_fd", "sea_afe_features_batch_slice", "sea_afe_slice_state_floats",
               "sea_features_utterances")
SLICE_KERNELS = (b"ns_denoise_pipe_fd_slice_kernel", b"afe_ceps_slice_kernel", b"afe_vad_slice_kernel")
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
    res, args = _lib.PROTOTYPES["sea_ns_denoise_batch_slice_fd"]
    assert res is ctypes.c_int and len(args) == 14 and args[10:13] == [ctypes.c_int] * 3
    res, args = _lib.PROTOTYPES["sea_afe_features_batch_slice"]
    assert res is ctypes.c_int and len(args) == 20 and args[8] is ctypes.c_longlong and args[16:19] == [ctypes.c_int] * 3
    assert len(_lib.PROTOTYPES["sea_afe_slice_state_floats"][1]) == 0
    assert len(_lib.PROTOTYPES["sea_features_utterances"][1]) == 6
    for name in ("ns_slice_state", "afe_slice_state", "ns_denoise_batch_slice", "afe_features_batch_slice", "features_utterances"):
        assert callable(getattr(sea, name))


def test_library_contains_gfx950_code_for_the_slice_kernels():
    import speech_enhancement_amd as sea
    blob = open(sea.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for name in SLICE_KERNELS:
        assert name in blob, f"no kernel {name.decode()} in the library"


def test_state_sizes():
    """no device needed: the sizes are constants.  Two frames and a sample of the float stream, the ring of 7 x 15, 12 weights,
    15 buffered features, five counters; the denoiser's states are as they were: the flags' slice form adds no word."""
    import speech_enhancement_amd as sea
    lib = sea.load()
    assert lib.sea_afe_slice_state_floats() >= 161 + 105 + 12 + 15 + 5
    assert lib.sea_ns_slice_state_floats() == 2 * 640 + 12 * 64 + 3 * 8 + 40
    assert lib.sea_wb_slice_state_floats() == lib.sea_ns_slice_state_floats() + 117 + 3 + 800 + 8


def _fd(lib, din=P, out=P, offs=P, lens=P, flags=P, f32=P, state=P, first=P, onset=P, frame_base=0):
    return lib.sea_ns_denoise_batch_slice_fd(din, out, f32, offs, lens, None, first, flags, onset, state, 1, frame_base, 0, None)


def _feat(lib, f32=P, flags=P, offs=P, lens=P, first=P, onset=P, afe=P, cc=P, f15=P, nf=P, ccum=P, fcum=P, frame_base=0, total=1):
    return lib.sea_afe_features_batch_slice(f32, flags, offs, lens, first, onset, None, ccum, total, cc, None, fcum, f15, nf, None,
                                            afe, 1, frame_base, 0, None)


@pytest.mark.parametrize("call,name,kw", [
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(flags=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(f32=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(first=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(onset=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(state=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(din=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(out=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(offs=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(lens=None)),
    (_fd, "sea_ns_denoise_batch_slice_fd", dict(frame_base=-1)),
    (_feat, "sea_afe_features_batch_slice", dict(afe=None)),
    (_feat, "sea_afe_features_batch_slice", dict(f32=None)),
    (_feat, "sea_afe_features_batch_slice", dict(flags=None)),
    (_feat, "sea_afe_features_batch_slice", dict(offs=None)),
    (_feat, "sea_afe_features_batch_slice", dict(lens=None)),
    (_feat, "sea_afe_features_batch_slice", dict(first=None)),
    (_feat, "sea_afe_features_batch_slice", dict(onset=None)),
    (_feat, "sea_afe_features_batch_slice", dict(ccum=None)),
    (_feat, "sea_afe_features_batch_slice", dict(fcum=None)),
    (_feat, "sea_afe_features_batch_slice", dict(cc=None)),
    (_feat, "sea_afe_features_batch_slice", dict(f15=None)),
    (_feat, "sea_afe_features_batch_slice", dict(nf=None)),
    (_feat, "sea_afe_features_batch_slice", dict(total=-1)),
    (_feat, "sea_afe_features_batch_slice", dict(frame_base=-1)),
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
    name = "sea_features_utterances:"
    assert lib.sea_features_utterances(None, None, None, None, None, 0) == 0
    x = np.zeros(160, np.int16)
    f = np.zeros((8, 15), np.float32)
    ins = (ctypes.c_void_p * 1)(x.ctypes.data)
    feats = (ctypes.c_void_p * 1)(f.ctypes.data)
    nf = (ctypes.c_int * 1)(-5)
    good = (ctypes.c_long * 1)(160)
    rc = lib.sea_features_utterances(ins, None, feats, nf, (ctypes.c_long * 1)(-1), 1)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and "negative length" in msg and msg.startswith(name), msg
    for args in ((None, None, feats, nf, good), (ins, None, None, nf, good), (ins, None, feats, None, good),
                 (ins, None, feats, nf, None)):
        rc = lib.sea_features_utterances(*args, 1)
        msg = lib.sea_last_error().decode()
        assert rc != 0 and msg.startswith(name), msg
    rc = lib.sea_features_utterances(ins, None, (ctypes.c_void_p * 1)(None), nf, good, 1)
    msg = lib.sea_last_error().decode()
    assert rc != 0 and "feats[0]" in msg and msg.startswith(name), msg
    assert nf[0] == -5 and not f.any(), "a refused call wrote something"


def test_engine_wrappers_reject_a_wrong_state():
    import torch
    import speech_enhancement_amd as sea
    lib = sea.load()
    b = sea.PackedBatch.from_arrays([np.zeros(160, np.int16), np.zeros(80, np.int16)], device="cpu")
    n_afe, n_ns = lib.sea_afe_slice_state_floats(), lib.sea_ns_slice_state_floats()
    for bad in (None, torch.zeros((2, n_afe - 1)), torch.zeros((1, n_afe)), torch.zeros((2, n_afe), dtype=torch.float64),
                torch.zeros((2, 2 * n_afe))[:, ::2]):
        with pytest.raises(ValueError, match="afe_state"):
            sea.afe_features_batch_slice(b, {}, bad, 0, False)
    for want_flags in (False, True):
        for bad in (None, torch.zeros((2, n_ns - 1)), torch.zeros((1, n_ns)), torch.zeros((2, n_ns), dtype=torch.float16),
                    torch.zeros((2, 2 * n_ns))[:, ::2]):
            with pytest.raises(ValueError, match="state"):
                sea.ns_denoise_batch_slice(b, bad, 0, False, want_flags=want_flags)
    assert tuple(sea.afe_slice_state(3, "cpu").shape) == (3, n_afe) and sea.afe_slice_state(3, "cpu").dtype == torch.float32
    assert tuple(sea.ns_slice_state(3, "cpu").shape) == (3, n_ns)
