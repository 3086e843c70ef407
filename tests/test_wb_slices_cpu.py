"""The wideband mode's time slices without a GPU: the built library exports the entry points, ``_lib.py`` declares them, the
shared object holds gfx950 code for the slice kernels, and the per-utterance state is large enough for what it must carry."""
import ctypes
import os

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sea_mi355x.h")

NEW_SYMBOLS = ("sea_wb_denoise_batch_slice", "sea_wb_slice_state_floats", "sea_wb_denoise_utterances")
SLICE_KERNELS = (b"wb_qmf_slice_kernel", b"ns_denoise_pipe_wb_slice_kernel", b"wb_hb_slice_kernel", b"wb_slice_end_kernel")


def test_library_exports_the_slice_entry_points_and_lib_declares_them():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    raw = ctypes.CDLL(sea.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by {sea.LIB_PATH}"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in _lib.py"
    res, args = _lib.PROTOTYPES["sea_wb_denoise_batch_slice"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[11] is ctypes.c_longlong and args[13:16] == [ctypes.c_int] * 3  # total_padded_samples; n_utt, frame_base, resume
    assert len(_lib.PROTOTYPES["sea_wb_denoise_utterances"][1]) == 6
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in header, f"{name} is not declared in include/sea_mi355x.h"


def test_library_contains_gfx950_code_for_the_slice_kernels():
    import speech_enhancement_amd as sea
    blob = open(sea.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for name in SLICE_KERNELS:
        assert name in blob, f"no kernel {name.decode()} in the library"


def test_state_holds_the_frame_loop_blob_the_delay_line_and_both_histories():
    """no device needed: the size is a constant.  117 raw samples of QMF history, five frames of 80 of either QMF stream."""
    import speech_enhancement_amd as sea
    lib = sea.load()
    assert lib.sea_wb_slice_state_floats() >= lib.sea_ns_slice_state_floats() + 117 + 800
