"""The Hu-Wang C ABI's refusals and size functions on both banks, without a GPU: every batch call of the 25-band (sea_hw25_*)
and the 64-band (sea_hw64_*) chain is one host text on a bank (csrc/hw_bank_capi.hip, csrc/hw_bank.h), so one table of calls is
run against both.  Only refused calls, empty batches and the size functions are made: every pointer here is host memory, and a
call that passed its checks would launch kernels on it."""
import ctypes

import numpy as np
import pytest

BANKS = {
    25: dict(nch=25, hop=80, delays=101, scratch_words=76, final_words=150, small_chunk=5, boundary=335544),
    64: dict(nch=64, hop=160, delays=201, scratch_words=193, final_words=384, small_chunk=8, boundary=131072),
}
FRONT = "in:hout in:hev in:offsets in:lengths in:row_offsets out?:acf_hc out?:acf_ev out:cross_hc out:cross_ev out:pitch out:pratio out:mark"


def calls(bank):
    """name of the exported call -> (the stage its messages name, the arguments in order).  An argument is `role:name` with the
    roles in / out (required pointers), in? / out? (pointers that may be null) and any? (out_f32 and out_i16: outputs of which
    one must be given); `none` for a pointer the call does not look at; anything else is passed as it stands."""
    tail = ["in?:order", 1, None]
    c = {
        f"sea_hw{bank}_correlogram_batch": ("correlogram", FRONT.split() + ["none"] + tail),
        f"sea_hw{bank}_frontend_batch": ("frontend", ["in:in", "out:hout", "out:hev"] + FRONT.split()[2:] + ["none"] + tail),
        f"sea_hw{bank}_pitch_batch": ("pitch", ["in:acf"] + (["in:cross"] if bank == 25 else []) + "in:pratio_in in:mark_in in:lengths "
                                      "in:row_offsets out:pitch out:grp out:pratio out:status out?:stages out:scratch".split() + tail),
        f"sea_hw{bank}_am_batch": ("am", "in:gout in:pitch in:offsets in:lengths in:row_offsets out:amcrn out?:ratio out?:seng out?:ampatt "
                                   "out?:am out:status out:scratch".split() + [64] + tail),
        f"sea_hw{bank}_finalseg_batch": ("finalseg", "in:grp in:amcrn in:cross_ev in:pratio in:lengths in:row_offsets out:mask "
                                         "out?:grp_final out:status out?:stages out:scratch".split() + tail),
        f"sea_hw{bank}_ibm_batch": ("ibm", "in:in in:offsets in:lengths in:row_offsets out:mask out:pitch out:status out?:stages "
                                    "out:scratch".split() + [64, 1] + tail),
    }
    gout = "in:in out:hout out:hev out?:gout in:offsets in:lengths".split() + tail
    if bank == 25:
        c["sea_hw25_periphery_gout_batch"] = ("periphery", gout)
        c["sea_hw25_periphery_batch"] = ("periphery", gout[:3] + gout[4:])
        c["sea_hw25_resynth_batch"] = ("resynth", "in:gout in:mask in:offsets in:lengths in:row_offsets".split() + [ctypes.c_float(0.0)] +
                                       ["any?:out_f32", "any?:out_i16"] + tail)
        c["sea_hw25_enhance_batch"] = ("enhance", "in:in in:offsets in:lengths in:row_offsets any?:out_f32 any?:out_i16 out:mask out:pitch "
                                       "out:status out:scratch".split() + [64, 1] + tail)
    else:
        c["sea_hw64_periphery_batch"] = ("periphery", gout)
    return c


CASES = [(bank, name) for bank in BANKS for name in calls(bank)]


@pytest.fixture(scope="module")
def lib():
    from speech_enhancement_amd import _lib
    return _lib.load()


def _role(arg):
    return arg.split(":")[0] if isinstance(arg, str) else None


def _refused(lib, rc, bank, stage, word):
    msg = lib.sea_last_error().decode(errors="replace")
    assert rc != 0 and msg.startswith(f"hw{bank}_{stage}:") and word in msg, (rc, msg)


@pytest.mark.parametrize("bank,name", CASES)
def test_null_and_shared_buffers_are_refused_before_a_device_is_touched(lib, bank, name):
    stage, spec = calls(bank)[name]
    buf = [np.zeros(16, np.float32) for _ in spec]  # a buffer of its own for every pointer, the optional ones too
    full = [b.ctypes.data_as(ctypes.c_void_p) if _role(a) else a for a, b in zip(spec, buf)]
    full = [None if a == "none" else v for a, v in zip(spec, full)]
    call = getattr(lib, name)
    # an empty batch is no work, whatever the pointers
    empty = [None if _role(a) else v for a, v in zip(spec, full)]
    empty[-2] = 0
    assert call(*empty) == 0
    # every required pointer null, one at a time
    required = [i for i, a in enumerate(spec) if _role(a) in ("in", "out")]
    assert len(required) >= 5
    for i in required:
        args = list(full)
        args[i] = None
        _refused(lib, call(*args), bank, stage, "null")
    both = [i for i, a in enumerate(spec) if _role(a) == "any?"]
    if both:
        args = list(full)
        for i in both:
            args[i] = None
        _refused(lib, call(*args), bank, stage, "null")
    # every output as every input, and every pair of outputs
    ins = [i for i, a in enumerate(spec) if _role(a) in ("in", "in?")]
    outs = [i for i, a in enumerate(spec) if _role(a) in ("out", "out?", "any?")]
    pairs = [(o, i) for o in outs for i in ins] + [(o, p) for k, o in enumerate(outs) for p in outs[:k]]
    assert len(outs) >= 2 and len(pairs) == len(outs) * len(ins) + len(outs) * (len(outs) - 1) // 2
    for out, other in pairs:
        args = list(full)
        args[out] = full[other]
        _refused(lib, call(*args), bank, stage, "must")


@pytest.mark.parametrize("bank", BANKS)
def test_single_utterance_forms_refuse_before_a_device_is_touched(lib, bank):
    x = np.zeros(16, np.float32).ctypes.data_as(ctypes.c_void_p)
    word = np.full(1, 99, np.int32)
    w = word.ctypes.data_as(ctypes.c_void_p)
    hop = BANKS[bank]["hop"]
    frontend, pitch, ibm = (getattr(lib, f"sea_hw{bank}_{n}") for n in ("frontend", "pitch", "ibm"))
    _refused(lib, frontend(x, 0, *([None] * 9)), bank, "frontend", "L=0")
    _refused(lib, frontend(None, hop, *([None] * 9)), bank, "frontend", "null")
    _refused(lib, pitch(x, 0, None, None, None, w), bank, "pitch", "L=0")
    _refused(lib, pitch(None, hop, None, None, None, w), bank, "pitch", "null")
    _refused(lib, pitch(x, hop, None, None, None, None), bank, "pitch", "null")
    _refused(lib, ibm(x, -1, None, None, w), bank, "ibm", "L=-1")
    _refused(lib, ibm(None, hop, None, None, w), bank, "ibm", "null")
    _refused(lib, ibm(x, hop, None, None, None), bank, "ibm", "null")
    assert ibm(None, 0, None, None, w) == 0 and word[0] == 0, "L = 0 is no work"


@pytest.mark.parametrize("bank", BANKS)
def test_size_functions_at_the_chunk_boundary(lib, bank):
    """The AM FFT takes all channels at once while its two complex buffers of 2 x the padded length, 2 * nch * 16 bytes per
    padded sample, stay within 256 MiB, else `small_chunk` channels at a time: the last total on the one side and the first on
    the other, whatever the number of utterances.  Every layout below is written out from the header's description."""
    b = BANKS[bank]
    nch, boundary = b["nch"], b["boundary"]
    assert boundary * 2 * nch * 16 <= 256 << 20 < (boundary + 1) * 2 * nch * 16
    f = {n: getattr(lib, f"sea_hw{bank}_{n}") for n in ("frames", "pitch_scratch_bytes", "am_scratch_bytes", "finalseg_scratch_bytes",
                                                        "ibm_scratch_bytes")}
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    pitch = lambda rows, n: 4 * (n * 2 * 400 + rows * b["scratch_words"])  # noqa: E731
    final = lambda rows: 4 * rows * b["final_words"] + 64  # noqa: E731
    am = lambda total, n, chunk: up(4 * n) + 2 * up(total * nch * 4 + 64) + 2 * up(total * 2 * chunk * 8 + 64)  # noqa: E731
    for total, chunk in ((boundary, nch), (boundary + 1, b["small_chunk"])):
        rows = total // b["hop"]
        assert f["frames"](total) == rows
        for n in (1, 7):
            assert f["am_scratch_bytes"](total, n) == am(total, n, chunk)
            assert f["pitch_scratch_bytes"](rows, n) == pitch(rows, n)
            assert f["finalseg_scratch_bytes"](rows, n) == final(rows)
            # hout | hev | gout | acf_hc | six frame planes and amcrn | the three stages' scratch, for one row more than asked
            r1 = rows + 1
            ibm = (3 * up(total * nch * 4 + 64) + up(r1 * nch * b["delays"] * 4) + 7 * up(r1 * nch * 4) + up(pitch(r1, n)) +
                   up(am(total, n, chunk)) + up(final(r1)))
            assert f["ibm_scratch_bytes"](total, rows, n) == ibm
    assert f["frames"](0) == f["frames"](-5) == f["frames"](b["hop"] - 1) == 0 and f["frames"](b["hop"]) == 1
    assert f["pitch_scratch_bytes"](-1, -1) == 0 and f["finalseg_scratch_bytes"](-3, 1) == 64
    assert f["am_scratch_bytes"](-1, 0) == 2 * up(64) + 2 * up(64)
    if bank == 25:
        assert lib.sea_hw25_scratch_bytes(boundary, 3) == 0
    else:
        assert lib.sea_hw64_workgroups_per_utterance(0) == 0 and lib.sea_hw64_pitch_waves_per_utterance(-2) == 0
