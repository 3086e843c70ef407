"""CPU tests of the inputs of tests/nonfinite_cases.py (Inf, NaN, finite floats whose energy overflows):

  1. the restatement equals the reference on them -- stored digests of the reference build's outputs (NaNs canonical), and
     the live build where oracle/_ref exists -- through ns_stream_f32, compceps_frame and rfft.  The 16 k-native variant's
     streams are not here: its frame loop is PARITY UNPINNED (no reference build of it exists; tests/test_gpu_ns16k.py);
  2. the inputs can see the bug class they are for: a MUTANT of the restatement whose logarithms take a non-finite argument
     apart by its bit pattern (oracle/ns_oracle.c, -DORA_BITPATTERN_LOG) differs from the restatement on them and equals it on
     the finite, non-overflowing streams of test_ns_stream_float_amplitude_extremes;
  3. the comparison rule itself."""
import json
import os

import numpy as np
import pytest

from tests import nonfinite_cases as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mutant():
    from oracle import oracle as O
    return O.BitPatternLogMutant()


@pytest.fixture(scope="module")
def streams():
    return N.streams_8k()


def test_same_words_rule():
    nan_pos, nan_neg = np.array([0x7FC00000], np.uint32).view(np.float32), np.array([0xFFC00000], np.uint32).view(np.float32)
    payload = np.array([0x7F800001], np.uint32).view(np.float32)
    f = lambda *v: np.array(v, np.float32)
    assert N.same_words(nan_pos, nan_neg) and N.same_words(payload, nan_neg)          # a NaN at a NaN position: payload, sign free
    assert not N.same_words(f(1.0), nan_pos) and not N.same_words(nan_pos, f(1.0))
    assert not N.same_words(f(np.inf), nan_pos) and not N.same_words(nan_pos, f(np.inf))
    assert N.same_words(f(np.inf, -np.inf), f(np.inf, -np.inf)) and not N.same_words(f(np.inf), f(-np.inf))
    assert not N.same_words(f(0.0), f(-0.0)) and N.same_words(f(-0.0), f(-0.0))
    assert not N.same_words(f(1.0), np.nextafter(f(1.0), f(2.0)))
    assert N.differing_words(f(1, 2, 3, np.nan), f(1, 5, 3, 4)) == 2
    assert N.same_words(np.array([1, 2], np.int32), np.array([1, 2], np.uint8)) and not N.same_words(np.array([1]), np.array([2]))
    assert N.digest(nan_pos) == N.digest(nan_neg) != N.digest(f(np.inf))


def test_cases_are_what_they_say(streams):
    from tests.test_gpu_parity import _float_stream_case
    base, s = streams
    assert np.array_equal(N.float_stream_case(12, 120), _float_stream_case(12, 120)) and np.array_equal(base, _float_stream_case(12, 120))
    assert len(s) == 12 + 4 + 11 and base.shape == (120, 80) and np.isfinite(base).all()
    for name, x in s.items():
        assert x.shape == base.shape and x.dtype == np.float32
        with np.errstate(over="ignore", invalid="ignore"):
            en = np.float32(64) + (x * x).sum(axis=1, dtype=np.float32)
        assert not np.isfinite(en).all(), f"{name}: every frame energy is finite"      # each stream reaches Inf or NaN energy
    assert np.isfinite(s["a/2/1.9e+19"]).all() and np.isfinite(s["b/x3e+30"]).all()    # ... some from finite samples alone
    b16, s16 = N.streams_16k()
    assert b16.shape == (48, 160) and len(s16) == 12 + 11
    g = N.ns16k_streams_per_group()
    order = N.batch_order(sorted(s16), 0, group=g)
    assert g >= 2 and len(order) == g * len(s16)
    for k in range(0, len(order), g):                        # every workgroup: one poisoned stream, the rest clean
        assert order[k] is not None and all(o is None for o in order[k + 1:k + g])
    order = N.batch_order(sorted(s), 3)
    assert order.count(None) == 3 and [o for o in order if o] == sorted(s) and order[0] is not None and order[-1] is not None
    cc = N.compceps_frames()
    for t in range(0, 35, 16):
        rows = set(range(t, min(t + 16, 35)))
        assert rows & set(N.CC_POISONED) and rows - set(N.CC_POISONED)
    assert all(np.isfinite(cc[i]).all() for i in range(35) if i not in N.CC_POISONED)


def test_nonfinite_inputs_vs_reference(oracle):
    """restatement == reference on every 8 kHz stream, CompCeps frame and rfft frame: by the stored digests of the reference
    build's outputs, and word by word under same_words against the live build where it exists"""
    from oracle import oracle as O
    with open(os.path.join(GOLD, "reference_live_digests.json")) as f:
        gold = {k: v for k, v in json.load(f).items() if k.startswith("nonfinite/")}
    got = N.live_nonfinite_digests(oracle)
    assert set(got) == set(gold), "tests/golden/reference_live_digests.json has other nonfinite/ entries"
    bad = sorted(k for k in got if got[k] != gold[k])
    assert not bad, f"differ from the reference's outputs (an '/in' entry: the seeded input itself changed): {bad[:8]}"
    if not O.have_reference():
        return
    ref = O.Reference()
    base, s = N.streams_8k()
    for name, x in [("base", base)] + sorted(s.items()):
        (wo, wp), (go, gp) = ref.ns_stream_f32(x), oracle.ns_stream_f32(x)
        assert np.array_equal(gp, wp) and N.same_words(go, wo), f"{name}: {N.differing_words(go, wo)} of {wo.size} words"
        g4 = oracle.ns_stream_f32_fd(x)
        assert N.same_words(g4[0], wo) and np.array_equal(g4[1], wp), f"{name}: the entry with flags gives another stream"
        if hasattr(ref.lib, "ref_ns_stream_f32_fd"):   # a reference build made from an earlier oracle/ref_driver.c has no such entry
            w4 = ref.ns_stream_f32_fd(x)
            assert all(np.array_equal(a, b) for a, b in zip(g4[1:], w4[1:])), f"{name}: flags / counter"
    for i, v in enumerate(N.compceps_frames()):
        assert N.same_words(oracle.compceps_frame(v), ref.compceps_frame(v)), f"CompCeps frame {i}"
    a, b = N.rfft_frames()
    for i, v in enumerate(a):
        assert N.same_words(oracle.rfft(v), ref.rfft(v)), f"rfft (256, 8) frame {i}"
    for i, v in enumerate(b):
        assert N.same_words(oracle.rfft(v, 8), ref.rfft(v, 8)), f"rfft (512, 8) frame {i}"


def test_expectations_hold_what_the_cases_are_for(oracle, streams):
    """the preconditions the GPU tests rely on, on the restatement alone"""
    base, s = streams
    for name in (n for n in s if n.startswith("a/")):
        out, _ = oracle.ns_stream_f32(s[name])
        ctl, _ = oracle.ns_stream_f32(N.a_control(s[name], name))
        assert not N.same_words(out, ctl), f"{name}: the same output as with 1e18 in the sample's place"
    want = np.stack([oracle.compceps_frame(v) for v in N.compceps_frames()])
    assert np.isnan(want).any() and np.isinf(want).any()
    for i in N.CC_TABLE_ROWS:
        assert not np.isfinite(want[i]).all(), f"CompCeps frame {i} ({N.CC_POISONED[i]}): all finite"
    assert all(np.isfinite(want[i]).all() for i in range(len(want)) if i not in N.CC_POISONED)


def test_bitpattern_log_mutant_is_told_apart(oracle, mutant, streams):
    """A logarithm that reads exponent and mantissa from the bit pattern (88.72 for +Inf, 89.13 for NaN) instead of returning
    Inf / NaN: different from the restatement on every stream with the overflowing sample in frame 2 or 6 and on the four
    non-finite CompCeps rows, equal on the finite non-overflowing streams of test_ns_stream_float_amplitude_extremes."""
    base, s = streams
    for name in (n for n in s if n.startswith("a/2/") or n.startswith("a/6/")):
        (wo, wp), (mo, mp) = oracle.ns_stream_f32(s[name]), mutant.ns_stream_f32(s[name])
        assert np.array_equal(wp, mp)
        n = N.differing_words(mo, wo)
        print(f"{name}: {n} of {wo.size} words differ between the mutant and the restatement")
        assert n > 0, f"{name}: the mutant is not told apart"
    cc = N.compceps_frames()
    for i in N.CC_TABLE_ROWS:
        assert not N.same_words(mutant.compceps_frame(cc[i]), oracle.compceps_frame(cc[i])), f"CompCeps frame {i} ({N.CC_POISONED[i]})"
    for i in range(len(cc)):
        if i not in N.CC_POISONED:
            assert N.same_words(mutant.compceps_frame(cc[i]), oracle.compceps_frame(cc[i])), f"clean CompCeps frame {i}"
    # the streams of tests/test_gpu_parity.py::test_ns_stream_float_amplitude_extremes, value for value
    from tests.test_gpu_parity import _float_stream_case
    b11 = _float_stream_case(11)
    cases = [b11 * np.float32(sc) for sc in (1.0, 1e-3, 3e-6, 1e-7, 3e-9, 1e-12, 1e-19, 1e-21, 30.0, 1e3, 1e5, 1e9, 1e18)]
    mixed = _float_stream_case(12, 90)
    mixed[20:35] *= np.float32(1e-9)
    mixed[35:50] *= np.float32(1e7)
    mixed[50:52] = 0.0
    mixed[60:75] *= np.float32(1e-20)
    cases += [mixed, np.concatenate([b11 * np.float32(1e6), b11, b11 * np.float32(2e-8)]), base]
    for k, x in enumerate(cases):
        (wo, wp), (mo, mp) = oracle.ns_stream_f32(x), mutant.ns_stream_f32(x)
        assert np.array_equal(wp, mp) and np.array_equal(wo.view(np.uint32), mo.view(np.uint32)), f"finite case {k}"
