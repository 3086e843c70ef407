"""The table of tests/stream_cases.py against include/sea_mi355x.h and the ctypes binding, without a GPU: every prototype whose
last parameter is `void *stream` has a row (so a new entry point cannot arrive without a stream test), no row is stale, every
row names a run of tests/test_gpu_streams.py and what judges it, and where a run's expectation comes from a fixture, the
decoy's expectation differs from the true one's at every index and in every compared array."""
import ctypes

import numpy as np
import pytest

from speech_enhancement_amd import _lib
from tests import stream_cases as S
from tests import test_gpu_streams as T

ENTRY_POINTS = 44


def test_the_table_is_the_headers_set_of_stream_taking_prototypes():
    protos = S.stream_prototypes()
    assert sorted(protos) == sorted(S.TABLE), (sorted(set(protos) - set(S.TABLE)), sorted(set(S.TABLE) - set(protos)))
    assert len(S.TABLE) == ENTRY_POINTS


def test_a_new_prototype_or_a_dropped_row_is_noticed():
    with open(S.HEADER) as f:
        text = f.read()
    more = S.stream_prototypes(text.replace("#ifdef __cplusplus\n}", "int sea_new_batch(const float *d_x, float *d_y, int n_utt,\n"
                                                                      "                  void *stream);\n#ifdef __cplusplus\n}", 1))
    assert sorted(set(more) - set(S.TABLE)) == ["sea_new_batch"]
    assert [p.const for p in more["sea_new_batch"]] == [True, False, False, False]
    fewer = {k: v for k, v in S.TABLE.items() if k != "sea_hw64_am_batch"}
    assert sorted(set(S.stream_prototypes()) - set(fewer)) == ["sea_hw64_am_batch"]


def test_comments_are_stripped_before_the_prototypes_are_read():
    text = "/* int sea_ghost_batch(const float *d_x, void *stream); */\nint sea_real_batch(float *d_x /* in place */, void *stream);\n" \
           "int sea_host_form(const float *x, long n);\n"
    protos = S.stream_prototypes(text)
    assert list(protos) == ["sea_real_batch"] and protos["sea_real_batch"][0] == S.Param("d_x", True, False)


@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_binding_and_row(name):
    params = S.PROTOTYPES[name]
    res, args = _lib.PROTOTYPES[name]
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p, "the binding does not end in the stream pointer"
    assert len(args) == len(params), f"the binding has {len(args)} arguments, the header {len(params)}"
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == p.pointer, f"{name}: {p.name}"
    row = S.TABLE[name]
    assert callable(T.RUNS.get(row.prepare)), f"{name}: no run {row.prepare!r} in tests/test_gpu_streams.py"
    assert row.expectation.split(":")[0] in ("oracle", "fixture", "model", "one launch"), row.expectation
    assert any(not p.const and p.pointer and p.name != "stream" for p in params), "a call without an output?"


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


FIXTURE_BORNE = sorted({row.prepare for row in S.TABLE.values() if row.expectation.startswith("fixture")})


def test_every_fixture_borne_run_states_its_expectation():
    assert FIXTURE_BORNE == sorted(T.EXPECTED), sorted(set(FIXTURE_BORNE) ^ set(T.EXPECTED))


@pytest.mark.parametrize("run", FIXTURE_BORNE)
def test_the_decoys_expectation_differs(run):
    """the decoy holds the same utterances at other indices: at every index, every array that the run compares differs"""
    true = T.EXPECTED[run]()
    decoy = T._pick(true, "decoy")
    assert len(true) >= 2 and T._pick(true, "true") == true
    for i, (a, b) in enumerate(zip(true, decoy)):
        assert a.keys() == b.keys()
        for k in a:
            assert not _same(a[k], b[k]), f"{run}: {k} of the decoy equals the true case's at index {i}"
