"""STOI on the GPU: frames, kept, stoi_terms, stoi_sum and every d bit for bit against the plain-C
statement of the contract (tests/stoi_model_driver.c, which tests/test_stoi_cpu.py holds to an independent float64 model).
stoi_band_kernel takes 64 kept frames per workgroup in two MFMA tiles of 32 rows, so the issue's frame counts -- the edges of
32 and 64 rows and of the 30-frame segment -- are its edges too.  The C model runs once per input set and is shared."""
import ctypes

import numpy as np
import pytest

from tests import stoi_model as M

pytestmark = pytest.mark.gpu


def _sea():
    import speech_enhancement_amd as sea
    return sea


def _check(refs, ests, rate, what, want):
    """stoi_utterances with the terms against the C model's results `want`, bit for bit"""
    got = _sea().stoi_utterances(refs, ests, rate=rate, terms=True)
    differ = 0
    for u, w in enumerate(want):
        g = dict(frames=int(got["frames"][u]), kept=int(got["kept"][u]), terms=int(got["stoi_terms"][u]), stoi_sum=got["stoi_sum"][u],
                 d=got["d"][u])
        n = M.same_result(g, w)
        if n:
            differ += n
            print(f"{what}, utterance {u} ({len(refs[u])} samples): {n} values differ; frames {g['frames']} / {w['frames']}, kept "
                  f"{g['kept']} / {w['kept']}, terms {g['terms']} / {w['terms']}, stoi_sum {g['stoi_sum']!r} / {w['stoi_sum']!r}")
        if w["terms"]:
            assert got["stoi"][u] == w["stoi_sum"] / w["terms"] or n
        else:
            assert np.isnan(got["stoi"][u])
    print(f"{what}: {len(want)} utterances, {sum(w['terms'] for w in want)} terms, {differ} differing values")
    assert differ == 0, what
    return got


@pytest.mark.parametrize("rate", M.RATES)
def test_frame_counts_at_the_edges_of_the_tiles(rate):
    """each length alone (its tiles start the launch) and all of them in one list; no frame is removed"""
    refs, ests, want = M.cached("tile", rate, lambda: M.tile_cases(rate))
    assert [w["kept"] for w in want] == [F for F in M.TILE_F for _ in M.TILE_R]
    _check(refs, ests, rate, f"rate {rate}, the lengths in one list", want)
    for u, (r, e) in enumerate(zip(refs, ests)):
        _check([r], [e], rate, f"rate {rate}, {r.size} samples alone", want[u:u + 1])


@pytest.mark.parametrize("rate", M.RATES)
def test_short_lengths(rate):
    refs, ests, want = M.cached("short", rate, lambda: M.short_cases(rate))
    assert [w["frames"] for w in want] == [0, 0, 0, 1] and want[3]["kept"] == 1
    _check(refs, ests, rate, f"rate {rate}, the short lengths in one list", want)
    for u, (r, e) in enumerate(zip(refs, ests)):
        _check([r], [e], rate, f"rate {rate}, {r.size} samples alone", want[u:u + 1])
    empty = _sea().stoi_utterances([], [], rate=rate)
    assert empty["stoi"].size == 0 and _sea().stoi_last_chunks() == 0


@pytest.mark.parametrize("rate", M.RATES)
def test_placement_in_lists(rate):
    for which, (refs, ests) in enumerate(M.placement_lists(rate)):
        want = M.cached(f"placement {which}", rate, lambda: (refs, ests))[2]
        _check(refs, ests, rate, f"rate {rate}, a list of {len(refs)}", want)
        if len(refs) > 2:
            assert want[len(refs) // 2]["frames"] == 0 and any(0 < w["kept"] < 30 for w in want)


@pytest.mark.parametrize("rate", M.RATES)
def test_frame_removal(rate):
    cases = M.removal_cases(rate)
    refs, ests, want = M.cached("removal", rate, lambda: ([c[0] for c in cases.values()], [c[1] for c in cases.values()]))
    for u, name in enumerate(cases):
        got = _check(refs[u:u + 1], ests[u:u + 1], rate, f"rate {rate}, {name}", want[u:u + 1])
        if name == "silent reference":
            assert got["kept"][0] == 0 and got["stoi_terms"][0] == 0
        if name == "silent estimate":
            assert got["stoi_terms"][0] > 0 and np.all(got["d"][0].view(np.uint32) == 0)
        if name == "identical":
            assert abs(got["stoi"][0] - 1.0) <= 1e-6
    _check(refs, ests, rate, f"rate {rate}, the removal cases in one list", want)


def test_results_do_not_depend_on_the_cut(monkeypatch):
    sea = _sea()
    refs, ests, want = M.cached("chunk", 16000, lambda: M.chunk_list(16000))
    monkeypatch.delenv("SEA_SCORE_SCRATCH_MB", raising=False)
    whole = _check(refs, ests, 16000, "the list whole", want)
    assert sea.stoi_last_chunks() == 1
    for mb, chunks in ((1, 4), (0, len(refs))):
        monkeypatch.setenv("SEA_SCORE_SCRATCH_MB", str(mb))
        got = _check(refs, ests, 16000, f"SEA_SCORE_SCRATCH_MB={mb}", want)
        assert sea.stoi_last_chunks() == chunks
        for key in ("stoi_sum", "stoi_terms", "frames", "kept"):
            assert got[key].tobytes() == whole[key].tobytes(), key
    # the mixed list of 67 (one utterance empty) at 8 kHz, one chunk per utterance
    refs8, ests8 = M.placement_lists(8000)[2]
    _check(refs8, ests8, 8000, "rate 8000, a list of 67, one chunk per utterance", M.cached("placement 2", 8000, lambda: (refs8, ests8))[2])
    assert sea.stoi_last_chunks() == 67


def test_terms_for_some_utterances_only(monkeypatch):
    """d_out NULL for some utterances and given for others, in two chunks; [S][15] written and nothing past it"""
    sea = _sea()
    lib = sea.load()
    refs, ests, want = M.cached("chunk", 16000, lambda: M.chunk_list(16000))
    monkeypatch.setenv("SEA_SCORE_SCRATCH_MB", "2")
    n = len(refs)
    d = [np.full(w["terms"] + 2, -777.0, np.float32) if u % 3 != 1 else None for u, w in enumerate(want)]
    ptr = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in arrays])  # noqa: E731
    s, t, fk = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.sea_stoi_utterances(ptr(refs), ptr(ests), (ctypes.c_long * n)(*[r.size for r in refs]), n, 16000, vp(s), vp(t), vp(fk), ptr(d))
    assert rc == 0, lib.sea_last_error()
    assert sea.stoi_last_chunks() == 2
    for u, w in enumerate(want):
        assert s[u].tobytes() == w["stoi_sum"].tobytes() and t[u] == w["terms"] and fk[u].tolist() == [w["frames"], w["kept"]]
        if d[u] is not None:
            assert d[u][:-2].tobytes() == w["d"].tobytes() and np.all(d[u][-2:] == -777.0), u
    assert all(lib.sea_stoi_last_stage_ms(st) > 0 for st in range(6))
