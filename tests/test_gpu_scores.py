"""The objective scores on the GPU, every output bit for bit against the model of
tests/score_model.py (which tests/test_scores_cpu.py holds to the plain-C statement of the contract): lengths at the edges of
the kernel's tiles, placement in lists, special inputs, chunking, frame_db on request, masks, and dnn_score_utterances against
its composition.  score_frames_kernel tiles as the issue assumed -- 63 frames per wave, 252 per workgroup -- so the lengths are
the issue's."""
import ctypes

import numpy as np
import pytest

from tests import score_model as M

pytestmark = pytest.mark.gpu
HOPS = (80, 160)


def _sea():
    import speech_enhancement_amd as sea
    return sea


def _check(refs, ests, hop, what, want=None):
    """score_utterances with frame_db against the model (computed here unless the caller has it), bit for bit; the derived
    figures are the host's own"""
    import speech_enhancement_amd.scores as S
    got = _sea().score_utterances(refs, ests, hop=hop, frames=True)
    want = M.scores(refs, ests, hop) if want is None else want
    differ = 0
    for u, w in enumerate(want):
        g = dict(sums=np.array([got["srr"][u], got["see"][u], got["sre"][u]], np.int64), seg_sum=got["seg_sum"][u],
                 seg_frames=int(got["seg_frames"][u]), frame_db=got["frame_db"][u])
        if not M.same_scores(g, w):
            differ += 1
            print(f"{what}, utterance {u} ({len(refs[u])} samples): sums {g['sums'].tolist()} / {w['sums'].tolist()}, seg_sum "
                  f"{g['seg_sum']!r} / {w['seg_sum']!r}, frames {g['seg_frames']} / {w['seg_frames']}, "
                  f"{int(np.sum(g['frame_db'].view(np.uint32) != w['frame_db'].view(np.uint32)))} of {w['frame_db'].size} d differ")
        s = [int(v) for v in w["sums"]]
        for key, fn in (("snr_db", S.snr_db), ("si_sdr_db", S.si_sdr_db)):
            assert np.float64(got[key][u]).tobytes() == np.float64(fn(*s)).tobytes() or (np.isnan(got[key][u]) and np.isnan(fn(*s)))
        if w["seg_frames"]:
            assert got["segsnr_db"][u] == w["seg_sum"] / w["seg_frames"]
        else:
            assert np.isnan(got["segsnr_db"][u])
    print(f"{what}: {len(want)} utterances, {sum(w['frame_db'].size for w in want)} frames, {differ} utterances differ")
    assert differ == 0, what
    return got


@pytest.mark.parametrize("hop", HOPS)
def test_lengths_at_the_edges_of_the_tiles(hop):
    """each length alone (its tiles start the launch) and all of them in one list"""
    refs, ests = M.length_cases(hop)
    want = M.scores(refs, ests, hop)
    _check(refs, ests, hop, f"hop {hop}, the lengths in one list", want)
    for u, (r, e) in enumerate(zip(refs, ests)):
        _check([r], [e], hop, f"hop {hop}, {r.size} samples alone", want[u:u + 1])


@pytest.mark.parametrize("hop", HOPS)
def test_placement_in_lists(hop):
    for refs, ests in M.placement_lists(hop):
        _check(refs, ests, hop, f"hop {hop}, a list of {len(refs)}")
    # nothing but utterances without a tile, and an empty list
    z = np.zeros(0, np.int16)
    got = _check([z, np.ones(hop - 1, np.int16), z], [z, np.full(hop - 1, -2, np.int16), z], hop, f"hop {hop}, no half-frame at all")
    assert got["srr"].tolist() == [0, hop - 1, 0] and got["sre"].tolist() == [0, -2 * (hop - 1), 0]
    empty = _sea().score_utterances([], [], hop=hop)
    assert empty["srr"].size == 0 and _sea().score_last_chunks() == 0


@pytest.mark.parametrize("hop", HOPS)
def test_special_inputs(hop):
    cases = M.special_cases(hop)
    for name, (ref, est) in cases.items():
        _check([ref], [est], hop, f"hop {hop}, {name}")
    _check([c[0] for c in cases.values()], [c[1] for c in cases.values()], hop, f"hop {hop}, the special inputs in one list")


def test_results_do_not_depend_on_the_cut(monkeypatch):
    sea = _sea()
    refs, ests = M.chunk_list()
    monkeypatch.delenv("SEA_SCORE_SCRATCH_MB", raising=False)
    want = M.scores(refs, ests, 160)
    whole = _check(refs, ests, 160, "the list whole", want)
    assert sea.score_last_chunks() == 1
    for mb, chunks in ((1, 4), (0, len(refs))):
        monkeypatch.setenv("SEA_SCORE_SCRATCH_MB", str(mb))
        got = _check(refs, ests, 160, f"SEA_SCORE_SCRATCH_MB={mb}", want)
        assert sea.score_last_chunks() == chunks
        for key in ("srr", "see", "sre", "seg_sum", "seg_frames"):
            assert got[key].tobytes() == whole[key].tobytes(), key
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got["frame_db"], whole["frame_db"]))
    # the mixed list of 67 (one utterance empty), one chunk per utterance
    refs, ests = M.placement_lists(80)[2]
    _check(refs, ests, 80, "hop 80, a list of 67, one chunk per utterance")
    assert sea.score_last_chunks() == 67
    est, ideal = M.mask_cases(0.5, 0.5)
    got = sea.mask_scores(est, ideal)
    assert np.array_equal(got["counts"], M.mask_counts(est, ideal, 0.5, 0.5)) and sea.score_last_chunks() == len(est)


def test_frame_db_for_some_utterances_only():
    sea = _sea()
    lib = sea.load()
    hop = 160
    refs, ests = M.placement_lists(hop)[2]
    refs, ests = refs[:9], ests[:9]
    want = M.scores(refs, ests, hop)
    n = len(refs)
    db = [np.full(w["frame_db"].size + 2, -777.0, np.float32) if u % 3 != 1 else None for u, w in enumerate(want)]
    ptr = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in arrays])  # noqa: E731
    sums, seg, used = np.zeros((n, 3), np.int64), np.zeros(n, np.float64), np.zeros(n, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.sea_score_utterances(ptr(refs), ptr(ests), (ctypes.c_long * n)(*[r.size for r in refs]), n, hop, vp(sums), vp(seg),
                                  vp(used), ptr(db))
    assert rc == 0, lib.sea_last_error()
    for u, w in enumerate(want):
        assert np.array_equal(sums[u], w["sums"]) and seg[u].tobytes() == w["seg_sum"].tobytes() and used[u] == w["seg_frames"]
        if db[u] is not None:  # [F] written, nothing past it
            assert db[u][:-2].tobytes() == w["frame_db"].tobytes() and np.all(db[u][-2:] == -777.0), u


@pytest.mark.parametrize("t_est,t_ideal", [(t, t) for t in M.MASK_THRESHOLDS] + [(0.5, M.MASK_THRESHOLDS[2])])
def test_mask_counts(t_est, t_ideal):
    import speech_enhancement_amd.scores as S
    sea = _sea()
    est, ideal = M.mask_cases(t_est, t_ideal)
    want = M.mask_counts(est, ideal, t_est, t_ideal)
    assert want.sum(axis=0).min() >= 0.10 * want.sum()
    got = sea.mask_scores(est, ideal, t_est, t_ideal)
    print(f"thresholds {t_est}, {t_ideal}: counts\n{got['counts']}\nmodel\n{want}")
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want)
    assert np.array_equal(got["pooled"]["counts"], want.sum(axis=0))
    h, f, hf = S.hit_fa(*want.sum(axis=0).tolist())
    assert (got["pooled"]["hit"], got["pooled"]["fa"], got["pooled"]["hit_fa"]) == (h, f, hf)
    assert np.isnan(got["hit"][0]) and got["hit"][5] == want[5, 0] / (want[5, 0] + want[5, 2])
    # each utterance alone, and the order of the list reversed
    for u in range(len(est)):
        assert np.array_equal(sea.mask_scores(est[u:u + 1], ideal[u:u + 1], t_est, t_ideal)["counts"], want[u:u + 1])
    assert np.array_equal(sea.mask_scores(est[::-1], ideal[::-1], t_est, t_ideal)["counts"], want[::-1])


def test_dnn_score_utterances_is_its_composition():
    sea = _sea()
    from speech_enhancement_amd import corpus
    rng = np.random.default_rng(0)
    net = sea.DnnMask(1, np.full(192, -10.0), np.full(192, 0.1), [rng.standard_normal((64, 192)) / 8], [np.zeros(64)], ["sigmoid"])
    clean = [corpus.synth_utterance(40 + i, L) for i, L in enumerate((1600, 3333, 480))]
    noisy = [np.clip(c.astype(np.int32) + (corpus.synth_utterance(50 + i, c.size) // 4), -32768, 32767).astype(np.int16)
             for i, c in enumerate(clean)]
    got = sea.dnn_score_utterances(net, noisy, clean)
    enhanced = sea.dnn_enhance_utterances(net, noisy)
    want = {"enhanced": sea.score_utterances(clean, enhanced), "noisy": sea.score_utterances(clean, noisy)}
    for which in ("enhanced", "noisy"):
        assert set(got[which]) == set(want[which])
        for key, v in want[which].items():
            assert got[which][key].tobytes() == v.tobytes(), (which, key)
        _check(clean, enhanced if which == "enhanced" else noisy, 160, f"dnn_score_utterances, {which}")
    for key in ("snr_db", "si_sdr_db", "segsnr_db"):
        assert np.array_equal(got["gain_db"][key], want["enhanced"][key] - want["noisy"][key], equal_nan=True)
    assert np.all(np.isfinite(got["noisy"]["snr_db"])) and got["noisy"]["seg_frames"].tolist() == [8, 19, 2]  # one silent frame
