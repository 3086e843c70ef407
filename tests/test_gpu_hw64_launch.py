"""hw64_correlogram_kernel's frame stride past the workgroups dealt.  The launch gives every utterance of a batch the same
number of workgroups, sea_hw64_workgroups_per_utterance (n_utt), and workgroup g walks the frames g, g + G, ...: a batch only
reaches the loop's later trips -- LDS (the window stage, hOut's ACF normalised in place, hEv's ring, sumCorr, acf0, sPitch)
reused from frame to frame -- when it has enough utterances.  The seven inputs of tests/test_gpu_hw64.py sit among fillers,
the fixture's 160-sample input (d): one frame each, known from the reference.  Every output is compared bit for bit."""
import numpy as np
import pytest

from tests import test_gpu_hw64 as H

pytestmark = pytest.mark.gpu


def _per_utt(n):
    import speech_enhancement_amd as sea
    return sea.hw64_workgroups_per_utterance(n)


def _smallest_batch_with(per_utt):
    """the smallest utterance count for which the launch deals per_utt workgroups to every utterance"""
    n = 1
    while _per_utt(n) > per_utt:
        n *= 2
    lo, hi = n // 2, n  # _per_utt (lo) > per_utt >= _per_utt (hi); it does not rise with n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _per_utt(mid) > per_utt else (lo, mid)
    assert _per_utt(hi) == per_utt, f"no batch size gives {per_utt} workgroups per utterance"
    return hi


def _trips(frames, per_utt):
    """trips of the frame loop per (utterance, workgroup): ceil ((frames - g) / per_utt)"""
    frames = np.asarray(frames, np.int64)
    return np.maximum(frames[:, None] - np.arange(per_utt)[None, :] + per_utt - 1, 0) // per_utt


def _case(n):
    """n utterances: the seven inputs spread over the batch, the fixture's (d) everywhere else"""
    import torch
    seven = H.seven_inputs()[0]
    ids = np.full(n, 4, np.int64)
    where = 3 + np.arange(7) * ((n - 6) // 7)
    ids[where] = np.arange(7)
    case = H.make_case([seven[i] for i in ids])
    perm = np.random.default_rng(n).permutation(n).astype(np.int32)
    case["d_perm"] = torch.from_numpy(perm).to("cuda:0")
    return case, ids, where


def _check(case, out, ids, where, names, what):
    nrows, total = int(case["rows"].sum()), case["batch"].total
    for name in ("hout", "hev"):
        assert (out[name][total * H.NCH:] == H.SENT).all(), f"{what}: {name} guard"
    for name in ("acf_hc", "acf_ev", "cross_hc", "cross_ev", "pratio", "mark"):
        if out[name] is not None:
            assert (out[name][nrows:] == H.SENT).all() and not (out[name][:nrows] == H.SENT).any(), f"{what}: {name} rows"
    assert (out["pitch"][nrows:] == H.SENT_I).all()
    for u in where:  # the real utterances, every array
        got = H.utterance(case, out, u)
        for name in names:
            assert H.matches(got[name], name, ids[u]), f"{what}: utterance {u} (input {ids[u]}): {name}"
    # the fillers: all alike, so one comparison of the stacked rows against the fixture's single frame
    g = H.seven_inputs()[2]
    fill = np.setdiff1d(np.arange(len(ids)), where)
    r = case["offs"][fill]
    for name, key in (("cross_hc", "cross_hc"), ("cross_ev", "cross_ev"), ("pitch", "pitch"), ("pRatio", "pratio"), ("mark", "mark")):
        want = np.broadcast_to(g[f"{name}_d"][0], (len(fill),) + g[f"{name}_d"].shape[1:])
        assert H.M.same_bits(np.ascontiguousarray(out[key][r]), np.ascontiguousarray(want)), f"{what}: the fillers' {name}"
    for u in fill[[0, len(fill) // 2, -1]]:
        got = H.utterance(case, out, u)
        for name in names:
            assert H.matches(got[name], name, 4), f"{what}: filler {u}: {name}"


@pytest.mark.parametrize("mode,order", [("group", False), ("two", True)], ids=["group_plain", "two_calls_permuted"])
def test_three_workgroups_per_utterance(mode, order):
    """as many utterances as give three workgroups each (342 with 256 CUs): the 11-frame inputs take four trips of the frame
    loop in workgroups 0 and 1, three in workgroup 2; the 8-frame one three, three and two.  With the ACF outputs."""
    n = _smallest_batch_with(3)
    case, ids, where = _case(n)
    t = _trips(case["rows"], 3)
    assert t.max() == 4 and (t[where[0]] == [4, 4, 3]).all() and (t[where[6]] == [3, 3, 2]).all() and (t >= 3).sum() >= 11
    out = H.launch(case, mode, order, True)
    _check(case, out, ids, where, H.ARRAYS, f"3 workgroups per utterance, {mode}")


def test_one_workgroup_per_utterance():
    """as many utterances as give one workgroup each (1024 with 256 CUs): one workgroup walks all 11 frames.  Permuted, null
    ACF pointers (proven equivalent in tests/test_gpu_hw64.py)."""
    n = _smallest_batch_with(1)
    assert _per_utt(n + 1) == 1 and _per_utt(0) == 0
    case, ids, where = _case(n)
    assert _trips(case["rows"], 1).max() == 11
    out = H.launch(case, "group", True, False)
    assert out["acf_hc"] is None and out["acf_ev"] is None
    _check(case, out, ids, where, tuple(k for k in H.ARRAYS if not k.startswith("acf_")), "1 workgroup per utterance")
