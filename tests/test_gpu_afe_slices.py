"""GPU tests of the 8 kHz FEATURE CHAIN in TIME SLICES (sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice,
sea_features_utterances): an utterance cut along the time axis, one launch group per slice, the feature side's own state carried
per utterance -- three frames of the float stream, PostProc's weights, the VAD's feature buffer, ring of seven and counters --
and the speech measures and the gate's onset carried in the frame loop's blob.

The criterion is exact: concatenated over an utterance's slices, feats, feat_cc, feat_pp, the flag bytes, the int16 audio and the
float stream are the BITS of the one launch (afe_features_batch, which these tests do not touch and which is pinned to the oracle
and to the reference's recorded outputs elsewhere), floats compared as uint32, and the counts sum to its counts.  So that both
sides cannot be wrong together, test 1 also holds the sliced result against the reference's recorded outputs
(tests/golden/afe_golden.npz) with tests/test_gpu_golden.py::test_golden_afe_feature_chain's limits: 1e-3 on features, zero
tolerance on counts, VAD flags and flag bytes.  Outputs start as sentinels and states as NaN.  Run on an MI355X with
``pytest -m gpu``."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT_I16 = 12321          # what every output holds before a launch
SENT_F32 = 54321.5
SENT_INT = -77
SENT_FLAG = 0xA5
# every frame of the zero leads (5, 8) and of the four-frame latency, the first cepstral frames (6 / 11 / 14), the first emissions
# (12 / 17 / 20), inside the ring of 7 and the tile of 8, then the ends of the utterances
BOUNDS = tuple(range(23)) + (40, 41, 97, 98, 150, 400)
FIXTURE = (("kat_head", 400, 0, 0), ("plain_1s", 200, 0, 0), ("leading_zeros", 100, 0, 5), ("gap", 98, 0, 8), ("loud", 60, 0, 0),
           ("ragged", 50, 37, 0))  # name, frames of 80, ragged tail, onset: longest first
EDGE_BOUNDS = (0, 7, 9, 10, 11, 35, 36, 99, 100, 101, 140, 230, 300, 600, 1030)
DEV = "cuda:0"


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _is_sent(a):
    return (_u32(a) == np.float32(SENT_F32).view(np.uint32)).all()


def _sorted(utts):
    """longest first (stable), so that the utterances of a later slice are a prefix of the list"""
    ids = sorted(range(len(utts)), key=lambda u: -(len(utts[u]) // 80))
    return ids, [utts[u] for u in ids]


def _flag_bytes(host_flags, offset, nfr):
    return host_flags[int(offset) // 8 + 10 * np.arange(nfr)]


def _one_launch(utts):
    """afe_features_batch on the list -> per utterance dict of numpy arrays; bytes and samples of frames without an output are
    zero, audio and float stream hold the whole frames only"""
    import speech_enhancement_amd as sea
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device=DEV)
    r = sea.afe_features_batch(b, want_intermediates=True)
    torch.cuda.synchronize()
    out, f32 = b.split(r["out"], full_frames_only=True), b.split(r["den_f32"], full_frames_only=True)
    flags = r["flags"].cpu().numpy()
    first, onset, n_ceps = (r[k].cpu().numpy() for k in ("first_out", "onset", "n_ceps"))
    cc, pp, cum = r["feat_cc"].cpu().numpy(), r["feat_pp"].cpu().numpy(), r["ceps_cum"]
    res = []
    for u, x in enumerate(utts):
        nc = int(n_ceps[u])
        res.append(dict(feats=r["feats"][u], n_ceps=nc, feat_cc=cc[cum[u]:cum[u] + nc], feat_pp=pp[cum[u]:cum[u] + nc],
                        flags=_flag_bytes(flags, b.host_offsets[u], len(x) // 80), out=out[u], f32=f32[u].reshape(-1, 80),
                        first_out=int(first[u]), onset=int(onset[u])))
    return res


@functools.lru_cache(maxsize=None)
def _fixture_one_launch():
    """the six fixtures, longest first, through the one launch: computed once, nothing modifies it"""
    with np.load(os.path.join(GOLD, "ns_golden.npz")) as z:
        utts = [z[f"{name}/in"] for name, *_ in FIXTURE]
    want = _one_launch(utts)
    for (name, nfr, tail, onset), x, w in zip(FIXTURE, utts, want):
        assert (len(x) // 80, len(x) % 80, w["onset"]) == (nfr, tail, onset), name
    assert _sorted(utts)[0] == list(range(len(utts)))
    return utts, want


def _cuts(utts, bounds, final=True):
    """[(frame_base, the active prefix's parts, final bytes or None)]: the list (longest first) cut at `bounds` (frames of 80);
    an utterance's last slice carries its ragged tail and, with `final`, its flush"""
    nfr = [len(x) // 80 for x in utts]
    assert nfr == sorted(nfr, reverse=True) and bounds[0] == 0 and bounds[-1] >= nfr[0]
    slices = []
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        act = [u for u in range(len(utts)) if nfr[u] > b0]
        assert act == list(range(len(act)))
        if not act:
            break
        parts = [utts[u][80 * b0:80 * b1] if b1 < nfr[u] else utts[u][80 * b0:] for u in act]
        slices.append((b0, parts, [b1 >= nfr[u] for u in act] if final else None))
    return slices


def _in_slices(n_utt, slices, features=True, states=None):
    """One launch group per slice into sentinel-filled buffers: sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice
    (features) or the plain sea_ns_denoise_batch_slice.  Both states start as NaN: resume = 0 must not read them.  Returns per
    utterance the concatenated pieces and the summed counts; `states`, a list, receives the feature chain's state after
    the last slice, one row per utterance."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    state = torch.full((n_utt, int(lib.sea_ns_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    afe = torch.full((n_utt, int(lib.sea_afe_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    first = torch.full((n_utt,), SENT_INT, dtype=torch.int32, device=DEV)
    onset = torch.full((n_utt,), SENT_INT, dtype=torch.int32, device=DEV)
    keys = ("out", "f32", "flags", "feat_cc", "feat_pp", "feats")
    got = [{k: [] for k in keys} for _ in range(n_utt)]
    n_feat, n_ceps = np.zeros(n_utt, np.int64), np.zeros(n_utt, np.int64)
    for k, (b0, parts, final) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        n = b.n_utt
        out = torch.full_like(b.data, SENT_I16)
        f32 = torch.full((b.data.numel(),), SENT_F32, dtype=torch.float32, device=DEV)
        flags = torch.full((max(b.total // 8, 1),), SENT_FLAG, dtype=torch.uint8, device=DEV)
        fr = np.array([len(x) // 80 for x in parts], np.int64)
        if not features:
            rc = lib.sea_ns_denoise_batch_slice(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order), _p(first),
                                                _p(state), n, b0, 1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
        else:
            rc = lib.sea_ns_denoise_batch_slice_fd(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                                   _p(first), _p(flags), _p(onset), _p(state), n, b0, 1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
            ccum = np.concatenate(([0], np.cumsum(fr))).astype(np.int64)
            fcum = np.concatenate(([0], np.cumsum(fr + 6))).astype(np.int64)
            tc, tf = int(ccum[-1]), int(fcum[-1])
            cc = torch.full((max(tc, 1), 14), SENT_F32, dtype=torch.float32, device=DEV)
            pp = torch.full((max(tc, 1), 14), SENT_F32, dtype=torch.float32, device=DEV)
            f15 = torch.full((max(tf, 1), 15), SENT_F32, dtype=torch.float32, device=DEV)
            nf = torch.full((n,), SENT_INT, dtype=torch.int32, device=DEV)
            nc = torch.full((n,), SENT_INT, dtype=torch.int32, device=DEV)
            d_ccum, d_fcum = torch.from_numpy(ccum).to(DEV), torch.from_numpy(fcum).to(DEV)
            d_final = torch.from_numpy(np.asarray(final, bool).astype(np.uint8)).to(DEV) if final is not None else None
            rc = lib.sea_afe_features_batch_slice(_p(f32), _p(flags), _p(b.offsets), _p(b.lengths), _p(first), _p(onset), _p(d_final),
                                                  _p(d_ccum), tc, _p(cc), _p(pp), _p(d_fcum), _p(f15), _p(nf), _p(nc), _p(afe), n, b0,
                                                  1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
        torch.cuda.synchronize()
        po, pf = b.split(out, full_frames_only=True), b.split(f32, full_frames_only=True)
        hflags = flags.cpu().numpy()
        for u in range(n):
            got[u]["out"].append(po[u])
            got[u]["f32"].append(pf[u].reshape(-1, 80))
            got[u]["flags"].append(_flag_bytes(hflags, b.host_offsets[u], fr[u]))
        if features:
            hcc, hpp, h15, hnf, hnc = (t.cpu().numpy() for t in (cc, pp, f15, nf, nc))
            for u in range(n):
                a, e = int(hnc[u]), int(hnf[u])
                assert 0 <= a <= fr[u] and 0 <= e <= fr[u] + 6, f"slice {k}, utterance {u}: counts {a} / {e} of {fr[u]} frames"
                got[u]["feat_cc"].append(hcc[ccum[u]:ccum[u] + a])
                got[u]["feat_pp"].append(hpp[ccum[u]:ccum[u] + a])
                got[u]["feats"].append(h15[fcum[u]:fcum[u] + e])
                assert not (_u32(h15[fcum[u]:fcum[u] + e]) == np.float32(SENT_F32).view(np.uint32)).any(), \
                    f"slice {k}, utterance {u}: an emitted row was not written"
                assert _is_sent(hcc[ccum[u] + a:ccum[u + 1]]) and _is_sent(hpp[ccum[u] + a:ccum[u + 1]]) \
                    and _is_sent(h15[fcum[u] + e:fcum[u + 1]]), f"slice {k}, utterance {u}: rows behind the slice's counts were written"
                n_feat[u] += e
                n_ceps[u] += a
    if states is not None:
        states.append(afe.cpu().numpy())
    first, onset = first.cpu().numpy(), onset.cpu().numpy()
    res = []
    for u, g in enumerate(got):
        r = dict(first_out=int(first[u]), onset=int(onset[u]), n_feat=int(n_feat[u]), n_ceps=int(n_ceps[u]))
        for key in keys:
            if g[key]:
                r[key] = np.concatenate(g[key])
        res.append(r)
    return res


def _assert_features_equal(got, want, what):
    """got: an entry of _in_slices; want: an entry of _one_launch"""
    assert (got["first_out"], got["onset"]) == (want["first_out"], want["onset"]), \
        f"{what}: first_out / onset {got['first_out']} / {got['onset']}, one launch {want['first_out']} / {want['onset']}"
    assert got["n_ceps"] == want["n_ceps"] and got["n_feat"] == len(want["feats"]), \
        f"{what}: {got['n_ceps']} cepstral / {got['n_feat']} emitted frames, one launch {want['n_ceps']} / {len(want['feats'])}"
    for k in ("feat_cc", "feat_pp", "feats"):
        assert got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} != {want[k].shape}"
        bad = (_u32(got[k]) != _u32(want[k])).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} rows of {k} differ in bits from the one launch, first at {np.flatnonzero(bad)[:4]}"
    quiet = want["first_out"] if want["first_out"] >= 0 else len(want["flags"])
    assert (got["flags"][:quiet] == SENT_FLAG).all(), f"{what}: flag bytes of frames without an output were written"
    assert np.array_equal(got["flags"][quiet:], want["flags"][quiet:]), f"{what}: flag bytes differ from the one launch"
    assert np.array_equal(got["out"], want["out"]), f"{what}: int16 audio differs from the one launch"
    assert _is_sent(got["f32"][:quiet]), f"{what}: the float stream of frames without an output was written"
    assert np.array_equal(_u32(got["f32"][quiet:]), _u32(want["f32"][quiet:])), f"{what}: float stream differs in bits from the one launch"


def test_fixtures_in_slices():
    """The six fixtures, longest first, cut at BOUNDS, d_final on each utterance's last slice.  Everything equals the one launch
    bit for bit, what the _fd slice shares with sea_ns_denoise_batch_slice equals that call's on the same cuts, and the sliced
    result is within test_golden_afe_feature_chain's limits of the reference's recorded outputs."""
    utts, want = _fixture_one_launch()
    slices = _cuts(utts, BOUNDS)
    got = _in_slices(len(utts), slices)
    plain = _in_slices(len(utts), slices, features=False)
    worst = 0.0
    with np.load(os.path.join(GOLD, "afe_golden.npz")) as g:
        for j, (name, nfr, tail, onset) in enumerate(FIXTURE):
            _assert_features_equal(got[j], want[j], name)
            assert got[j]["onset"] == onset and got[j]["first_out"] == plain[j]["first_out"] == onset + 4, name
            assert np.array_equal(got[j]["out"], plain[j]["out"]), f"{name}: int16 audio != sea_ns_denoise_batch_slice's"
            assert np.array_equal(_u32(got[j]["f32"]), _u32(plain[j]["f32"])), f"{name}: float stream != sea_ns_denoise_batch_slice's"
            f0 = got[j]["first_out"]
            wf = g[f"{name}/flags"]
            assert wf.shape[0] == nfr
            assert np.array_equal(got[j]["flags"][f0:], wf[f0:nfr, :4] @ np.array([1, 2, 4, 8])), f"{name}: flag bytes != the reference's"
            wcc, wpp, w15 = g[f"{name}/feat_cc"], g[f"{name}/feat_pp"], g[f"{name}/vad_out"]
            assert got[j]["n_ceps"] == len(wcc) and got[j]["feats"].shape == w15.shape, f"{name}: counts != the reference's"
            assert np.array_equal(got[j]["feats"][:, 14], w15[:, 14]), f"{name}: VAD decisions differ from the reference's"
            for what, gg, ww in (("feat_cc", got[j]["feat_cc"], wcc), ("feat_pp", got[j]["feat_pp"], wpp),
                                 ("feats", got[j]["feats"][:, :14], w15[:, :14])):
                d = float(np.abs(gg - ww).max()) if len(ww) else 0.0
                worst = max(worst, d)
                assert d <= 1e-3, f"{name} {what}: off the reference by {d}"
    print(f"\n{len(slices)} slices: the one launch's bits; worst |delta| to the reference's recorded outputs {worst}")


def _single_frames(x):
    """One utterance alone, one launch group per frame (and one for a ragged tail), pointers advanced frame by frame into
    buffers of the whole utterance; per-slice feature blocks of 1 cepstral and 7 emitted rows.  One read-back at the end."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    nfr, tail = len(x) // 80, len(x) % 80
    ns = nfr + (1 if tail else 0)
    xin = np.zeros(80 * (nfr + 1), np.int16)
    xin[:len(x)] = x
    d_in = torch.from_numpy(xin).to(DEV)
    out = torch.full((80 * (nfr + 1),), SENT_I16, dtype=torch.int16, device=DEV)
    f32 = torch.full((80 * (nfr + 1),), SENT_F32, dtype=torch.float32, device=DEV)
    flags = torch.full((10 * (nfr + 1),), SENT_FLAG, dtype=torch.uint8, device=DEV)
    first = torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV)
    onset = torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV)
    meta = torch.tensor([0, 80, 0, 1, 0, 7], dtype=torch.int64, device=DEV)        # offsets | lengths | ceps_cum | feat_cum
    meta_t = torch.tensor([0, tail, 0, 0, 0, 6], dtype=torch.int64, device=DEV)    # the tail: no whole frame
    one = torch.ones(1, dtype=torch.uint8, device=DEV)
    state = torch.full((1, int(lib.sea_ns_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    afe = torch.full((1, int(lib.sea_afe_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    cc = torch.full((ns, 14), SENT_F32, dtype=torch.float32, device=DEV)
    pp = torch.full((ns, 14), SENT_F32, dtype=torch.float32, device=DEV)
    f15 = torch.full((ns, 7, 15), SENT_F32, dtype=torch.float32, device=DEV)
    nf = torch.full((ns,), SENT_INT, dtype=torch.int32, device=DEV)
    nc = torch.full((ns,), SENT_INT, dtype=torch.int32, device=DEV)
    for f in range(ns):
        is_tail = f == nfr
        m = meta_t if is_tail else meta
        rc = lib.sea_ns_denoise_batch_slice_fd(_p(d_in, 160 * f), _p(out, 160 * f), _p(f32, 320 * f), _p(m), _p(m, 8), None, _p(first),
                                               _p(flags, 10 * f), _p(onset), _p(state), 1, f, 1 if f > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
        rc = lib.sea_afe_features_batch_slice(_p(f32, 320 * f), _p(flags, 10 * f), _p(m), _p(m, 8), _p(first), _p(onset),
                                              _p(one) if f == ns - 1 else None, _p(m, 16), 0 if is_tail else 1, _p(cc, 56 * f),
                                              _p(pp, 56 * f), _p(m, 32), _p(f15, 420 * f), _p(nf, 4 * f), _p(nc, 4 * f), _p(afe), 1, f,
                                              1 if f > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    hcc, hpp, h15, hnf, hnc = (t.cpu().numpy() for t in (cc, pp, f15, nf, nc))
    assert ((hnc == 0) | (hnc == 1)).all() and (hnf[:-1] <= 1).all() and 0 <= hnf[-1] <= 7, "a slice's counts are out of range"
    for f in range(ns):
        assert _is_sent(hcc[f][None][hnc[f]:]) and _is_sent(h15[f][hnf[f]:]), f"slice {f}: rows behind the counts were written"
    return dict(first_out=int(first.cpu()[0]), onset=int(onset.cpu()[0]), n_feat=int(hnf.sum()), n_ceps=int(hnc.sum()),
                feat_cc=hcc[hnc == 1], feat_pp=hpp[hnc == 1], feats=np.concatenate([h15[f][:hnf[f]] for f in range(ns)]),
                flags=flags.cpu().numpy()[10 * np.arange(nfr)], out=out.cpu().numpy()[:80 * nfr],
                f32=f32.cpu().numpy()[:80 * nfr].reshape(nfr, 80))


@pytest.mark.parametrize("name", ["gap", "ragged"])
def test_single_frame_slices(name):
    """`gap` alone in 98 launch groups, `ragged` alone in 50 plus one for its 37-sample tail (no whole frame, d_final there):
    every hang-over count, the frameCounter <= 35 switch, every ring position and every history shift is a cut.  The one launch
    of an utterance alone is its rows of the batch (the kernels know no neighbour), so the shared one launch is the reference."""
    utts, want = _fixture_one_launch()
    j = [n for n, *_ in FIXTURE].index(name)
    got = _single_frames(utts[j])
    _assert_features_equal(got, want[j], f"{name} in single-frame slices")
    assert got["onset"] == FIXTURE[j][3]


def test_edge_signals_in_slices():
    """The 14 signals of tests/ns_edge_cases.signals_8k(), longest first, cut at test_b_time_slices_equal_one_launch's cuts plus
    the frameCounter <= 35 switch: the WaveProc bypass on every frame, the raised hang-over, PostProc's middle weight and the
    floored trackers cross slice boundaries.  The one launch's bits."""
    from tests import ns_edge_cases
    sig = ns_edge_cases.signals_8k()
    names = list(sig)
    assert len(names) == 14
    ids, utts = _sorted([sig[n] for n in names])
    assert len(utts[0]) // 80 == EDGE_BOUNDS[-1]
    want = _one_launch(utts)
    got = _in_slices(len(utts), _cuts(utts, EDGE_BOUNDS))
    for j, u in enumerate(ids):
        _assert_features_equal(got[j], want[j], f"edge signal {names[u]}")


def _short_batch():
    from speech_enhancement_amd import corpus
    z = lambda n: np.zeros(n, np.int16)  # noqa: E731
    seeds = (61, 62, 63, 64, 66, 67, 68, 69)  # not the multiples of 5: those utterances start with 400 zeros of their own
    utts = [corpus.synth_utterance(s, 80 * n) for s, n in zip(seeds, (4, 5, 6, 7, 8, 13, 14, 15))]
    utts.append(corpus.synth_utterance(71, 80 * 15 + 37))
    utts.append(np.concatenate([z(3 * 80), corpus.synth_utterance(72, 80 * 40)]))
    utts.append(np.concatenate([z(5 * 80), corpus.synth_utterance(73, 80 * 40)]))
    utts.append(z(80 * 20))
    assert all(x[:80].any() for x in utts[:9])
    return utts


def test_short_utterances_cut_at_every_frame():
    """4, 5, 6, 7, 8, 13, 14, 15 frames, 15 frames + 37 samples, 40 frames behind 3 and behind 5 zero frames, 20 zero frames, cut
    at EVERY frame: the one launch's bits, including the six zero flush rows of the utterances that never produce an output."""
    utts = _short_batch()
    assert [len(x) // 80 for x in utts] == [4, 5, 6, 7, 8, 13, 14, 15, 15, 43, 45, 20] and len(utts[8]) % 80 == 37
    ids, utts = _sorted(utts)
    want = _one_launch(utts)
    got = _in_slices(len(utts), _cuts(utts, tuple(range(46))))
    for j, u in enumerate(ids):
        _assert_features_equal(got[j], want[j], f"short utterance {u} ({len(utts[j])} samples)")
    never = [j for j in range(len(utts)) if want[j]["first_out"] < 0]
    assert never and all(got[j]["n_feat"] == want[j]["onset"] + 6 and not got[j]["feats"][-6:].any() for j in never)
    assert any(want[j]["onset"] == 20 for j in never), "the all-zero utterance: twenty null vectors, then the flush"


def test_the_final_flag():
    """`loud` (60 frames) cut at 0 / 20 / 40 / 60: d_final only in a fourth slice of zero samples gives the bits of d_final on the
    third, which are the one launch's; with no d_final at all the emitted rows are the one launch's first n - 6 and nothing else
    is written."""
    utts, want = _fixture_one_launch()
    j = [n for n, *_ in FIXTURE].index("loud")
    x, w = utts[j], want[j]
    base = _cuts([x], (0, 20, 40, 60))
    assert len(base) == 3
    on_third = _in_slices(1, base)[0]
    _assert_features_equal(on_third, w, "d_final on the third slice")
    no_final = [(b0, parts, None) for b0, parts, _ in base]
    late = _in_slices(1, no_final + [(60, [np.zeros(0, np.int16)], [True])])[0]
    _assert_features_equal(late, w, "d_final on a fourth, empty slice")
    none = _in_slices(1, no_final)[0]
    n = len(w["feats"])
    assert none["n_feat"] == n - 6 and np.array_equal(_u32(none["feats"]), _u32(w["feats"][:n - 6])), \
        f"without d_final: {none['n_feat']} rows, expected the one launch's first {n - 6}"
    assert none["n_ceps"] == w["n_ceps"] and np.array_equal(_u32(none["feat_cc"]), _u32(w["feat_cc"]))


def test_engine_wrappers_in_two_slices():
    """Six utterances cut at frame 41 through the ENGINE wrappers (ns_slice_state, afe_slice_state,
    ns_denoise_batch_slice(.., want_flags=True), afe_features_batch_slice), first_out / onset handed from slice to slice.  Every
    fixture outlasts frame 41, so the sixth utterance is `ragged` cut to 30 frames + its 37-sample tail: six utterances in the
    first slice, five in the second.  Rows, cepstra, counts, flag bytes and audio are the one launch's bits, so an argument out
    of place in either wrapper's call shows."""
    import speech_enhancement_amd as sea
    torch = _torch()
    fixtures, _ = _fixture_one_launch()
    utts = list(fixtures[:5]) + [np.concatenate([fixtures[5][:80 * 30], fixtures[5][80 * 50:]])]
    assert len(utts[5]) == 80 * 30 + 37
    want = _one_launch(utts)
    slices = _cuts(utts, (0, 41, 400))
    assert [len(parts) for _, parts, _ in slices] == [6, 5]
    n_utt = len(utts)
    state, afe = sea.ns_slice_state(n_utt, DEV), sea.afe_slice_state(n_utt, DEV)
    first = onset = None
    keys = ("out", "flags", "feats", "feat_cc", "feat_pp")
    got = [{k: [] for k in keys} for _ in range(n_utt)]
    for k, (b0, parts, final) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        den = sea.ns_denoise_batch_slice(b, state, b0, k > 0, first_out=first, onset=onset, want_flags=True)
        r = sea.afe_features_batch_slice(b, den, afe, b0, k > 0, final=final, want_pp=True)
        torch.cuda.synchronize()
        first, onset = den["first_out"], den["onset"]
        po, hflags = b.split(den["out"], full_frames_only=True), den["flags"].cpu().numpy()
        cc, pp, cum = r["feat_cc"].cpu().numpy(), r["feat_pp"].cpu().numpy(), r["ceps_cum"]
        for u in range(b.n_utt):
            nc = int(r["n_ceps"][u])
            assert len(r["feats"][u]) == int(r["n_feat"][u])
            pg = _flag_bytes(hflags, b.host_offsets[u], len(parts[u]) // 80)
            for key, v in zip(keys, (po[u], pg, r["feats"][u], cc[cum[u]:cum[u] + nc], pp[cum[u]:cum[u] + nc])):
                got[u][key].append(v)
    first, onset = first.cpu().numpy(), onset.cpu().numpy()
    for j in range(n_utt):
        what, w = f"utterance {j} through the wrappers", want[j]
        g = {k: np.concatenate(got[j][k]) for k in keys}
        assert (int(first[j]), int(onset[j])) == (w["first_out"], w["onset"]), what
        assert len(g["feat_cc"]) == w["n_ceps"], f"{what}: {len(g['feat_cc'])} cepstral frames, one launch {w['n_ceps']}"
        for k in ("feats", "feat_cc", "feat_pp"):
            assert g[k].shape == w[k].shape, f"{what}: {k} {g[k].shape} != {w[k].shape}"
            assert np.array_equal(_u32(g[k]), _u32(w[k])), f"{what}: {k} differs in bits from the one launch"
        assert np.array_equal(g["out"], w["out"]), f"{what}: int16 audio differs from the one launch"
        assert np.array_equal(g["flags"], w["flags"]), f"{what}: flag bytes differ from the one launch"


def _assert_final_state(st, want, x, what):
    """st: one utterance's feature-chain state after its last slice, d_final set there (sea_kernels.h, kAfeStateFloats: history
    at 0, ring at 240, lanes at 352, scalars at 384); want: its entry of _one_launch; x: its samples.  Every expected word comes
    from the one launch and the length.  The history is copied from the slice's float stream, so frames before the first
    output hold what that buffer held before the launch: the sentinel."""
    assert st.shape == (392,)
    assert not np.isnan(st).any(), f"{what}: {int(np.isnan(st).sum())} words of the state are still NaN"
    nfr = len(x) // 80
    quiet = want["first_out"] if want["first_out"] >= 0 else nfr
    stream = want["f32"][:nfr].copy()
    stream[:quiet] = SENT_F32
    hist = np.concatenate([np.zeros(240, np.float32), stream.reshape(-1)])[-240:]
    assert np.array_equal(_u32(st[:240]), _u32(hist)), f"{what}: the history is not the float stream's last 240 words"
    scal = st[384:392].view(np.int32)
    assert (int(scal[5]), int(scal[6]), int(scal[7])) == (want["n_ceps"], min(want["onset"], nfr), 1), \
        f"{what}: cepstral frames / null vectors / flushed {scal[5:8]}, expected {want['n_ceps']} / {min(want['onset'], nfr)} / 1"


def test_final_state_words():
    """The words of the state that no later slice reads back: after the last slice (d_final set) the 240 history floats are the
    tail of the one launch's float stream, zeros in front where the utterance is shorter, the three diagnostic integers are the
    one launch's n_ceps, min(onset, frames) and 1, and no word is still the NaN it started as.  Six utterances cut at frame 41
    (test_engine_wrappers_in_two_slices' list) and the short batch cut at every frame."""
    fixtures, _ = _fixture_one_launch()
    six = list(fixtures[:5]) + [np.concatenate([fixtures[5][:80 * 30], fixtures[5][80 * 50:]])]
    for name, utts, bounds in (("six cut at 41", six, (0, 41, 400)), ("short batch", _sorted(_short_batch())[1], tuple(range(46)))):
        want = _one_launch(utts)
        states = []
        _in_slices(len(utts), _cuts(utts, bounds), states=states)
        for j, x in enumerate(utts):
            _assert_final_state(states[0][j], want[j], x, f"{name}, utterance {j} ({len(x)} samples)")


def test_slice_arguments_are_checked():
    """NULL d_afe_state, NULL flags, NULL feat15 / n_feat / feat_cc, negative frame_base; for the _fd slice call NULL flags /
    float stream / state and a negative frame_base: non-zero, the call's name in the message, sentinels intact.  The same calls
    with valid arguments run."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    x = _short_batch()[0]
    assert len(x) == 320
    b = sea.PackedBatch.from_arrays([x], device=DEV)
    T = dict(out=torch.full_like(b.data, SENT_I16),
             f32=torch.full((b.total,), SENT_F32, dtype=torch.float32, device=DEV),
             flags=torch.full((b.total // 8,), SENT_FLAG, dtype=torch.uint8, device=DEV),
             first=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             onset=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             cc=torch.full((4, 14), SENT_F32, dtype=torch.float32, device=DEV),
             f15=torch.full((10, 15), SENT_F32, dtype=torch.float32, device=DEV),
             nf=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             state=torch.zeros((1, int(lib.sea_ns_slice_state_floats())), dtype=torch.float32, device=DEV),
             afe=torch.zeros((1, int(lib.sea_afe_slice_state_floats())), dtype=torch.float32, device=DEV),
             ccum=torch.tensor([0, 4], dtype=torch.int64, device=DEV), fcum=torch.tensor([0, 10], dtype=torch.int64, device=DEV))

    def fd(frame_base=0, **kw):
        t = dict(T, **kw)
        return lib.sea_ns_denoise_batch_slice_fd(_p(b.data), _p(t["out"]), _p(t["f32"]), _p(b.offsets), _p(b.lengths), None,
                                                 _p(t["first"]), _p(t["flags"]), _p(t["onset"]), _p(t["state"]), 1, frame_base, 0, None)

    def feat(frame_base=0, **kw):
        t = dict(T, **kw)
        return lib.sea_afe_features_batch_slice(_p(t["f32"]), _p(t["flags"]), _p(b.offsets), _p(b.lengths), _p(t["first"]),
                                                _p(t["onset"]), None, _p(t["ccum"]), 4, _p(t["cc"]), None, _p(t["fcum"]), _p(t["f15"]),
                                                _p(t["nf"]), None, _p(t["afe"]), 1, frame_base, 0, None)

    for call, name, cases in (
            (fd, "sea_ns_denoise_batch_slice_fd", (("NULL flags", dict(flags=None)), ("NULL float stream", dict(f32=None)),
                                                   ("NULL state", dict(state=None)), ("negative frame_base", dict(frame_base=-1)))),
            (feat, "sea_afe_features_batch_slice", (("NULL d_afe_state", dict(afe=None)), ("NULL flags", dict(flags=None)),
                                                    ("negative frame_base", dict(frame_base=-1)), ("NULL feat15", dict(f15=None)),
                                                    ("NULL n_feat", dict(nf=None)), ("NULL feat_cc", dict(cc=None))))):
        for what, kw in cases:
            rc = call(**kw)
            msg = lib.sea_last_error().decode()
            assert rc != 0 and msg.startswith(name + ":"), f"{name}, {what}: rc {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert (T["out"].cpu().numpy() == SENT_I16).all() and (T["first"].cpu().numpy() == SENT_INT).all() \
        and (T["nf"].cpu().numpy() == SENT_INT).all() and _is_sent(T["f15"].cpu().numpy()) \
        and (T["flags"].cpu().numpy() == SENT_FLAG).all(), "a refused call launched something"
    assert fd() == 0, lib.sea_last_error()
    assert feat() == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    assert int(T["first"].cpu()[0]) == -1 and int(T["onset"].cpu()[0]) == 0 and int(T["nf"].cpu()[0]) == 0
    assert _is_sent(T["f15"].cpu().numpy()) and _is_sent(T["cc"].cpu().numpy())  # four frames, no d_final: nothing emitted
    assert not T["out"].cpu().numpy()[:320].any()


def test_host_pipeline_equals_one_launch():
    """features_utterances on (i) the six fixtures plus 31 short synthetic utterances of 0 .. 40 frames, some ragged, one empty,
    one all-zero, (ii) ONE utterance of 120 s, (iii) twelve utterances of 2000 .. 0 frames, some ragged.  (ii) and (iii) must be
    cut into several launches.  Rows and counts are the one launch's bit for bit, a list run twice gives the same bits,
    SEA_HOST_SLICES=3 gives the bits of the default, and the audio, where asked for, is ns_denoise_batch's."""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    torch = _torch()
    fixtures, _ = _fixture_one_launch()
    utts = list(fixtures)
    for i in range(29):
        n = 1 + (i * 11) % 40
        utts.append(corpus.synth_utterance(60 + i, 80 * n + (0 if i % 3 else 17 + i)))
    utts += [np.zeros(0, np.int16), np.zeros(80 * 9 + 5, np.int16)]
    assert len(utts) == 37 and sum(len(x) % 80 != 0 for x in utts) >= 10
    long_one = np.tile(corpus.synth_utterance(3, 32000), 30)
    assert len(long_one) == 8000 * 120
    ragged = [corpus.synth_utterance(100 + i, 80 * n + (0 if i % 3 else 17 + i))
              for i, n in enumerate((2000, 1500, 1200, 900, 700, 500, 300, 200, 100, 40, 9, 0))]
    saved = os.environ.pop("SEA_HOST_SLICES", None)
    try:
        for name, lst, cut in (("short list", utts, False), ("one long utterance", [long_one], True),
                               ("cut and ragged list", ragged, True)):
            want = _one_launch(lst)
            b = sea.PackedBatch.from_arrays(lst, device=DEV)
            audio = b.split(sea.ns_denoise_batch(b)[0], full_frames_only=True)
            torch.cuda.synchronize()
            got = sea.features_utterances(lst, want_out=True)
            plain = sea.features_utterances(lst)
            again = sea.features_utterances(lst)
            os.environ["SEA_HOST_SLICES"] = "3"
            three = sea.features_utterances(lst)
            del os.environ["SEA_HOST_SLICES"]
            if cut:
                assert got["slices"] > 1 and plain["slices"] > 1, f"{name}: run as {got['slices']} launch(es)"
                assert 1 < three["slices"] <= 3, f"{name}: SEA_HOST_SLICES=3 ran as {three['slices']} launch(es)"
            else:
                assert got["slices"] == three["slices"] == 1, f"{name}: a small list is one slice"
            for u, w in enumerate(want):
                what = f"{name}, utterance {u} ({len(lst[u])} samples)"
                for r in (got, plain, again, three):
                    assert r["feats"][u].shape == w["feats"].shape, f"{what}: {len(r['feats'][u])} rows, one launch {len(w['feats'])}"
                    assert np.array_equal(_u32(r["feats"][u]), _u32(w["feats"])), f"{what}: rows differ in bits from the one launch"
                whole = len(lst[u]) // 80 * 80
                assert np.array_equal(got["out"][u][:whole], audio[u]) and np.array_equal(audio[u], w["out"]), f"{what}: audio"
                assert not got["out"][u][whole:].any(), f"{what}: the trailing partial frame was written"
            print(f"\n{name}: {len(lst)} utterance(s), {got['slices']} launch(es), {sum(len(w['feats']) for w in want)} rows equal to the one launch bit for bit")
    finally:
        if saved is not None:
            os.environ["SEA_HOST_SLICES"] = saved
