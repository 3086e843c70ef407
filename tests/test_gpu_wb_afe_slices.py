"""GPU tests of the wideband (16 kHz) FEATURE CHAIN in TIME SLICES (sea_wb_denoise_batch_slice_fd +
sea_wb_afe_features_batch_slice, sea_wb_features_utterances): an utterance cut along the time axis, one launch group per
slice, the feature side's own state carried per utterance -- three frames of the low band's float stream, two high-band and
code rows, PostProc's weights, the VAD's feature buffer, ring of seven and counters.

The criterion is exact: concatenated over an utterance's slices, feats, feat_cc, feat_pp and the flag bytes are the BITS of the
one launch (wb_afe_features_batch, which these tests do not touch), floats compared as uint32, and the counts sum to its
counts.  So that both sides cannot be wrong together, test 1 also holds the sliced result against the reference's recorded
outputs (tests/golden/wb_afe_golden.npz) with tests/test_gpu_wb_afe.py's limits: 1e-3 on features, zero tolerance on counts,
VAD flags, flag bytes and null positions.

Inputs are the fixture's seven utterances (frames of 160 / ragged tail / first output / onset: 100 / 0 / 4 / 0, 100 / 0 / 6 / 2,
300 / 0 / 4 / 0, 300 / 0 / 4 / 0, 303 / 77 / 7 / 3, 4 / 0 / none / 0, 200 / 0 / 4 / 0; utterance 6 has 117 frames on WaveProc's
bypass and 77 through it).  Run on an MI355X with ``pytest -m gpu``."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wb_afe_golden.npz")
N_FIXTURE = 7
SENT_I16 = 12321          # what every output holds before a launch
SENT_F32 = 54321.5
SENT_INT = -77
SENT_FLAG = 0xA5
BOUNDS = tuple(range(17)) + (40, 41, 97, 150, 303)
FIXTURE = {  # frames of 160, ragged tail, first output, onset: the fixture's own numbers
    0: (100, 0, 4, 0), 1: (100, 0, 6, 2), 2: (300, 0, 4, 0), 3: (300, 0, 4, 0), 4: (303, 77, 7, 3), 5: (4, 0, -1, 0),
    6: (200, 0, 4, 0)}
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


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    for u, (nfr, tail, first, onset) in FIXTURE.items():
        assert (len(g[f"x{u}"]) // 160, len(g[f"x{u}"]) % 160, int(g["first_out"][u]), int(g["onset"][u])) == (nfr, tail, first, onset)
    return g


def _sorted(utts):
    """longest first (stable), so that the utterances of a later slice are a prefix of the list"""
    ids = sorted(range(len(utts)), key=lambda u: -(len(utts[u]) // 160))
    return ids, [utts[u] for u in ids]


def _one_launch(utts):
    """wb_afe_features_batch on the list -> per utterance dict of numpy arrays; rows of frames without an output are zero"""
    import speech_enhancement_amd as sea
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device=DEV)
    r = sea.wb_afe_features_batch(b, want_intermediates=True)
    torch.cuda.synchronize()
    out, f32 = sea.wb_split(b, r["out"]), sea.wb_split(b, r["f32"])
    flags, hpr, code = (sea.wb_rows(b, r[k]) for k in ("flag_rows", "hp_rows", "code_rows"))
    first, onset, n_ceps = (r[k].cpu().numpy() for k in ("first_out", "onset", "n_ceps"))
    cc, pp, cum = r["feat_cc"].cpu().numpy(), r["feat_pp"].cpu().numpy(), r["ceps_cum"]
    res = []
    for u, x in enumerate(utts):
        nc = int(n_ceps[u])
        res.append(dict(feats=r["feats"][u], n_ceps=nc, feat_cc=cc[cum[u]:cum[u] + nc], feat_pp=pp[cum[u]:cum[u] + nc],
                        flags=flags[u], out=out[u], f32=f32[u].reshape(-1, 80), hp=hpr[u], code=code[u],
                        first_out=int(first[u]), onset=int(onset[u])))
    return res


@functools.lru_cache(maxsize=None)
def _fixture_one_launch():
    """the seven fixtures, longest first, through the one launch: computed once, nothing modifies it"""
    g = _gold()
    ids, utts = _sorted([g[f"x{u}"] for u in range(N_FIXTURE)])
    assert ids == [4, 2, 3, 6, 0, 1, 5]
    return ids, utts, _one_launch(utts)


def _cuts(utts, bounds, final=True):
    """[(frame_base, the active prefix's parts, final bytes or None)]: the list (longest first) cut at `bounds` (frames of 160);
    an utterance's last slice carries its ragged tail and, with `final`, its flush"""
    nfr = [len(x) // 160 for x in utts]
    assert nfr == sorted(nfr, reverse=True) and bounds[0] == 0 and bounds[-1] >= nfr[0]
    slices = []
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        act = [u for u in range(len(utts)) if nfr[u] > b0]
        assert act == list(range(len(act)))
        if not act:
            break
        parts = [utts[u][160 * b0:160 * b1] if b1 < nfr[u] else utts[u][160 * b0:] for u in act]
        slices.append((b0, parts, [b1 >= nfr[u] for u in act] if final else None))
    return slices


def _in_slices(n_utt, slices, features=True, states=None):
    """One launch group per slice into sentinel-filled buffers: sea_wb_denoise_batch_slice_fd + sea_wb_afe_features_batch_slice
    (features) or the plain sea_wb_denoise_batch_slice.  Both states start as NaN: resume = 0 must not read them.  Returns per
    utterance the concatenated pieces and the summed counts; `states`, a list, receives the feature chain's state after
    the last slice, one row per utterance."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    state = torch.full((n_utt, int(lib.sea_wb_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    afe = torch.full((n_utt, int(lib.sea_wb_afe_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    first = torch.full((n_utt,), SENT_INT, dtype=torch.int32, device=DEV)
    onset = torch.full((n_utt,), SENT_INT, dtype=torch.int32, device=DEV)
    keys = ("out", "f32", "hp", "code", "flags", "feat_cc", "feat_pp", "feats")
    got = [{k: [] for k in keys} for _ in range(n_utt)]
    n_feat, n_ceps = np.zeros(n_utt, np.int64), np.zeros(n_utt, np.int64)
    for k, (b0, parts, final) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        n = b.n_utt
        half = (b.total // 2 + 7) // 8 * 8
        rows = int(lib.sea_wb_rows(b.total))
        out = torch.full((half,), SENT_I16, dtype=torch.int16, device=DEV)
        f32 = torch.full((half,), SENT_F32, dtype=torch.float32, device=DEV)
        hp = torch.full((rows, 3), SENT_F32, dtype=torch.float32, device=DEV)
        code = torch.full((rows, 9), SENT_F32, dtype=torch.float32, device=DEV)
        flags = torch.full((rows,), SENT_FLAG, dtype=torch.uint8, device=DEV)
        scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(b.total, n)) // 4 + 4, dtype=torch.float32, device=DEV)
        if not features:
            rc = lib.sea_wb_denoise_batch_slice(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order), _p(first),
                                                _p(onset), _p(hp), _p(code), _p(scratch), b.total, _p(state), n, b0,
                                                1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
        else:
            rc = lib.sea_wb_denoise_batch_slice_fd(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                                   _p(first), _p(onset), _p(flags), _p(hp), _p(code), _p(scratch), b.total,
                                                   _p(state), n, b0, 1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
            fr = np.array([len(x) // 160 for x in parts], np.int64)
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
            rc = lib.sea_wb_afe_features_batch_slice(_p(f32), _p(flags), _p(hp), _p(code), _p(b.offsets), _p(b.lengths), _p(first),
                                                     _p(onset), _p(d_final), _p(d_ccum), tc, _p(cc), _p(pp), _p(d_fcum), _p(f15),
                                                     _p(nf), _p(nc), _p(afe), n, b0, 1 if k > 0 else 0, None)
            assert rc == 0, lib.sea_last_error()
        torch.cuda.synchronize()
        po, pf = sea.wb_split(b, out), sea.wb_split(b, f32)
        ph, pc, pg = sea.wb_rows(b, hp), sea.wb_rows(b, code), sea.wb_rows(b, flags)
        for u in range(n):
            for key, v in zip(("out", "f32", "hp", "code", "flags"), (po[u], pf[u].reshape(-1, 80), ph[u], pc[u], pg[u])):
                got[u][key].append(v)
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
    assert (got["flags"][:quiet] == SENT_FLAG).all(), f"{what}: flag rows of frames without an output were written"
    assert np.array_equal(got["flags"][quiet:], want["flags"][quiet:]), f"{what}: flag bytes differ from the one launch"
    assert np.array_equal(got["out"], want["out"]), f"{what}: low band differs from the one launch"
    for k in ("f32", "hp", "code"):
        assert _is_sent(got[k][:quiet]), f"{what}: {k} of frames without an output was written"
        assert np.array_equal(_u32(got[k][quiet:]), _u32(want[k][quiet:])), f"{what}: {k} differs in bits from the one launch"


def test_slices_equal_one_launch():
    """All seven fixtures, longest first, cut at BOUNDS: every frame of the zero lead and of the four-frame latency, the first
    cepstral frame (first output + 2), the first emission (first output + 8: frames 12, 14, 15), inside the ring of 7 and the
    tile of 8, past the end of 5, then 0/1, then 6; d_final on each utterance's last slice.  Everything equals the one launch
    bit for bit, what the _fd slice shares with sea_wb_denoise_batch_slice equals that call's on the same cuts, and the sliced
    result is within the fixture's limits."""
    from tests.test_gpu_wb_afe import _Stats, _compare
    g = _gold()
    ids, utts, want = _fixture_one_launch()
    slices = _cuts(utts, BOUNDS)
    got = _in_slices(len(utts), slices)
    plain = _in_slices(len(utts), slices, features=False)
    st = _Stats()
    for j, u in enumerate(ids):
        what = f"fixture utterance {u}"
        _assert_features_equal(got[j], want[j], what)
        assert (got[j]["first_out"], got[j]["onset"]) == (plain[j]["first_out"], plain[j]["onset"]) == FIXTURE[u][2:]
        assert np.array_equal(got[j]["out"], plain[j]["out"]), f"{what}: low band != sea_wb_denoise_batch_slice's"
        for k in ("f32", "hp", "code"):
            assert np.array_equal(_u32(got[j][k]), _u32(plain[j][k])), f"{what}: {k} != sea_wb_denoise_batch_slice's"
        fo = FIXTURE[u][2]
        quiet = fo if fo >= 0 else FIXTURE[u][0]
        flags = got[j]["flags"].copy()
        flags[:quiet] = 0  # checked above to hold the sentinel: the fixture's comparison expects unwritten rows as zeros
        mine = dict(got[j], flags=flags, cc_cap=got[j]["feat_cc"])
        ref = dict(feat_cc=g[f"feat_cc{u}"], feat_pp=g[f"feat_pp{u}"], feat15=g[f"feat15_{u}"], flags=g[f"flags{u}"],
                   first_out=int(g["first_out"][u]), onset=int(g["onset"][u]))
        _compare(st, mine, ref, FIXTURE[u][0], what + " in slices")
    st.report(f"{len(slices)} slices against the fixture")
    st.check()


def _single_frames(x):
    """One utterance alone, one launch group per frame (and one for a ragged tail), pointers advanced frame by frame into
    buffers of the whole utterance; per-slice feature blocks of 1 cepstral and 7 emitted rows.  One read-back at the end."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    nfr, tail = len(x) // 160, len(x) % 160
    ns = nfr + (1 if tail else 0)
    xin = np.zeros(160 * (nfr + 1), np.int16)
    xin[:len(x)] = x
    d_in = torch.from_numpy(xin).to(DEV)
    out = torch.full((80 * (nfr + 1),), SENT_I16, dtype=torch.int16, device=DEV)
    f32 = torch.full((80 * (nfr + 1),), SENT_F32, dtype=torch.float32, device=DEV)
    hp = torch.full((nfr + 2, 3), SENT_F32, dtype=torch.float32, device=DEV)
    code = torch.full((nfr + 2, 9), SENT_F32, dtype=torch.float32, device=DEV)
    flags = torch.full((nfr + 2,), SENT_FLAG, dtype=torch.uint8, device=DEV)
    first = torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV)
    onset = torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV)
    meta = torch.tensor([0, 160, 0, 1, 0, 7], dtype=torch.int64, device=DEV)       # offsets | lengths | ceps_cum | feat_cum
    meta_t = torch.tensor([0, tail, 0, 0, 0, 6], dtype=torch.int64, device=DEV)    # the tail: no whole frame
    one = torch.ones(1, dtype=torch.uint8, device=DEV)
    state = torch.full((1, int(lib.sea_wb_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    afe = torch.full((1, int(lib.sea_wb_afe_slice_state_floats())), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(160, 1)) // 4 + 4, dtype=torch.float32, device=DEV)
    cc = torch.full((ns, 14), SENT_F32, dtype=torch.float32, device=DEV)
    pp = torch.full((ns, 14), SENT_F32, dtype=torch.float32, device=DEV)
    f15 = torch.full((ns, 7, 15), SENT_F32, dtype=torch.float32, device=DEV)
    nf = torch.full((ns,), SENT_INT, dtype=torch.int32, device=DEV)
    nc = torch.full((ns,), SENT_INT, dtype=torch.int32, device=DEV)
    for f in range(ns):
        is_tail = f == nfr
        m = meta_t if is_tail else meta
        total = (tail + 7) // 8 * 8 if is_tail else 160
        rc = lib.sea_wb_denoise_batch_slice_fd(_p(d_in, 320 * f), _p(out, 160 * f), _p(f32, 320 * f), _p(m), _p(m, 8), None, _p(first),
                                               _p(onset), _p(flags, f), _p(hp, 12 * f), _p(code, 36 * f), _p(scratch), total,
                                               _p(state), 1, f, 1 if f > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
        rc = lib.sea_wb_afe_features_batch_slice(_p(f32, 320 * f), _p(flags, f), _p(hp, 12 * f), _p(code, 36 * f), _p(m), _p(m, 8),
                                                 _p(first), _p(onset), _p(one) if f == ns - 1 else None, _p(m, 16),
                                                 0 if is_tail else 1, _p(cc, 56 * f), _p(pp, 56 * f), _p(m, 32), _p(f15, 420 * f),
                                                 _p(nf, 4 * f), _p(nc, 4 * f), _p(afe), 1, f, 1 if f > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    hcc, hpp, h15, hnf, hnc = (t.cpu().numpy() for t in (cc, pp, f15, nf, nc))
    assert ((hnc == 0) | (hnc == 1)).all() and (hnf[:-1] <= 1).all() and 0 <= hnf[-1] <= 7, "a slice's counts are out of range"
    for f in range(ns):
        assert _is_sent(hcc[f][None][hnc[f]:]) and _is_sent(h15[f][hnf[f]:]), f"slice {f}: rows behind the counts were written"
    return dict(first_out=int(first.cpu()[0]), onset=int(onset.cpu()[0]), n_feat=int(hnf.sum()), n_ceps=int(hnc.sum()),
                feat_cc=hcc[hnc == 1], feat_pp=hpp[hnc == 1], feats=np.concatenate([h15[f][:hnf[f]] for f in range(ns)]),
                flags=flags.cpu().numpy()[:nfr], out=out.cpu().numpy()[:80 * nfr], f32=f32.cpu().numpy()[:80 * nfr].reshape(nfr, 80),
                hp=hp.cpu().numpy()[:nfr], code=code.cpu().numpy()[:nfr])


@pytest.mark.parametrize("u", [6, 4])
def test_single_frame_slices(u):
    """Fixture 6 alone in 200 launch groups, fixture 4 alone in 303 plus one for its 77-sample tail: every hang-over count, the
    frameCounter <= 35 switch, every ring position and every history shift is a cut.  The one launch of the utterance alone is
    its rows of the batch (tests/test_gpu_wb_afe.py::test_c_composition), so the shared one-launch result is the reference."""
    ids, utts, want = _fixture_one_launch()
    j = ids.index(u)
    got = _single_frames(utts[j])
    _assert_features_equal(got, want[j], f"fixture utterance {u} in single-frame slices")
    assert (got["first_out"], got["onset"]) == FIXTURE[u][2:]


def test_short_utterances_cut_at_every_frame():
    """4, 5, 6, 7, 8, 13, 14, 15 frames, 15 frames + 77 samples, 40 frames behind 3 zero frames, 40 behind 400 zeros, 20 zero
    frames (tests/test_gpu_wb_afe.py::_edge_batch), cut at EVERY frame: the one launch's bits, including the six flush rows of
    the utterances that never produce an output."""
    from tests.test_gpu_wb_afe import _edge_batch
    utts = _edge_batch()[0][:12]
    assert [len(x) // 160 for x in utts] == [4, 5, 6, 7, 8, 13, 14, 15, 15, 43, 42, 20] and len(utts[8]) % 160 == 77
    ids, utts = _sorted(utts)
    want = _one_launch(utts)
    got = _in_slices(len(utts), _cuts(utts, tuple(range(44))))
    for j, u in enumerate(ids):
        _assert_features_equal(got[j], want[j], f"edge utterance {u} ({len(utts[j])} samples)")
    never = [j for j in range(len(utts)) if want[j]["first_out"] < 0]
    assert never and all(got[j]["n_feat"] == want[j]["onset"] + 6 and not got[j]["feats"][-6:].any() for j in never)


def test_the_final_flag():
    """Fixture 0 in three slices: d_final only in a fourth slice of zero samples gives the bits of d_final on the third; with no
    d_final at all the emitted rows are the one launch's first n - 6 and nothing else is written."""
    ids, utts, want = _fixture_one_launch()
    j = ids.index(0)
    x, w = utts[j], want[j]
    base = _cuts([x], (0, 30, 60, 100))
    on_third = _in_slices(1, base)[0]
    _assert_features_equal(on_third, w, "d_final on the third slice")
    no_final = [(b0, parts, None) for b0, parts, _ in base]
    late = _in_slices(1, no_final + [(100, [np.zeros(0, np.int16)], [True])])[0]
    _assert_features_equal(late, w, "d_final on a fourth, empty slice")
    none = _in_slices(1, no_final)[0]
    n = len(w["feats"])
    assert none["n_feat"] == n - 6 and np.array_equal(_u32(none["feats"]), _u32(w["feats"][:n - 6])), \
        f"without d_final: {none['n_feat']} rows, expected the one launch's first {n - 6}"
    assert none["n_ceps"] == w["n_ceps"] and np.array_equal(_u32(none["feat_cc"]), _u32(w["feat_cc"]))


def test_engine_wrappers_in_two_slices():
    """The seven fixtures cut at frame 41 through the ENGINE wrappers (wb_slice_state, wb_afe_slice_state,
    wb_denoise_batch_slice(.., want_flags=True), wb_afe_features_batch_slice), first_out / onset handed from slice to slice:
    seven utterances in the first slice, six in the second.  Rows, cepstra, counts and the low band are the one launch's bits, so
    an argument out of place in either wrapper's call shows."""
    import speech_enhancement_amd as sea
    torch = _torch()
    ids, utts, want = _fixture_one_launch()
    slices = _cuts(utts, (0, 41, 303))
    assert [len(parts) for _, parts, _ in slices] == [7, 6]
    n_utt = len(utts)
    state, afe = sea.wb_slice_state(n_utt, DEV), sea.wb_afe_slice_state(n_utt, DEV)
    first = onset = None
    keys = ("out", "flags", "feats", "feat_cc", "feat_pp")
    got = [{k: [] for k in keys} for _ in range(n_utt)]
    for k, (b0, parts, final) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        den = sea.wb_denoise_batch_slice(b, state, b0, k > 0, first_out=first, onset=onset, want_flags=True)
        r = sea.wb_afe_features_batch_slice(b, den, afe, b0, k > 0, final=final, want_pp=True)
        torch.cuda.synchronize()
        first, onset = den["first_out"], den["onset"]
        po, pg = sea.wb_split(b, den["out"]), sea.wb_rows(b, den["flag_rows"])
        cc, pp, cum = r["feat_cc"].cpu().numpy(), r["feat_pp"].cpu().numpy(), r["ceps_cum"]
        for u in range(b.n_utt):
            nc = int(r["n_ceps"][u])
            assert len(r["feats"][u]) == int(r["n_feat"][u])
            for key, v in zip(keys, (po[u], pg[u], r["feats"][u], cc[cum[u]:cum[u] + nc], pp[cum[u]:cum[u] + nc])):
                got[u][key].append(v)
    first, onset = first.cpu().numpy(), onset.cpu().numpy()
    for j, u in enumerate(ids):
        what, w = f"fixture utterance {u} through the wrappers", want[j]
        g = {k: np.concatenate(got[j][k]) for k in keys}
        assert (int(first[j]), int(onset[j])) == (w["first_out"], w["onset"]) == FIXTURE[u][2:], what
        assert len(g["feat_cc"]) == w["n_ceps"], f"{what}: {len(g['feat_cc'])} cepstral frames, one launch {w['n_ceps']}"
        for k in ("feats", "feat_cc", "feat_pp"):
            assert g[k].shape == w[k].shape, f"{what}: {k} {g[k].shape} != {w[k].shape}"
            assert np.array_equal(_u32(g[k]), _u32(w[k])), f"{what}: {k} differs in bits from the one launch"
        assert np.array_equal(g["out"], w["out"]), f"{what}: low band differs from the one launch"
        assert np.array_equal(g["flags"], w["flags"]), f"{what}: flag bytes differ from the one launch"


def _assert_final_state(st, want, x, what):
    """st: one utterance's feature-chain state after its last slice, d_final set there (sea_kernels.h, kWbAfeStateFloats:
    history at 0, high-band rows at 240, code rows at 248, ring at 272, lanes at 384, scalars at 416); want: its entry of
    _one_launch; x: its samples.  Every expected word comes from the one launch and the length.  History and rows are copied
    from the slice's buffers, so frames before the first output hold what those held before the launch: the sentinel."""
    assert st.shape == (424,)
    assert not np.isnan(st).any(), f"{what}: {int(np.isnan(st).sum())} words of the state are still NaN"
    nfr = len(x) // 160
    quiet = want["first_out"] if want["first_out"] >= 0 else nfr
    for key, at, keep, pad in (("f32", 0, 240, 0), ("hp", 240, 6, 2), ("code", 248, 18, 6)):
        rows = want[key][:nfr].copy()
        rows[:quiet] = SENT_F32
        tail = np.concatenate([np.zeros(keep, np.float32), rows.reshape(-1)])[-keep:]
        assert np.array_equal(_u32(st[at:at + keep]), _u32(tail)), f"{what}: {key} words of the state are not the one launch's last"
        assert not _u32(st[at + keep:at + keep + pad]).any(), f"{what}: the padding behind the {key} rows is not zero"
    scal = st[416:424].view(np.int32)
    assert (int(scal[5]), int(scal[6]), int(scal[7])) == (want["n_ceps"], min(want["onset"], nfr), 1), \
        f"{what}: cepstral frames / null vectors / flushed {scal[5:8]}, expected {want['n_ceps']} / {min(want['onset'], nfr)} / 1"


def test_final_state_words():
    """The words of the state that no later slice reads back: after the last slice (d_final set) the 240 history floats are the
    tail of the one launch's low-band float stream and the 2 x 3 / 2 x 9 rows the last two frames' rows, zeros in front where
    the utterance is shorter and in words 6-7 / 18-23 of the row blocks; the three diagnostic integers are the one launch's
    n_ceps, min(onset, frames) and 1, and no word is still the NaN it started as.  The seven fixtures cut at frame 41 and the
    short batch cut at every frame."""
    from tests.test_gpu_wb_afe import _edge_batch
    _, fixtures, fixture_want = _fixture_one_launch()
    short = _sorted(_edge_batch()[0][:12])[1]
    for name, utts, want, bounds in (("fixtures cut at 41", fixtures, fixture_want, (0, 41, 303)),
                                     ("short batch", short, None, tuple(range(44)))):
        want = want if want is not None else _one_launch(utts)
        states = []
        _in_slices(len(utts), _cuts(utts, bounds), states=states)
        for j, x in enumerate(utts):
            _assert_final_state(states[0][j], want[j], x, f"{name}, utterance {j} ({len(x)} samples)")


def test_slice_arguments_are_checked():
    """NULL d_afe_state, NULL flag rows, negative frame_base, a NULL among the required outputs; for the _fd slice call NULL flag
    rows / float stream: non-zero, the call's name in the message, sentinels intact.  The same calls with valid arguments run."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    x = _gold()["x5"]
    b = sea.PackedBatch.from_arrays([x], device=DEV)
    half, rows = (b.total // 2 + 7) // 8 * 8, int(lib.sea_wb_rows(b.total))
    T = dict(out=torch.full((half,), SENT_I16, dtype=torch.int16, device=DEV),
             f32=torch.full((half,), SENT_F32, dtype=torch.float32, device=DEV),
             hp=torch.full((rows, 3), SENT_F32, dtype=torch.float32, device=DEV),
             code=torch.full((rows, 9), SENT_F32, dtype=torch.float32, device=DEV),
             flags=torch.full((rows,), SENT_FLAG, dtype=torch.uint8, device=DEV),
             first=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             onset=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             cc=torch.full((4, 14), SENT_F32, dtype=torch.float32, device=DEV),
             f15=torch.full((10, 15), SENT_F32, dtype=torch.float32, device=DEV),
             nf=torch.full((1,), SENT_INT, dtype=torch.int32, device=DEV),
             state=torch.zeros((1, int(lib.sea_wb_slice_state_floats())), dtype=torch.float32, device=DEV),
             afe=torch.zeros((1, int(lib.sea_wb_afe_slice_state_floats())), dtype=torch.float32, device=DEV),
             ccum=torch.tensor([0, 4], dtype=torch.int64, device=DEV), fcum=torch.tensor([0, 10], dtype=torch.int64, device=DEV))
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(b.total, 1)) // 4 + 4, dtype=torch.float32, device=DEV)

    def fd(frame_base=0, **kw):
        t = dict(T, **kw)
        return lib.sea_wb_denoise_batch_slice_fd(_p(b.data), _p(t["out"]), _p(t["f32"]), _p(b.offsets), _p(b.lengths), None,
                                                 _p(t["first"]), _p(t["onset"]), _p(t["flags"]), _p(t["hp"]), _p(t["code"]),
                                                 _p(scratch), b.total, _p(t["state"]), 1, frame_base, 0, None)

    def feat(frame_base=0, **kw):
        t = dict(T, **kw)
        return lib.sea_wb_afe_features_batch_slice(_p(t["f32"]), _p(t["flags"]), _p(t["hp"]), _p(t["code"]), _p(b.offsets),
                                                   _p(b.lengths), _p(t["first"]), _p(t["onset"]), None, _p(t["ccum"]), 4,
                                                   _p(t["cc"]), None, _p(t["fcum"]), _p(t["f15"]), _p(t["nf"]), None, _p(t["afe"]),
                                                   1, frame_base, 0, None)

    for call, name, cases in (
            (fd, "sea_wb_denoise_batch_slice_fd", (("NULL flag rows", dict(flags=None)), ("NULL float stream", dict(f32=None)),
                                                   ("NULL state", dict(state=None)), ("negative frame_base", dict(frame_base=-1)))),
            (feat, "sea_wb_afe_features_batch_slice", (("NULL d_afe_state", dict(afe=None)), ("NULL flag rows", dict(flags=None)),
                                                       ("negative frame_base", dict(frame_base=-1)), ("NULL feat15", dict(f15=None)),
                                                       ("NULL n_feat", dict(nf=None)), ("NULL feat_cc", dict(cc=None))))):
        for what, kw in cases:
            rc = call(**kw)
            msg = lib.sea_last_error().decode()
            assert rc != 0 and name in msg, f"{name}, {what}: rc {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert (T["out"].cpu().numpy() == SENT_I16).all() and (T["first"].cpu().numpy() == SENT_INT).all() \
        and (T["nf"].cpu().numpy() == SENT_INT).all() and _is_sent(T["f15"].cpu().numpy()), "a refused call launched something"
    assert fd() == 0, lib.sea_last_error()
    assert feat() == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    assert int(T["first"].cpu()[0]) == -1 and int(T["onset"].cpu()[0]) == 0 and int(T["nf"].cpu()[0]) == 0
    assert _is_sent(T["f15"].cpu().numpy()) and _is_sent(T["cc"].cpu().numpy())  # four frames, no d_final: nothing emitted


def test_host_pipeline_equals_one_launch():
    """wb_features_utterances on (i) the seven fixtures plus 31 short synthetic utterances of 0 .. 40 frames, some ragged, one
    empty, one all-zero, (ii) ONE utterance of 120 s, (iii) twelve utterances of 2000 .. 0 frames, some ragged.  (ii) and (iii)
    must be cut into several launches.  Rows and counts are the one launch's bit for bit, a cut list run twice gives the same
    bits, and the low band, where asked for, is wb_denoise_utterances'."""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    _torch()
    g = _gold()
    utts = [g[f"x{u}"] for u in range(N_FIXTURE)]
    for i in range(29):
        n = 1 + (i * 11) % 40
        L = 160 * n + (0 if i % 3 else 17 + i)
        utts.append(corpus.synth_wideband(60 + i, L) if i % 2 else corpus.synth_utterance(60 + i, L))
    utts += [np.zeros(0, np.int16), np.zeros(160 * 9 + 5, np.int16)]
    assert len(utts) == 38 and sum(len(x) % 160 != 0 for x in utts) >= 10
    long_one = np.tile(corpus.synth_wideband(3, 16000 * 4), 30)
    assert len(long_one) == 16000 * 120
    ragged = []
    for i, n in enumerate((2000, 1500, 1200, 900, 700, 500, 300, 200, 100, 40, 9, 0)):
        L = 160 * n + (0 if i % 3 else 17 + i)
        ragged.append(corpus.synth_wideband(100 + i, L) if i % 2 else corpus.synth_utterance(100 + i, L))
    for name, lst, cut in (("short list", utts, False), ("one long utterance", [long_one], True), ("cut and ragged list", ragged, True)):
        want = _one_launch(lst)
        got = sea.wb_features_utterances(lst, want_lp=True)
        plain = sea.wb_features_utterances(lst)
        lp = sea.wb_denoise_utterances(lst)["out"]
        again = None
        if cut:
            assert got["slices"] > 1 and plain["slices"] > 1, f"{name}: run as {got['slices']} launch(es)"
            again = sea.wb_features_utterances(lst)
        for u, w in enumerate(want):
            what = f"{name}, utterance {u} ({len(lst[u])} samples)"
            for r in (got, plain, again):
                if r is None:
                    continue
                assert r["feats"][u].shape == w["feats"].shape, f"{what}: {len(r['feats'][u])} rows, one launch {len(w['feats'])}"
                assert np.array_equal(_u32(r["feats"][u]), _u32(w["feats"])), f"{what}: rows differ in bits from the one launch"
            assert np.array_equal(got["out"][u], lp[u]) and np.array_equal(lp[u], w["out"]), f"{what}: low band"
        print(f"\n{name}: {len(lst)} utterance(s), {got['slices']} launch(es), {sum(len(w['feats']) for w in want)} rows equal to the one launch bit for bit")


def _edge_set():
    """the wideband edge set (tests/ns_edge_cases.signals_wb()), longest first, and the bounds tests/wb_edge_cuts.py derives
    from the reference: -> (names, utterances, bounds)"""
    from tests import ns_edge_cases as E
    from tests import wb_edge_cuts as K
    from tests.test_gpu_wb_afe import _reference
    _reference()                         # the cuts come from the reference run live: a missing library is a failure
    sig = E.signals_wb()
    names = list(sig)
    ids, utts = _sorted([sig[k] for k in names])
    return [names[u] for u in ids], utts, K.bounds()


def test_edge_set_in_slices():
    """The eight signals of the wideband edge set, longest first, cut where the reference says their branches are taken:
    every frame of the first thirteen (the first ten frames' rules, the 12-frame utterance whose flush raises the hang-over),
    one-frame slices across the frames at which WaveProc first finds no neighbouring maximum (16, 34), at which speech is
    first found by VADNS alone (17) and by the mel measure alone (34), across the first frame at which a countdown alone
    holds the VAD flag, across the three noise floors, and inside the stretches on the floors.  Everything equals the one
    launch bit for bit, the raised hang-over included: it shows in the emitted flags behind the cut."""
    names, utts, bounds = _edge_set()
    assert {16, 17, 34, 35, 1373, 1374} <= set(bounds) and bounds[-1] == len(utts[0]) // 160
    want = _one_launch(utts)
    got = _in_slices(len(utts), _cuts(utts, bounds))
    words = 0
    for j, name in enumerate(names):
        _assert_features_equal(got[j], want[j], f"edge signal {name}")
        words += sum(got[j][k].size for k in ("feat_cc", "feat_pp", "feats", "flags", "out", "f32", "hp", "code")) + 4
    short = want[names.index("short_onset_wb")]
    assert len(short["feats"]) and short["feats"][:, 14].all(), "short_onset_wb: the flush no longer keeps the VAD flag up"
    print(f"\n{len(bounds) - 1} slices, {words} words compared with the one launch, 0 differ")


def test_edge_set_through_the_host_pipeline():
    """The edge set four times over (32 utterances, enough bytes for sea_wb_features_utterances to cut the list) against
    wb_afe_features_batch: emitted rows bit for bit, the low band too."""
    import speech_enhancement_amd as sea
    names, utts, _ = _edge_set()
    lst = utts * 4
    want = _one_launch(lst)
    got = sea.wb_features_utterances(lst, want_lp=True)
    assert got["slices"] > 1, f"run as {got['slices']} launch(es)"
    words = 0
    for u, w in enumerate(want):
        what = f"edge signal {names[u % len(names)]} (copy {u // len(names)})"
        assert got["feats"][u].shape == w["feats"].shape, f"{what}: {len(got['feats'][u])} rows, one launch {len(w['feats'])}"
        assert np.array_equal(_u32(got["feats"][u]), _u32(w["feats"])), f"{what}: rows differ in bits from the one launch"
        assert np.array_equal(got["out"][u], w["out"]), f"{what}: low band"
        words += w["feats"].size + w["out"].size
    print(f"\n{len(lst)} utterances, {got['slices']} launches, {words} words compared with the one launch, 0 differ")
