"""GPU tests of the plain CompCeps in TIME SLICES at both rates (sea_compceps_batch_slice, sea_wb_compceps_batch_slice) and of the
host pipelines built on them (sea_denoise_ceps_utterances, sea_wb_denoise_ceps_utterances): an utterance cut along the time axis,
one launch group per slice -- the denoiser's slice call, then the cepstrum's -- with the cepstrum's own state carried per
utterance: three frames of the float stream and, in the wideband mode, two high-band and two code rows.

The criterion is exact: concatenated over an utterance's slices the rows are the BITS of the one launch (ns_denoise_batch +
compceps_batch, wb_denoise_batch + wb_compceps_batch: unchanged code, pinned to the oracle and to the reference's recorded
outputs elsewhere), floats compared as uint32, and the counts sum to its count.  So that both sides cannot be wrong together,
tests 1 and 2 also hold the sliced rows against the reference's recorded cepstra (tests/golden/ns_golden.npz `<name>/ceps`,
tests/golden/wb_golden.npz `ceps{i}`) within 1e-3, the limit of tests/test_gpu_golden.py and tests/test_gpu_wb.py, with equal
counts.  Outputs start as sentinels and states as NaN.  Run on an MI355X with ``pytest -m gpu``."""
import functools
import os

import numpy as np
import pytest

from tests.test_gpu_afe_slices import (EDGE_BOUNDS, FIXTURE, SENT_F32, SENT_FLAG, SENT_I16, SENT_INT, _is_sent, _p, _short_batch,
                                       _torch, _u32)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# every frame of the zero leads (5, 8) and of the four-frame latency, the first cepstral frames (first output + 2), the 16-frame
# tile's edge on both sides (the first tile of an utterance with first output 4 / 9 / 12 ends with output frame 21 / 26 / 29; the
# second slice's tiles start at row 0 again), then the ends of the utterances
BOUNDS = tuple(range(23)) + (31, 32, 33, 40, 41, 97, 98, 150, 400)
DEV = "cuda:0"
RATES = pytest.mark.parametrize("wb", [False, True], ids=["8k", "wb"])


def _hop(wb):
    return 160 if wb else 80


def _sorted(utts, hop):
    """longest first (stable), so that the utterances of a later slice are a prefix of the list"""
    ids = sorted(range(len(utts)), key=lambda u: -(len(utts[u]) // hop))
    return ids, [utts[u] for u in ids]


def _cuts(utts, bounds, hop):
    """[(frame_base, the active prefix's parts)]: the list (longest first) cut at `bounds` (frames of `hop`); an utterance's last
    slice carries its ragged tail"""
    nfr = [len(x) // hop for x in utts]
    assert nfr == sorted(nfr, reverse=True) and bounds[0] == 0 and bounds[-1] >= nfr[0]
    slices = []
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        act = [u for u in range(len(utts)) if nfr[u] > b0]
        assert act == list(range(len(act)))
        if not act:
            break
        slices.append((b0, [utts[u][hop * b0:hop * b1] if b1 < nfr[u] else utts[u][hop * b0:] for u in act]))
    return slices


def _one_launch(utts, wb):
    """the yardstick: one denoiser launch + one cepstrum launch on the list -> per utterance dict(ceps, n_ceps, out, first_out);
    out holds the whole frames only (80 samples per frame at either rate)"""
    import speech_enhancement_amd as sea
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device=DEV)
    if wb:
        r = sea.wb_denoise_batch(b, want_f32=True, want_hb=True)
        ceps, cum, n_ceps = sea.wb_compceps_batch(b, r)
        torch.cuda.synchronize()
        out, first = sea.wb_split(b, r["out"]), r["first_out"].cpu().numpy()
    else:
        out_t, f32, first = sea.ns_denoise_batch(b, want_f32=True)
        ceps, cum, n_ceps = sea.compceps_batch(b, f32, first)
        torch.cuda.synchronize()
        out, first = b.split(out_t, full_frames_only=True), first.cpu().numpy()
    ceps, n_ceps = ceps.cpu().numpy(), n_ceps.cpu().numpy()
    return [dict(ceps=ceps[cum[u]:cum[u] + int(n_ceps[u])], n_ceps=int(n_ceps[u]), out=out[u], first_out=int(first[u]))
            for u in range(len(utts))]


@functools.lru_cache(maxsize=None)
def _fixtures(wb):
    """the golden utterances, longest first, through the one launch: computed once per rate, nothing modifies it.  Returns
    (names, utterances, one-launch results, the reference's recorded cepstra)"""
    if wb:
        with np.load(os.path.join(GOLD, "wb_golden.npz")) as z:
            n = len([k for k in z.files if k.startswith("x")])
            ids, utts = _sorted([z[f"x{i}"] for i in range(n)], 160)
            ref = [z[f"ceps{i}"] for i in ids]
        names = [f"x{i}" for i in ids]
    else:
        with np.load(os.path.join(GOLD, "ns_golden.npz")) as z:
            names = [name for name, *_ in FIXTURE]
            utts = [z[f"{name}/in"] for name in names]
            ref = [z[f"{name}/ceps"] for name in names]
        assert _sorted(utts, 80)[0] == list(range(len(utts)))
    return names, utts, _one_launch(utts, wb), ref


def _in_slices(n_utt, slices, wb, fd=False):
    """One launch group per slice into sentinel-filled buffers: the denoiser's slice call (fd: its _fd form), then the cepstrum's
    with a capacity of the slice's frames per utterance.  Both states start as NaN: resume = 0 must not read them.  Returns per
    utterance the concatenated rows and audio and the summed counts."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    hop = _hop(wb)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)  # noqa: E731
    state = full((n_utt, int(lib.sea_wb_slice_state_floats() if wb else lib.sea_ns_slice_state_floats())), float("nan"), torch.float32)
    ccst = full((n_utt, int(lib.sea_wb_cc_slice_state_floats() if wb else lib.sea_cc_slice_state_floats())), float("nan"), torch.float32)
    first, onset = full((n_utt,), SENT_INT, torch.int32), full((n_utt,), SENT_INT, torch.int32)
    got = [dict(ceps=[], out=[]) for _ in range(n_utt)]
    n_ceps = np.zeros(n_utt, np.int64)
    for k, (b0, parts) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        n, resume = b.n_utt, 1 if k > 0 else 0
        fr = np.array([len(x) // hop for x in parts], np.int64)
        cum = np.concatenate(([0], np.cumsum(fr))).astype(np.int64)
        total = int(cum[-1])
        ceps = full((max(total, 1), 14), SENT_F32, torch.float32)
        nc = full((n,), SENT_INT, torch.int32)
        d_cum = torch.from_numpy(cum).to(DEV)
        if wb:
            half, rows = (b.total // 2 + 7) // 8 * 8, int(lib.sea_wb_rows(b.total))
            out, f32 = full((half,), SENT_I16, torch.int16), full((half,), SENT_F32, torch.float32)
            hp, code = full((rows, 3), SENT_F32, torch.float32), full((rows, 9), SENT_F32, torch.float32)
            scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(b.total, n)) // 4 + 4, dtype=torch.float32, device=DEV)
            if fd:
                flags = full((rows,), SENT_FLAG, torch.uint8)
                rc = lib.sea_wb_denoise_batch_slice_fd(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                                       _p(first), _p(onset), _p(flags), _p(hp), _p(code), _p(scratch), b.total,
                                                       _p(state), n, b0, resume, None)
            else:
                rc = lib.sea_wb_denoise_batch_slice(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                                    _p(first), _p(onset), _p(hp), _p(code), _p(scratch), b.total, _p(state), n, b0,
                                                    resume, None)
            assert rc == 0, lib.sea_last_error()
            rc = lib.sea_wb_compceps_batch_slice(_p(f32), _p(b.offsets), _p(b.lengths), _p(first), _p(hp), _p(code), _p(d_cum), total,
                                                 _p(ceps), _p(nc), _p(ccst), n, b0, resume, None)
            assert rc == 0, lib.sea_last_error()
            torch.cuda.synchronize()
            po = sea.wb_split(b, out)
        else:
            out, f32 = torch.full_like(b.data, SENT_I16), full((b.data.numel(),), SENT_F32, torch.float32)
            if fd:
                flags = full((max(b.total // 8, 1),), SENT_FLAG, torch.uint8)
                rc = lib.sea_ns_denoise_batch_slice_fd(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                                       _p(first), _p(flags), _p(onset), _p(state), n, b0, resume, None)
            else:
                rc = lib.sea_ns_denoise_batch_slice(_p(b.data), _p(out), _p(f32), _p(b.offsets), _p(b.lengths), _p(b.order), _p(first),
                                                    _p(state), n, b0, resume, None)
            assert rc == 0, lib.sea_last_error()
            rc = lib.sea_compceps_batch_slice(_p(f32), _p(b.offsets), _p(b.lengths), _p(first), _p(d_cum), total, _p(ceps), _p(nc),
                                              _p(ccst), n, b0, resume, None)
            assert rc == 0, lib.sea_last_error()
            torch.cuda.synchronize()
            po = b.split(out, full_frames_only=True)
        hc, hn = ceps.cpu().numpy(), nc.cpu().numpy()
        for u in range(n):
            a = int(hn[u])
            assert 0 <= a <= fr[u], f"slice {k}, utterance {u}: count {a} of {fr[u]} frames"
            rows_u = hc[cum[u]:cum[u] + a]
            assert not (_u32(rows_u) == np.float32(SENT_F32).view(np.uint32)).any(), f"slice {k}, utterance {u}: a counted row was not written"
            assert _is_sent(hc[cum[u] + a:cum[u + 1]]), f"slice {k}, utterance {u}: rows behind the slice's count were written"
            got[u]["ceps"].append(rows_u)
            got[u]["out"].append(po[u])
            n_ceps[u] += a
        if total == 0:
            assert _is_sent(hc), f"slice {k}: no whole frame, but a row was written"
    first = first.cpu().numpy()
    return [dict(ceps=np.concatenate(g["ceps"]).reshape(-1, 14), out=np.concatenate(g["out"]), n_ceps=int(n_ceps[u]),
                 first_out=int(first[u])) for u, g in enumerate(got)]


def _assert_equal(got, want, what):
    assert got["first_out"] == want["first_out"], f"{what}: first_out {got['first_out']}, one launch {want['first_out']}"
    assert got["n_ceps"] == want["n_ceps"] == len(got["ceps"]), f"{what}: {got['n_ceps']} cepstral frames, one launch {want['n_ceps']}"
    bad = (_u32(got["ceps"]) != _u32(want["ceps"])).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} rows differ in bits from the one launch, first at {np.flatnonzero(bad)[:4]}"
    assert np.array_equal(got["out"], want["out"]), f"{what}: int16 audio differs from the one launch"


@RATES
def test_fixtures_in_slices(wb):
    """Tests 1 and 2: the golden utterances of the rate, longest first, cut at BOUNDS (frames of 80 / of 160).  Rows, counts and
    audio are the one launch's bits, rows behind each slice's count stay sentinels, the _fd slice call as the producer gives the
    same bits, and the sliced rows are within 1e-3 of the reference's recorded cepstra with equal counts."""
    names, utts, want, ref = _fixtures(wb)
    hop = _hop(wb)
    slices = _cuts(utts, BOUNDS, hop)
    got = _in_slices(len(utts), slices, wb)
    got_fd = _in_slices(len(utts), slices, wb, fd=True)
    worst = 0.0
    for j, name in enumerate(names):
        _assert_equal(got[j], want[j], name)
        _assert_equal(got_fd[j], want[j], f"{name} behind the _fd slice call")
        assert got[j]["n_ceps"] == len(ref[j]), f"{name}: {got[j]['n_ceps']} cepstral frames, the reference recorded {len(ref[j])}"
        d = float(np.abs(got[j]["ceps"] - ref[j]).max()) if len(ref[j]) else 0.0
        worst = max(worst, d)
        assert d <= 1e-3, f"{name}: off the reference's recorded cepstra by {d}"
    assert sum(g["n_ceps"] for g in got) > 0
    print(f"\n{len(slices)} slices: the one launch's bits; worst |delta| to the reference's recorded cepstra {worst}")


def _single_frames(x, wb):
    """One utterance alone, one launch group per frame (and one for a ragged tail), pointers advanced frame by frame into
    buffers of the whole utterance; per-slice blocks of one cepstral row.  One read-back at the end."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    hop = _hop(wb)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)  # noqa: E731
    nfr, tail = len(x) // hop, len(x) % hop
    ns = nfr + (1 if tail else 0)
    xin = np.zeros(hop * (nfr + 1), np.int16)
    xin[:len(x)] = x
    d_in = torch.from_numpy(xin).to(DEV)
    out, f32 = full((80 * (nfr + 1),), SENT_I16, torch.int16), full((80 * (nfr + 1),), SENT_F32, torch.float32)
    hp, code = full((nfr + 2, 3), SENT_F32, torch.float32), full((nfr + 2, 9), SENT_F32, torch.float32)
    first, onset = full((1,), SENT_INT, torch.int32), full((1,), SENT_INT, torch.int32)
    meta = torch.tensor([0, hop, 0, 1], dtype=torch.int64, device=DEV)      # offsets | lengths | ceps_cum
    meta_t = torch.tensor([0, tail, 0, 0], dtype=torch.int64, device=DEV)   # the tail: no whole frame
    state = full((1, int(lib.sea_wb_slice_state_floats() if wb else lib.sea_ns_slice_state_floats())), float("nan"), torch.float32)
    ccst = full((1, int(lib.sea_wb_cc_slice_state_floats() if wb else lib.sea_cc_slice_state_floats())), float("nan"), torch.float32)
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(160, 1)) // 4 + 4, dtype=torch.float32, device=DEV)
    ceps, nc = full((ns, 14), SENT_F32, torch.float32), full((ns,), SENT_INT, torch.int32)
    before_tail = None
    for f in range(ns):
        is_tail = f == nfr
        m = meta_t if is_tail else meta
        resume = 1 if f > 0 else 0
        if is_tail:
            before_tail = ccst.clone()
        if wb:
            total = (tail + 7) // 8 * 8 if is_tail else 160
            rc = lib.sea_wb_denoise_batch_slice(_p(d_in, 320 * f), _p(out, 160 * f), _p(f32, 320 * f), _p(m), _p(m, 8), None, _p(first),
                                                _p(onset), _p(hp, 12 * f), _p(code, 36 * f), _p(scratch), total, _p(state), 1, f,
                                                resume, None)
            assert rc == 0, lib.sea_last_error()
            rc = lib.sea_wb_compceps_batch_slice(_p(f32, 320 * f), _p(m), _p(m, 8), _p(first), _p(hp, 12 * f), _p(code, 36 * f),
                                                 _p(m, 16), 0 if is_tail else 1, _p(ceps, 56 * f), _p(nc, 4 * f), _p(ccst), 1, f,
                                                 resume, None)
        else:
            rc = lib.sea_ns_denoise_batch_slice(_p(d_in, 160 * f), _p(out, 160 * f), _p(f32, 320 * f), _p(m), _p(m, 8), None, _p(first),
                                                _p(state), 1, f, resume, None)
            assert rc == 0, lib.sea_last_error()
            rc = lib.sea_compceps_batch_slice(_p(f32, 320 * f), _p(m), _p(m, 8), _p(first), _p(m, 16), 0 if is_tail else 1,
                                              _p(ceps, 56 * f), _p(nc, 4 * f), _p(ccst), 1, f, resume, None)
        assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    hc, hn = ceps.cpu().numpy(), nc.cpu().numpy()
    assert ((hn == 0) | (hn == 1)).all(), f"a slice's count is neither 0 nor 1: {hn}"
    for f in range(ns):
        assert _is_sent(hc[f][None][hn[f]:]), f"slice {f}: a row behind the count was written"
    if tail:
        assert hn[-1] == 0, "the tail's slice holds no whole frame and must report 0"
        assert np.array_equal(before_tail.cpu().numpy().view(np.uint32), ccst.cpu().numpy().view(np.uint32)), \
            "the tail's slice changed the state"
    return dict(ceps=hc[hn == 1], n_ceps=int(hn.sum()), out=out.cpu().numpy()[:80 * nfr], first_out=int(first.cpu()[0]))


@pytest.mark.parametrize("wb,name", [(False, "gap"), (False, "ragged"), (True, "x5"), (True, "x4")])
def test_single_frame_slices(wb, name):
    """Test 3: `gap` alone in 98 launch groups, `ragged` alone in 50 plus one for its 37-sample tail, the shortest wideband golden
    utterance (x5: four frames, no output) and the ragged one (x4: 303 frames + 77 samples) frame by frame: every history shift
    and every position of a row in the carried pair is a cut.  Every count is 0 or 1, the tail's slice reports 0 and leaves the
    state as it found it, and the rows are the one launch's bits (an utterance alone is its rows of the batch: the kernels know
    no neighbour)."""
    names, utts, want, _ = _fixtures(wb)
    j = names.index(name)
    if name == "x5":
        assert len(utts[j]) == min(len(x) for x in utts)
    got = _single_frames(utts[j], wb)
    _assert_equal(got, want[j], f"{name} in single-frame slices")


def test_short_utterances_cut_at_every_frame():
    """Test 4: 4, 5, 6, 7, 8, 13, 14, 15 frames, 15 frames + 37 samples, 40 frames behind 3 and behind 5 zero frames, 20 zero frames,
    cut at EVERY frame: the one launch's bits, and utterances that never produce an output give zero rows in every slice."""
    utts = _short_batch()
    assert [len(x) // 80 for x in utts] == [4, 5, 6, 7, 8, 13, 14, 15, 15, 43, 45, 20] and len(utts[8]) % 80 == 37
    ids, utts = _sorted(utts, 80)
    want = _one_launch(utts, False)
    got = _in_slices(len(utts), _cuts(utts, tuple(range(46)), 80), False)
    for j, u in enumerate(ids):
        _assert_equal(got[j], want[j], f"short utterance {u} ({len(utts[j])} samples)")
    never = [j for j in range(len(utts)) if want[j]["first_out"] < 0]
    assert never and all(got[j]["n_ceps"] == 0 for j in never)
    assert any(w["n_ceps"] > 0 for w in want) and any(w["first_out"] >= 0 and w["n_ceps"] == 0 for w in want)


def test_edge_signals_in_slices():
    """Test 5: the 14 signals of tests/ns_edge_cases.signals_8k(), longest first, cut at tests/test_gpu_afe_slices.py's
    EDGE_BOUNDS: the one launch's bits."""
    from tests import ns_edge_cases
    sig = ns_edge_cases.signals_8k()
    names = list(sig)
    ids, utts = _sorted([sig[n] for n in names], 80)
    assert len(utts[0]) // 80 == EDGE_BOUNDS[-1]
    want = _one_launch(utts, False)
    got = _in_slices(len(utts), _cuts(utts, EDGE_BOUNDS, 80), False)
    for j, u in enumerate(ids):
        _assert_equal(got[j], want[j], f"edge signal {names[u]}")


@RATES
def test_engine_wrappers_in_two_slices(wb):
    """Test 6: six utterances cut at frame 41 through the ENGINE wrappers, first_out handed from slice to slice: six utterances
    in the first slice, five in the second.  Rows, counts and audio are the one launch's bits, so an argument out of place in
    either wrapper's call shows."""
    import speech_enhancement_amd as sea
    torch = _torch()
    _, fixtures, _, _ = _fixtures(wb)
    hop = _hop(wb)
    if wb:
        utts = list(fixtures)
    else:  # every 8 kHz fixture outlasts frame 41: the sixth is `ragged` cut to 30 frames + its 37-sample tail
        utts = list(fixtures[:5]) + [np.concatenate([fixtures[5][:80 * 30], fixtures[5][80 * 50:]])]
        assert len(utts[5]) == 80 * 30 + 37
    want = _one_launch(utts, wb)
    slices = _cuts(utts, (0, 41, 400), hop)
    assert [len(parts) for _, parts in slices] == [6, 5]
    n_utt = len(utts)
    if wb:
        state, ccst = sea.wb_slice_state(n_utt, DEV), sea.wb_cc_slice_state(n_utt, DEV)
    else:
        state, ccst = sea.ns_slice_state(n_utt, DEV), sea.cc_slice_state(n_utt, DEV)
    first = onset = None
    got = [dict(ceps=[], out=[]) for _ in range(n_utt)]
    for k, (b0, parts) in enumerate(slices):
        b = sea.PackedBatch.from_arrays(parts, device=DEV)
        if wb:
            den = sea.wb_denoise_batch_slice(b, state, b0, k > 0, want_f32=True, want_hb=True, first_out=first, onset=onset)
            r = sea.wb_compceps_batch_slice(b, den, ccst, b0, k > 0)
            po = sea.wb_split(b, den["out"])
        else:
            den = sea.ns_denoise_batch_slice(b, state, b0, k > 0, want_f32=True, first_out=first)
            r = sea.compceps_batch_slice(b, den, ccst, b0, k > 0)
            po = b.split(den["out"], full_frames_only=True)
        torch.cuda.synchronize()
        first, onset = den["first_out"], den["onset"]
        for u in range(b.n_utt):
            assert len(r["ceps"][u]) == int(r["n_ceps"][u]) <= len(parts[u]) // hop
            got[u]["ceps"].append(r["ceps"][u])
            got[u]["out"].append(po[u])
    first = first.cpu().numpy()
    for j in range(n_utt):
        g = dict(ceps=np.concatenate(got[j]["ceps"]).reshape(-1, 14), out=np.concatenate(got[j]["out"]), first_out=int(first[j]))
        g["n_ceps"] = len(g["ceps"])
        _assert_equal(g, want[j], f"utterance {j} through the wrappers")
    assert sum(w["n_ceps"] for w in want) > 0


@RATES
def test_slice_arguments_are_checked(wb):
    """Test 7: NULL state, float stream, first_out, rows (wideband), prefix sums, ceps, n_ceps, offsets, lengths; negative
    frame_base and total_frames: non-zero, the call's name in the message, sentinels intact.  The same call with valid arguments
    runs: four frames without an output give a count of 0 and no row."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    hop = _hop(wb)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)  # noqa: E731
    b = sea.PackedBatch.from_arrays([np.zeros(4 * hop, np.int16)], device=DEV)
    T = dict(f32=full((b.total,), 0.0, torch.float32), first=full((1,), -1, torch.int32), hp=full((6, 3), 0.0, torch.float32),
             code=full((6, 9), 0.0, torch.float32), cum=torch.tensor([0, 4], dtype=torch.int64, device=DEV),
             ceps=full((4, 14), SENT_F32, torch.float32), nc=full((1,), SENT_INT, torch.int32), offs=b.offsets, lens=b.lengths,
             state=full((1, int(lib.sea_wb_cc_slice_state_floats() if wb else lib.sea_cc_slice_state_floats())), SENT_F32, torch.float32))
    name = "sea_wb_compceps_batch_slice" if wb else "sea_compceps_batch_slice"

    def call(frame_base=0, total=4, **kw):
        t = dict(T, **kw)
        if wb:
            return lib.sea_wb_compceps_batch_slice(_p(t["f32"]), _p(t["offs"]), _p(t["lens"]), _p(t["first"]), _p(t["hp"]), _p(t["code"]),
                                                   _p(t["cum"]), total, _p(t["ceps"]), _p(t["nc"]), _p(t["state"]), 1, frame_base, 0, None)
        return lib.sea_compceps_batch_slice(_p(t["f32"]), _p(t["offs"]), _p(t["lens"]), _p(t["first"]), _p(t["cum"]), total,
                                            _p(t["ceps"]), _p(t["nc"]), _p(t["state"]), 1, frame_base, 0, None)

    cases = [dict(state=None), dict(f32=None), dict(first=None), dict(cum=None), dict(ceps=None), dict(nc=None), dict(offs=None),
             dict(lens=None), dict(frame_base=-1), dict(total=-1)] + ([dict(hp=None), dict(code=None)] if wb else [])
    for kw in cases:
        rc = call(**kw)
        msg = lib.sea_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":"), f"{name}, {kw}: rc {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert _is_sent(T["ceps"].cpu().numpy()) and int(T["nc"].cpu()[0]) == SENT_INT and _is_sent(T["state"].cpu().numpy()), \
        "a refused call launched something"
    assert call() == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    assert int(T["nc"].cpu()[0]) == 0 and _is_sent(T["ceps"].cpu().numpy())
    assert not T["state"].cpu().numpy().any(), "resume = 0 and four frames of a zero stream: the history is zeros"


@RATES
def test_host_pipeline_equals_one_launch(wb):
    """Test 8: denoise_ceps_utterances / wb_denoise_ceps_utterances on (i) the golden utterances plus 31 short synthetic ones of
    0 .. 40 frames, some ragged, one empty, one all-zero -- one slice --, (ii) ONE utterance of 120 s, (iii) twelve utterances of
    2000 .. 0 frames, some ragged.  (ii) and (iii) must be cut into several launches.  Rows, counts and audio are the one launch's
    bit for bit, a list run twice gives the same bits, SEA_HOST_SLICES=3 gives the bits of the default, and the trailing partial
    frame of the 8 kHz `out` is not written."""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    hop = _hop(wb)
    run = (lambda lst: sea.wb_denoise_ceps_utterances(lst, want_lp=True)) if wb else (lambda lst: sea.denoise_ceps_utterances(lst))
    _, fixtures, _, _ = _fixtures(wb)
    utts = list(fixtures)
    for i in range(29):
        n = 1 + (i * 11) % 40
        utts.append(corpus.synth_utterance(60 + i, hop * n + (0 if i % 3 else 17 + i)))
    utts += [np.zeros(0, np.int16), np.zeros(hop * 9 + 5, np.int16)]
    assert len(utts) == 37 and sum(len(x) % hop != 0 for x in utts) >= 10
    long_one = np.tile(corpus.synth_utterance(3, 32000), 30 * hop // 80)
    assert len(long_one) == 100 * hop * 120
    ragged = [corpus.synth_utterance(100 + i, hop * n + (0 if i % 3 else 17 + i))
              for i, n in enumerate((2000, 1500, 1200, 900, 700, 500, 300, 200, 100, 40, 9, 0))]
    saved = {k: os.environ.pop(k, None) for k in ("SEA_HOST_SLICES", "SEA_HOST_CEPS_PIPELINE")}
    try:
        for name, lst, cut in (("short list", utts, False), ("one long utterance", [long_one], True),
                               ("cut and ragged list", ragged, True)):
            want = _one_launch(lst, wb)
            got, again = run(lst), run(lst)
            os.environ["SEA_HOST_SLICES"] = "3"
            three = run(lst)
            del os.environ["SEA_HOST_SLICES"]
            if cut:
                assert got["slices"] > 1 and again["slices"] > 1, f"{name}: run as {got['slices']} launch(es)"
                assert 1 < three["slices"] <= 3, f"{name}: SEA_HOST_SLICES=3 ran as {three['slices']} launch(es)"
            else:
                assert got["slices"] == three["slices"] == 1, f"{name}: a small list is one slice"
            for u, w in enumerate(want):
                what = f"{name}, utterance {u} ({len(lst[u])} samples)"
                for r in (got, again, three):
                    assert int(r["n_ceps"][u]) == w["n_ceps"] == len(r["ceps"][u]), f"{what}: {int(r['n_ceps'][u])} rows, one launch {w['n_ceps']}"
                    assert np.array_equal(_u32(r["ceps"][u]), _u32(w["ceps"])), f"{what}: rows differ in bits from the one launch"
                    whole = len(lst[u]) // hop * 80
                    assert np.array_equal(r["out"][u][:whole], w["out"]), f"{what}: audio differs from the one launch"
                    assert not r["out"][u][whole:].any(), f"{what}: the trailing partial frame was written"
            print(f"\n{name}: {len(lst)} utterance(s), {got['slices']} launch(es), {sum(w['n_ceps'] for w in want)} rows equal to the one launch bit for bit")
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def _wb_edge_set():
    """the wideband edge set (tests/ns_edge_cases.signals_wb()), longest first, and the bounds tests/wb_edge_cuts.py derives
    from the reference: -> (names, utterances, bounds)"""
    from tests import ns_edge_cases
    from tests import wb_edge_cuts
    from tests.test_gpu_wb import _reference
    _reference()                         # the cuts come from the reference run live: a missing library is a failure
    sig = ns_edge_cases.signals_wb()
    names = list(sig)
    ids, utts = _sorted([sig[k] for k in names], 160)
    return [names[u] for u in ids], utts, wb_edge_cuts.bounds()


def test_wb_edge_signals_in_slices():
    """The eight signals of the wideband edge set, longest first, cut at tests/wb_edge_cuts.bounds(): one-frame slices across
    the frames at which the reference first reaches the three noise floors (the high band's and code rows carried in the
    cepstrum's state are then the floored ones), inside the first thirteen frames and inside the stretches on the floors.
    Rows, counts and audio are the one launch's bits, behind the plain and behind the _fd slice call."""
    names, utts, bounds = _wb_edge_set()
    want = _one_launch(utts, True)
    slices = _cuts(utts, bounds, 160)
    got, got_fd = _in_slices(len(utts), slices, True), _in_slices(len(utts), slices, True, fd=True)
    words = 0
    for j, name in enumerate(names):
        _assert_equal(got[j], want[j], f"edge signal {name}")
        _assert_equal(got_fd[j], want[j], f"edge signal {name} behind the _fd slice call")
        words += 2 * (got[j]["ceps"].size + got[j]["out"].size + 2)
    assert want[names.index("ones_then_zeros_wb")]["n_ceps"] > 1510
    print(f"\n{len(slices)} slices, {words} words compared with the one launch, 0 differ")


def test_wb_edge_signals_through_the_host_pipeline():
    """The edge set four times over (32 utterances, enough bytes for sea_wb_denoise_ceps_utterances to cut the list) against
    wb_denoise_batch + wb_compceps_batch: rows, counts and audio bit for bit."""
    import speech_enhancement_amd as sea
    names, utts, _ = _wb_edge_set()
    lst = utts * 4
    want = _one_launch(lst, True)
    got = sea.wb_denoise_ceps_utterances(lst, want_lp=True)
    assert got["slices"] > 1, f"run as {got['slices']} launch(es)"
    words = 0
    for u, w in enumerate(want):
        what = f"edge signal {names[u % len(names)]} (copy {u // len(names)})"
        assert int(got["n_ceps"][u]) == w["n_ceps"] == len(got["ceps"][u]), f"{what}: {int(got['n_ceps'][u])} rows, one launch {w['n_ceps']}"
        assert np.array_equal(_u32(got["ceps"][u]), _u32(w["ceps"])), f"{what}: rows differ in bits from the one launch"
        assert np.array_equal(got["out"][u][:len(w["out"])], w["out"]), f"{what}: audio differs from the one launch"
        words += w["ceps"].size + w["out"].size + 1
    print(f"\n{len(lst)} utterances, {got['slices']} launches, {words} words compared with the one launch, 0 differ")
