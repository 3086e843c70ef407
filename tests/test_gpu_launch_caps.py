"""Every grid-stride kernel past its launch cap, bit for bit.

Most kernels outside the NoiseSup frame loop are launched with a capped grid and walk their work in a grid-stride loop (the
table in tests/launch_caps.py).  These tests call each entry point at a size where workgroups take a second and a third trip
of that loop; the sizes come from tests/launch_caps.py (the caps parsed from csrc/capi.hip) and the device's CU count, and
each test asserts that precondition before it runs and prints how many words it compared and how many trips the busiest
workgroup took.

Rules of the file: every comparison is on the bits (uint32 views; NaNs by position where they can occur); buffers handed to
the C calls start as sentinels and carry guard rows, so a trip that never ran shows up as sentinel rows; the oracle or the
reference runs once per DISTINCT input and the large inputs repeat a small distinct set whose size is a prime that does not
divide the grid (otherwise a workgroup's trips would all see the same content).  Run on an MI355X with ``pytest -m gpu``."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import launch_caps as LC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_F32, SENT_INT = -7777.25, -77
GUARD_ROWS = 3
N_DISTINCT = 61  # prime; 16384 % 61 = 36, 8192 % 61 = 18
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _n_cu():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _caps():
    return LC.parse()


@pytest.fixture(scope="module", autouse=True)
def _release_the_big_results():
    """the one-launch results are shared between the tests of this file and dropped after the last one"""
    yield
    for f in (_cc_one_launch, _afe_one_launch, _wb_one_launch, _wb_afe_one_launch, _wb_want, _batch_wb, _batch_8k):
        f.cache_clear()


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _is_sent(a):
    return bool((_u32(a) == np.float32(SENT_F32).view(np.uint32)).all())


def _report(what, words, t):
    print(f"\n{what}: {words} words compared bit for bit; grid {t.grid}, {t.work} work items, the busiest workgroup takes "
          f"{t.busiest} trips, {t.at_least_2} workgroups take >= 2 and {t.at_least_3} take >= 3")


def _report_slices(what, words, trips):
    print(f"\n{what}: {words} words compared bit for bit with the one launch")
    for k, t in enumerate(trips):
        print(f"  slice {k}: grid {t.grid}, {t.work} work items, the busiest workgroup takes {t.busiest} trips, "
              f"{t.at_least_2} workgroups take >= 2 and {t.at_least_3} take >= 3")


def _tile_on_device(distinct, n):
    """rows k % len(distinct) of `distinct`, k < n, built on the device (only the distinct rows are uploaded)"""
    torch = _torch()
    d = torch.from_numpy(np.ascontiguousarray(distinct)).to(DEV)
    return d[torch.arange(n, device=DEV) % len(distinct)].contiguous()


# ---------------------------------------------------------------- (a) sea_rfft256_batch ----
def test_a_rfft_batch_past_the_cap(oracle):
    """2 (2 * 16 n_cu) + 3 frames: an odd count (the last pair is half empty), every wave takes two trips of rfft256_kernel's
    prefetching loop and two take three.  The frames repeat test_rfft_bit_exact's 257 (zero, impulse and full-scale rows kept);
    expected: the oracle's rfft of the distinct frames."""
    import speech_enhancement_amd as sea
    torch = _torch()
    caps, n_cu = _caps(), _n_cu()
    rng = np.random.default_rng(1)
    frames = (rng.standard_normal((257, 256)) * rng.uniform(0.1, 3000.0, (257, 1))).astype(np.float32)
    frames[0] = 0.0
    frames[1, :] = 0.0
    frames[1, 3] = 1.0
    frames[2] = 32767.0
    want = np.stack([oracle.rfft(f) for f in frames])
    n = 2 * (2 * caps.rfft_per_cu * n_cu) + 3
    t = LC.rfft_trips(n, n_cu, caps)
    assert n % 2 == 1 and n >= LC.rfft_second_trip_frames(n_cu, caps)
    assert t.busiest >= 3 and t.at_least_2 == t.grid and t.at_least_3 >= 1, t
    assert t.grid % len(frames) != 0 and (2 * t.grid) % len(frames) != 0, "a wave's trips would all see the same frames"
    x = _tile_on_device(frames, n)
    out = torch.full((n + GUARD_ROWS, 256), SENT_F32, dtype=torch.float32, device=DEV)
    lib = sea.load()
    assert lib.sea_rfft256_batch(_p(x), _p(out), n, None) == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _is_sent(got[n:]), "guard rows behind the last frame were written"
    bad = (_u32(got[:n]) != _u32(want)[np.arange(n) % len(frames)]).any(axis=1)
    assert not bad.any(), (f"{int(bad.sum())} of {n} frames differ in bits from the oracle's rfft, first at {np.flatnonzero(bad)[:6]} "
                           f"(frames from {2 * t.grid} on are second trips)")
    assert torch.equal(x, _tile_on_device(frames, n)), "the input was modified"
    _report("(a) sea_rfft256_batch", n * 256, t)


# ---------------------------------------------------------------- (b) sea_compceps_frames ----
def test_b_compceps_frames_past_the_cap(oracle):
    """16 (8192 + 100) + 5 frames of 201 floats: 100 waves of compceps_frames_kernel take a second tile, the last tile holds
    five frames.  277 distinct frames as test_compceps_frames_amplitudes_and_ragged_tiles builds its own (the scales 1e-30 ..
    1e14 and a silent frame); expected: the oracle's compceps_frame of the distinct frames.  The 107 MB input is tiled on the
    device from the distinct rows."""
    import speech_enhancement_amd as sea
    torch = _torch()
    caps = _caps()
    rng = np.random.default_rng(77)
    base = rng.standard_normal((35, 201)).astype(np.float32)
    distinct = np.concatenate([base * np.float32(sc) for sc in (1e-30, 1e-12, 1e-6, 1e-3, 1.0, 1e4, 1e9, 1e14)])
    distinct[5] = 0.0  # a silent frame
    distinct = np.ascontiguousarray(distinct[:277])
    want = np.stack([oracle.compceps_frame(f) for f in distinct])
    assert np.isfinite(want).all()
    n = caps.frames_tile * (caps.frames_grid + 100) + 5
    t = LC.frames_trips(n, caps)
    assert n >= LC.frames_second_trip_frames(caps) and t.grid == caps.frames_grid and t.busiest >= 2 and t.at_least_2 >= 100, t
    assert (caps.frames_tile * t.grid) % len(distinct) != 0 and t.grid % len(distinct) != 0
    x = _tile_on_device(distinct, n)
    out = torch.full((n + GUARD_ROWS, 14), SENT_F32, dtype=torch.float32, device=DEV)
    lib = sea.load()
    assert lib.sea_compceps_frames(_p(x), _p(out), n, None) == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _is_sent(got[n:]), "guard rows behind the last frame were written"
    bad = (_u32(got[:n]) != _u32(want)[np.arange(n) % len(distinct)]).any(axis=1)
    assert not bad.any(), (f"{int(bad.sum())} of {n} frames differ in bits from the oracle, first at {np.flatnonzero(bad)[:6]} "
                           f"(frames from {caps.frames_tile * t.grid} on are second trips)")
    _report("(b) sea_compceps_frames", n * 14, t)


# ---------------------------------------------------------------- the 8 kHz batches of (c), (d), (e) ----
@functools.lru_cache(maxsize=None)
def _distinct_8k():
    """61 short utterances of 3 .. 40 frames with ragged tails (every fifth seed has 400 leading zeros: corpus.py), one empty, one
    all zero, one shorter than five frames (no output); three of about 2000 frames"""
    from speech_enhancement_amd import corpus
    rng = np.random.default_rng(61)
    nfr, tail = rng.integers(3, 41, N_DISTINCT), rng.integers(0, 80, N_DISTINCT)
    short = [corpus.synth_utterance(700 + k, 80 * int(n) + int(r)) for k, (n, r) in enumerate(zip(nfr, tail))]
    short[7] = np.zeros(0, np.int16)
    short[13] = np.zeros(80 * 20 + 5, np.int16)
    short[29] = short[29][:80 * 4 + 17]
    short[40] = corpus.synth_utterance(740, 80 * 40 + 79)  # the longest, whatever the draw
    short[41] = corpus.synth_utterance(741, 80 * 7)        # the first length with a cepstral frame, no tail
    long = [corpus.synth_utterance(900 + k, 80 * n + r) for k, (n, r) in enumerate(((2000, 0), (1987, 33), (2011, 79)))]
    return tuple(short), tuple(long)


def _place(nfr_short, nfr_long, tile, grid, hop_cap, n_min):
    """the batch as indices into short + long: the short ones in cycles, long[0] early, long[1] where its slots lie on both
    sides of slot index `grid`, long[2] near the end; as many utterances as give one workgroup a third tile"""
    ns = len(nfr_short)
    caps_all = np.maximum(np.array(list(nfr_short) + list(nfr_long), np.int64) - hop_cap, 0)
    cap_of = lambda ids: caps_all[np.asarray(ids)]  # noqa: E731
    n = n_min
    while True:
        ids = [k % ns for k in range(n)]
        ids.insert(5, ns)
        base = LC.slot_base(np.concatenate(([0], np.cumsum(cap_of(ids)))), tile)
        half = (nfr_long[1] - hop_cap) // tile // 2
        k = int(np.argmax(base >= grid - half))
        assert 5 < k < len(ids) - 7 and base[k] < grid
        ids.insert(k, ns + 1)
        ids.insert(len(ids) - 7, ns + 2)
        cum = np.concatenate(([0], np.cumsum(cap_of(ids))))
        t = LC.slot_trips(cum, tile, grid)
        if t.at_least_3 >= 1:
            return ids, cum, t, k
        n += ns


@functools.lru_cache(maxsize=None)
def _batch_8k(kind):
    """kind "cc": kCcGrid + 64 utterances or more for compceps_kernel's slots of 16; "afe": kAfeGrid + 64 or more for the feature
    chain's slots of 8.  Returns (utterances, ids into the distinct set, prefix sums of the capacities, Trips, the straddler)"""
    caps = _caps()
    short, long = _distinct_8k()
    tile, grid = (caps.cc_tile, caps.cc_grid) if kind == "cc" else (caps.afe_tile, caps.afe_grid)
    ids, cum, t, k = _place([len(x) // 80 for x in short], [len(x) // 80 for x in long], tile, grid, 6, grid + 64)
    both = short + long
    utts = [both[i] for i in ids]
    assert len(utts) >= grid + 64 and grid % N_DISTINCT != 0 and len(short) == N_DISTINCT
    assert t.grid == grid and t.at_least_2 >= grid // 2 and t.at_least_3 >= 1, t
    assert k in LC.straddles(cum, tile, grid), f"utterance {k} does not own slots on both sides of slot {grid}"
    return utts, ids, cum, t, k


@pytest.fixture(scope="module")
def oracle_8k(oracle):
    """the oracle on the distinct 8 kHz utterances, once: ns_trace (cepstra) and afe_trace (the feature chain)"""
    short, long = _distinct_8k()
    both = short + long
    ns = [oracle.ns_trace(x, want_state=False) for x in both]
    counts = [tr["nceps"] for tr in ns[:N_DISTINCT]]
    assert ns[7]["nceps"] == 0 and ns[13]["nceps"] == 0 and ns[29]["nceps"] == 0 and ns[41]["nceps"] == 1
    assert sum(c > 16 for c in counts) >= 10 and sum(0 < c < 16 for c in counts) >= 10, counts
    return dict(ns=ns, afe=[oracle.afe_trace(x) for x in both])


@functools.lru_cache(maxsize=None)
def _cc_one_launch(use_order):
    """ns_denoise_batch (want_f32) + sea_compceps_batch on the "cc" batch into sentinel-filled buffers with guard rows ->
    host arrays, computed once per launch order"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    utts, ids, cum, t, k = _batch_8k("cc")
    b = sea.PackedBatch.from_arrays(utts, device=DEV)
    out, f32, first = sea.ns_denoise_batch(b, want_f32=True, use_order=use_order)
    total = int(cum[-1])
    ceps = torch.full((total + GUARD_ROWS, 14), SENT_F32, dtype=torch.float32, device=DEV)
    n_ceps = torch.full((b.n_utt + GUARD_ROWS,), SENT_INT, dtype=torch.int32, device=DEV)
    d_cum = torch.from_numpy(np.asarray(cum, np.int64)).to(DEV)
    rc = lib.sea_compceps_batch(_p(f32), _p(b.offsets), _p(b.lengths), _p(first), _p(d_cum), total, _p(ceps), _p(n_ceps), b.n_utt, None)
    assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    return dict(ceps=ceps.cpu().numpy(), n_ceps=n_ceps.cpu().numpy(), first=first.cpu().numpy(),
                out=b.split(out, full_frames_only=True))


# ---------------------------------------------------------------- (c) sea_compceps_batch ----
@pytest.mark.parametrize("use_order", [True, False], ids=["launch_order", "plain_order"])
def test_c_compceps_batch_past_the_cap(oracle_8k, use_order):
    """kCcGrid + 64 utterances or more, so that the utterance count and not the audio reaches the cap of compceps_kernel: the
    61 distinct short ones in cycles, three of about 2000 frames of which one owns slots on both sides of slot kCcGrid.
    n_ceps, every cepstral row and the zeros behind the last row of each capacity against the oracle's ns_trace of the distinct
    utterances.  An utterance without capacity owns no tile: its count is not written (the Python layer zero-fills it)."""
    caps = _caps()
    utts, ids, cum, t, k = _batch_8k("cc")
    r = _cc_one_launch(use_order)
    n, total = len(utts), int(cum[-1])
    want = oracle_8k["ns"]
    assert _is_sent(r["ceps"][total:]) and (r["n_ceps"][n:] == SENT_INT).all(), "guard rows were written"
    cap = np.diff(cum)
    want_n = np.array([want[i]["nceps"] if c > 0 else SENT_INT for i, c in zip(ids, cap)], np.int64)
    assert all(want[i]["nceps"] <= c for i, c in zip(ids, cap))
    bad = np.flatnonzero(r["n_ceps"][:n] != want_n)
    assert bad.size == 0, f"n_ceps differs for {bad.size} utterances, first {bad[:6]}: {r['n_ceps'][bad[:6]]} vs {want_n[bad[:6]]}"
    pad = [np.concatenate([w["ceps"], np.zeros((max(len(x) // 80 - 6, 0) - w["nceps"], 14), np.float32)])
           for w, x in zip(want, _distinct_8k()[0] + _distinct_8k()[1])]
    expect = np.concatenate([pad[i] for i in ids])
    assert expect.shape == (total, 14)
    assert not (_u32(r["ceps"][:total]) == np.float32(SENT_F32).view(np.uint32)).all(axis=1).any(), "a row was left at the sentinel"
    badrow = np.flatnonzero((_u32(r["ceps"][:total]) != _u32(expect)).any(axis=1))
    owner = np.searchsorted(cum, badrow[:6], side="right") - 1
    assert badrow.size == 0, (f"{badrow.size} of {total} rows differ in bits from the oracle; first rows {badrow[:6]} of utterances "
                              f"{owner}, first slots {LC.slot_base(cum, caps.cc_tile)[owner]}")
    _report(f"(c) sea_compceps_batch, {n} utterances, utterance {k} across slot {caps.cc_grid}", total * 14 + n, t)


# ---------------------------------------------------------------- (d) the 8 kHz slice forms ----
def _slice_trips(slices, hop, tile, grid):
    res = []
    for s in slices:
        fr = np.array([len(x) // hop for x in s[1]], np.int64)
        res.append(LC.slot_trips(np.concatenate(([0], np.cumsum(fr))), tile, grid))
    return res


def _longest_first(utts, hop):
    """the utterances with a whole frame, longest first (stable): the list the slice helpers cut"""
    keep = [u for u in range(len(utts)) if len(utts[u]) >= hop]
    return sorted(keep, key=lambda u: -(len(utts[u]) // hop))


def test_d_compceps_batch_slices_past_the_cap(oracle_8k):
    """(c)'s batch through sea_ns_denoise_batch_slice + sea_compceps_batch_slice in three time slices cut at frames 9 and 1003
    (no multiple of 16; the second inside the long utterances): rows, counts and audio are byte-equal to (c)'s one launch,
    which (c) pins to the oracle.  The first two slices hold more than 16384 slots."""
    from tests import test_gpu_ceps_slices as CS
    caps = _caps()
    utts, ids, cum, _, _ = _batch_8k("cc")
    r = _cc_one_launch(True)
    order = _longest_first(utts, 80)
    slices = CS._cuts([utts[u] for u in order], (0, 9, 1003, 2100), 80)
    trips = _slice_trips(slices, 80, caps.cc_tile, caps.cc_slice_grid)
    assert len(slices) == 3 and all(t.grid == caps.cc_slice_grid and t.busiest >= 2 and t.at_least_2 >= 1000 for t in trips[:2]), trips
    got = CS._in_slices(len(order), slices, False)
    words = 0
    for j, u in enumerate(order):
        nc = max(int(r["n_ceps"][u]), 0)
        want = dict(ceps=r["ceps"][cum[u]:cum[u] + nc], n_ceps=nc, out=r["out"][u], first_out=int(r["first"][u]))
        CS._assert_equal(got[j], want, f"utterance {u}")
        words += 14 * nc
    _report_slices("(d) sea_compceps_batch_slice", words, trips)


# ---------------------------------------------------------------- (e) sea_afe_features_batch and its slice form ----
@functools.lru_cache(maxsize=None)
def _afe_one_launch():
    from tests import test_gpu_afe_slices as AS
    return AS._one_launch(_batch_8k("afe")[0])


def test_e_afe_features_batch_past_the_cap(oracle_8k):
    """kAfeGrid + 64 utterances or more from the same distinct set, a long one across slot kAfeGrid of afe_ceps_kernel's slots
    of 8: feat_cc, feat_pp, the emitted feats, the flag bytes and the counts against the oracle's afe_trace of the distinct
    utterances, bit for bit."""
    caps = _caps()
    utts, ids, cum, t, k = _batch_8k("afe")
    res = _afe_one_launch()
    want = oracle_8k["afe"]
    words = 0
    for u, (i, g) in enumerate(zip(ids, res)):
        w, nfr = want[i], len(utts[u]) // 80
        f0 = nfr - w["nout"] if w["nout"] else -1
        assert (g["n_ceps"], len(g["feats"]), g["first_out"]) == (w["nceps"], w["nvad"], f0), \
            f"utterance {u} (distinct {i}): counts / first output {(g['n_ceps'], len(g['feats']), g['first_out'])} vs {(w['nceps'], w['nvad'], f0)}"
        for name, a, b in (("feat_cc", g["feat_cc"], w["feat_cc"]), ("feat_pp", g["feat_pp"], w["feat_pp"]), ("feats", g["feats"], w["vad_out"])):
            assert a.shape == b.shape and np.array_equal(_u32(a), _u32(b)), \
                f"utterance {u} (distinct {i}): {name} differs in bits from the oracle in {int((_u32(a) != _u32(b)).sum())} of {a.size} words"
            words += a.size
        quiet = f0 if f0 >= 0 else nfr
        assert not g["flags"][:quiet].any() and np.array_equal(g["flags"][quiet:], w["flags"][quiet:nfr, :4] @ np.array([1, 2, 4, 8])), \
            f"utterance {u} (distinct {i}): flag bytes differ"
        words += nfr
    _report(f"(e) sea_afe_features_batch, {len(utts)} utterances, utterance {k} across slot {caps.afe_grid}", words, t)


def test_e_afe_features_batch_slices_past_the_cap():
    """(e)'s batch through sea_ns_denoise_batch_slice_fd + sea_afe_features_batch_slice in three slices cut at frames 9 and
    1003, the flush with each utterance's last slice: byte-equal to the one launch."""
    from tests import test_gpu_afe_slices as AS
    caps = _caps()
    utts = _batch_8k("afe")[0]
    want = _afe_one_launch()
    order = _longest_first(utts, 80)
    slices = AS._cuts([utts[u] for u in order], (0, 9, 1003, 2100))
    trips = _slice_trips(slices, 80, caps.afe_tile, caps.afe_grid)
    assert len(slices) == 3 and all(t.grid == caps.afe_grid and t.busiest >= 2 and t.at_least_2 >= 1000 for t in trips[:2]), trips
    got = AS._in_slices(len(order), slices)
    words = 0
    for j, u in enumerate(order):
        AS._assert_features_equal(got[j], want[u], f"utterance {u}")
        words += sum(want[u][key].size for key in ("feat_cc", "feat_pp", "feats"))
    _report_slices("(e) sea_afe_features_batch_slice", words, trips)


# ---------------------------------------------------------------- (f) the wideband mode ----
def _wb_reference():
    from tests import wb_afe_reference as A
    from tests import wb_reference as W
    if not W.available():
        pytest.fail("oracle/_ref/libetsi_ref.so is missing: `make -C oracle ref` builds it where the reference's sources "
                    "are; this test needs the built library beside the tree")
    return W, A


@functools.lru_cache(maxsize=None)
def _batch_wb():
    """16384 + 64 wideband utterances or more of 3 .. 40 frames of 160 samples from 61 distinct ones (synth_wideband and
    synth_utterance, ragged, zero-led, one all zero, one empty), plus the six long inputs of wb_golden.npz whose high-band VAD
    moves: one early, one across slot 16384 of the cepstrum's slots of 16, the others spread."""
    from speech_enhancement_amd import corpus
    caps = _caps()
    rng = np.random.default_rng(161)
    nfr, tail = rng.integers(3, 41, N_DISTINCT), rng.integers(0, 160, N_DISTINCT)
    short = []
    for k, (n, r) in enumerate(zip(nfr, tail)):
        L = 160 * int(n) + (int(r) if k % 3 else 0)
        x = corpus.synth_wideband(k, L) if k % 2 else corpus.synth_utterance(800 + k, L)
        if k % 7 == 3:
            x[:160 * (1 + k % 3) + 50] = 0  # zero-led
        short.append(x)
    short[11] = np.zeros(160 * 20 + 9, np.int16)
    short[17] = np.zeros(0, np.int16)
    short[40] = corpus.synth_wideband(40, 160 * 40 + 159)
    with np.load(os.path.join(GOLD, "wb_golden.npz")) as z:
        long = [z[f"x{u}"] for u in range(6)]
    assert caps.wb_cc_grid == caps.cc_slice_grid
    grid = caps.wb_cc_grid
    nshort = [len(x) // 160 for x in short]
    cap_of = lambda x: max(len(x) // 160 - 6, 0)  # noqa: E731
    n = grid + 64
    while True:
        utts = [short[k % N_DISTINCT] for k in range(n)]
        ids = [k % N_DISTINCT for k in range(n)]
        utts.insert(5, long[0])
        ids.insert(5, N_DISTINCT)
        pick = int(np.argmax([len(x) for x in long[1:]])) + 1
        base = LC.slot_base(np.concatenate(([0], np.cumsum([cap_of(x) for x in utts]))), caps.cc_tile)
        k = int(np.argmax(base >= grid - cap_of(long[pick]) // caps.cc_tile // 2))
        assert 5 < k and base[k] < grid
        utts.insert(k, long[pick])
        ids.insert(k, N_DISTINCT + pick)
        rest = [j for j in range(1, 6) if j != pick]
        for m, j in enumerate(rest):
            at = k + 1 + (m + 1) * (len(utts) - k - 8) // (len(rest) + 1)
            utts.insert(at, long[j])
            ids.insert(at, N_DISTINCT + j)
        cum = np.concatenate(([0], np.cumsum([cap_of(x) for x in utts]))).astype(np.int64)
        t = LC.slot_trips(cum, caps.cc_tile, grid)
        if t.at_least_3 >= 1:
            break
        n += N_DISTINCT
    assert len(utts) >= grid + 64 and grid % N_DISTINCT != 0 and caps.afe_grid % N_DISTINCT != 0 and min(nshort) == 0 and max(nshort) == 40
    assert k in LC.straddles(cum, caps.cc_tile, grid), f"utterance {k} does not own slots on both sides of slot {grid}"
    assert t.at_least_2 >= grid // 2, t
    return utts, ids, tuple(short) + tuple(long), cum, t, k


@functools.lru_cache(maxsize=None)
def _wb_want():
    """the reference on the distinct wideband inputs, once: (tests/wb_reference.py::trace, tests/wb_afe_reference.py::trace)"""
    W, A = _wb_reference()
    distinct = _batch_wb()[2]
    return [W.trace(x) for x in distinct], [A.trace(x) for x in distinct]


@functools.lru_cache(maxsize=None)
def _wb_one_launch():
    from tests import test_gpu_wb as WB
    return WB._run(_batch_wb()[0])


@functools.lru_cache(maxsize=None)
def _wb_afe_one_launch():
    from tests import test_gpu_wb_afe as WA
    return WA._run(_batch_wb()[0])


def _no_bits_differ(st):
    for key, (m, n, nb) in st.f.items():
        assert nb == 0, f"{key}: {nb} of {n} values differ in bits from the reference (max error {m:.3g})"
    return sum(n for _, n, _ in st.f.values())


def test_f_wb_compceps_batch_past_the_cap():
    """wb_denoise_batch + wb_compceps_batch on 16384 + 64 utterances or more (compceps_wb_kernel's cap, reached by the utterance
    count) against tests/wb_reference.py::trace of the distinct inputs: int16 low band, float stream, high-band rows, code and
    cepstra, all on the bits."""
    from tests import test_gpu_wb as WB
    caps = _caps()
    utts, ids, distinct, cum, t, k = _batch_wb()
    want = _wb_want()[0]
    res = _wb_one_launch()
    st = WB._Stats()
    for u, (i, g) in enumerate(zip(ids, res)):
        WB._compare(st, g, want[i], len(utts[u]) // 160, f"utterance {u} (distinct {i})")
    st.report("(f) wideband one launch")
    st.check()
    assert st.i16_diff == 0, f"{st.i16_diff} of {st.i16_n} int16 samples differ from the reference"
    words = _no_bits_differ(st) + st.i16_n
    _report(f"(f) sea_wb_compceps_batch, {len(utts)} utterances, utterance {k} across slot {caps.wb_cc_grid}", words, t)


def test_f_wb_afe_features_batch_past_the_cap():
    """wb_afe_features_batch on the same batch (afe_wb_ceps_kernel's slots of 8 against kAfeGrid) against
    tests/wb_afe_reference.py::trace of the distinct inputs: counts, flag bytes, VAD flags and null vectors exact, feat_cc,
    feat_pp and the emitted features on the bits."""
    from tests import test_gpu_wb_afe as WA
    caps = _caps()
    utts, ids, distinct, cum, _, _ = _batch_wb()
    want = _wb_want()[1]
    t = LC.slot_trips(cum, caps.afe_tile, caps.afe_grid)
    assert t.grid == caps.afe_grid and t.busiest >= 3 and t.at_least_2 >= caps.afe_grid // 2, t
    res = _wb_afe_one_launch()
    st = WA._Stats()
    for u, (i, g) in enumerate(zip(ids, res)):
        WA._compare(st, g, want[i], len(utts[u]) // 160, f"utterance {u} (distinct {i})")
    st.report("(f) wideband feature chain, one launch")
    st.check()
    words = _no_bits_differ(st) + sum(st.exact.values())
    _report(f"(f) sea_wb_afe_features_batch, {len(utts)} utterances", words, t)


def test_f_wb_compceps_batch_slices_past_the_cap():
    """the wideband batch through sea_wb_denoise_batch_slice + sea_wb_compceps_batch_slice in three slices cut at frames 9 and
    141 (the second inside the long inputs): byte-equal to the one launch."""
    from tests import test_gpu_ceps_slices as CS
    caps = _caps()
    utts = _batch_wb()[0]
    want = _wb_one_launch()
    order = _longest_first(utts, 160)
    slices = CS._cuts([utts[u] for u in order], (0, 9, 141, 100000), 160)
    trips = _slice_trips(slices, 160, caps.cc_tile, caps.cc_slice_grid)
    assert len(slices) == 3 and all(t.grid == caps.cc_slice_grid and t.busiest >= 2 and t.at_least_2 >= 1000 for t in trips[:2]), trips
    got = CS._in_slices(len(order), slices, True)
    words = 0
    for j, u in enumerate(order):
        CS._assert_equal(got[j], want[u], f"utterance {u}")
        words += want[u]["ceps"].size
    _report_slices("(f) sea_wb_compceps_batch_slice", words, trips)


def test_f_wb_afe_features_batch_slices_past_the_cap():
    """the wideband batch through sea_wb_denoise_batch_slice_fd + sea_wb_afe_features_batch_slice in three slices cut at
    frames 9 and 141, the flush with each utterance's last slice: byte-equal to the one launch."""
    from tests import test_gpu_wb_afe_slices as WS
    caps = _caps()
    utts = _batch_wb()[0]
    want = _wb_afe_one_launch()
    order = _longest_first(utts, 160)
    slices = WS._cuts([utts[u] for u in order], (0, 9, 141, 100000))
    trips = _slice_trips(slices, 160, caps.afe_tile, caps.afe_grid)
    assert len(slices) == 3 and all(t.grid == caps.afe_grid and t.busiest >= 2 and t.at_least_2 >= 1000 for t in trips[:2]), trips
    got = WS._in_slices(len(order), slices)
    words = 0
    for j, u in enumerate(order):
        WS._assert_features_equal(got[j], want[u], f"utterance {u}")
        words += sum(want[u][key].size for key in ("feat_cc", "feat_pp", "feats"))
    _report_slices("(f) sea_wb_afe_features_batch_slice", words, trips)


# ---------------------------------------------------------------- (g) hw25_correlogram_kernel ----
def _hw25_case(ids, real):
    """a batch for tests/test_gpu_hw25.py's _launch / _utterance: utterance u is input ids[u] of the seven where real[u], else
    eight zeros (no frame, no row)"""
    import speech_enhancement_amd as sea
    from tests import test_gpu_hw25 as H
    torch = _torch()
    seven, want7, tables = H.seven_inputs()
    zeros8 = np.zeros(8, np.float32)
    utts = [seven[i] if r else zeros8 for i, r in zip(ids, real)]
    batch = sea.PackedBatch.from_arrays(utts, device=DEV, dtype=np.float32)
    rows = np.array([len(x) // 80 for x in utts], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    perm = np.random.default_rng(len(utts)).permutation(len(utts)).astype(np.int32)
    return dict(utts=utts, want7=want7, batch=batch, rows=rows, offs=offs, d_offs=torch.from_numpy(offs).to(DEV),
                d_perm=torch.from_numpy(perm).to(DEV), tables=tables)


def _hw25_check(case, out, ids, real, names, what):
    from tests import hw25_model as M
    from tests import test_gpu_hw25 as H
    nrows, total = int(case["rows"].sum()), case["batch"].total
    for name in ("hout", "hev"):
        assert (out[name][total * H.NCH:] == H.SENT).all(), f"{what}: {name} guard"
    for name in ("acf_hc", "acf_ev", "cross_hc", "cross_ev", "pratio", "mark"):
        if out[name] is not None:
            assert (out[name][nrows:] == H.SENT).all(), f"{what}: {name} guard rows"
            left = np.flatnonzero((out[name][:nrows].reshape(nrows, -1) == H.SENT).any(axis=1))
            assert left.size == 0, f"{what}: {left.size} of {nrows} rows of {name} were left at the sentinel, first {left[:6]}"
    assert (out["pitch"][nrows:] == H.SENT_I).all(), f"{what}: pitch guard rows"
    left = np.flatnonzero(out["pitch"][:nrows] == H.SENT_I)
    assert left.size == 0, f"{what}: {left.size} of {nrows} pitch rows were left at the sentinel, first {left[:6]}"
    words = 0
    for u in np.flatnonzero(real):
        got, want = H._utterance(case, out, int(u)), case["want7"][ids[u]]
        for name in names:
            assert M.same_bits(np.ascontiguousarray(got[name]), want[name]), \
                f"{what}, utterance {u} (input {ids[u]}, rows from {int(case['offs'][u])}): {name}"
            words += want[name].size
        assert (got["pad_hOut"] == H.SENT).all() and (got["pad_hEv"] == H.SENT).all(), f"{what}: padding of utterance {u}"
    return words


@pytest.mark.parametrize("mode,order", [("group", False), ("two", True)], ids=["group_plain", "two_calls_permuted"])
def test_g_hw25_three_workgroups_per_utterance(mode, order):
    """Shape 1: as many utterances as give per_utt == 3 (683 with 256 CUs), cycling through the seven inputs of
    tests/test_gpu_hw25.py: the 15-frame utterances take five trips of the frame loop per workgroup, the 8-frame one three, the
    last partial -- LDS (win, acf modified in place by crossCorr, sumCorr, acf0, sPitch) reused from frame to frame.  With the
    ACF outputs, through the launch group in plain order and through the two calls in a permuted one."""
    from tests import test_gpu_hw25 as H
    caps, n_cu = _caps(), _n_cu()
    n = LC.hw25_utterances_for(3, n_cu, caps)
    ids = [u % 7 for u in range(n)]
    real = np.ones(n, bool)
    case = _hw25_case(ids, real)
    t = LC.hw25_trips(case["rows"], LC.hw25_per_utt(n, n_cu, caps))
    assert t.grid == 3 and t.busiest == 5 and t.at_least_3 >= 3 * (n // 7) * 3, t
    out = H._launch(case, mode, order, True)
    words = _hw25_check(case, out, ids, real, H.ARRAYS, f"per_utt 3, {mode}")
    _report(f"(g) hw25 correlogram, {n} utterances, 3 workgroups per utterance, {mode}", words, t)


def test_g_hw25_one_workgroup_per_utterance():
    """Shape 2: 8 n_cu + 1 utterances, so that per_utt == 1 and one workgroup walks all 15 frames of an utterance.  All are eight
    zeros (no frame; the chain is causal, so they give the first eight samples of input (d)'s hOut and the model's hEv) except
    41 real ones spread over the batch.  Null ACF pointers (proven equivalent in tests/test_gpu_hw25.py)."""
    from tests import hw25_model as M
    from tests import test_gpu_hw25 as H
    caps, n_cu = _caps(), _n_cu()
    n = caps.hw25_per_cu * n_cu + 1
    real = np.zeros(n, bool)
    where = (np.arange(41) * (n // 41) + 3) % n
    real[where] = True
    ids = np.zeros(n, np.int64)
    ids[where] = np.arange(41) % 7
    ids = ids.tolist()
    case = _hw25_case(ids, real)
    assert LC.hw25_per_utt(n, n_cu, caps) == 1 and real.sum() == 41
    t = LC.hw25_trips(case["rows"], 1)
    assert t.busiest == 15 and t.at_least_3 >= 20, t
    out = H._launch(case, "group", True, False)
    assert out["acf_hc"] is None and out["acf_ev"] is None
    frame_arrays = tuple(k for k in H.ARRAYS if not k.startswith("acf_"))
    words = _hw25_check(case, out, ids, real, frame_arrays, "per_utt 1")
    hout8 = np.ascontiguousarray(M.load_golden()["hOut_d"][:, :8])
    hev8 = M.lowpass(hout8, case["tables"]["lp"])
    off = np.asarray(case["batch"].host_offsets)[~real]
    idx = (off[:, None] * H.NCH + np.arange(H.NCH * 8)[None, :])
    assert M.same_bits(out["hout"][idx].reshape(-1, H.NCH, 8), np.broadcast_to(hout8, (len(off), H.NCH, 8)).copy()), "hOut of the zero utterances"
    assert M.same_bits(out["hev"][idx].reshape(-1, H.NCH, 8), np.broadcast_to(hev8, (len(off), H.NCH, 8)).copy()), "hEv of the zero utterances"
    words += 2 * idx.size
    _report(f"(g) hw25 correlogram, {n} utterances, one workgroup per utterance", words, t)
