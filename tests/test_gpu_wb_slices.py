"""GPU tests of the wideband (16 kHz) mode in TIME SLICES (sea_wb_denoise_batch_slice, sea_wb_denoise_utterances): an
utterance cut along the time axis and run as one launch per slice, with everything it needs carried in a per-utterance
state -- the QMF delay line, the onset, the frame loop's recursion, five frames of both QMF streams for the high band's
windows, the spectral subtraction's tracker.

The criterion is exact: the slices of an utterance give the BITS of the one launch (sea_wb_denoise_batch, which these
tests do not touch), floats compared as uint32.  So that the comparison cannot pass by both sides being wrong together,
test 1 also holds the sliced result against the reference's recorded outputs (tests/golden/wb_golden.npz) with the project's
tolerances, the checks of tests/test_gpu_wb.py::_compare restated here: int16 max |delta| <= 2 LSB and >= 99.9 % exact,
zero tolerance on which samples are zero and on every index, floats |delta| <= 1e-4 max(1, |ref|).

Inputs are the fixture's six utterances (frames of 160 / onset / first output: 100 / 0 / 4, 100 / 2 / 6, 300 / 0 / 4,
300 / 0 / 4, 303 + a ragged tail of 77 samples / 3 / 7, 4 / 0 / none); 2, 3 and 4 are the ones whose high-band VAD visits
all three states.  Run on an MI355X with ``pytest -m gpu``."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wb_golden.npz")
SENT_I16 = 12321          # what every output holds before a launch
SENT_F32 = 54321.5
SENT_INT = -77
BOUNDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 40, 41, 97, 150, 303)
FIXTURE = {  # frames of 160, onset, first output: the fixture's own numbers
    0: (100, 0, 4), 1: (100, 2, 6), 2: (300, 0, 4), 3: (300, 0, 4), 4: (303, 3, 7), 5: (4, 0, -1)}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    for u, (nfr, onset, first) in FIXTURE.items():
        assert (len(g[f"x{u}"]) // 160, int(g["onset"][u]), int(g["first_out"][u])) == (nfr, onset, first)
    assert len(g["x4"]) % 160 == 77
    return g


def _sorted_fixtures(g):
    """the six utterances longest first (stable), so that the utterances of a later slice are a prefix of the list"""
    ids = sorted(range(6), key=lambda u: -(len(g[f"x{u}"]) // 160))
    assert ids == [4, 2, 3, 0, 1, 5]
    return ids, [g[f"x{u}"] for u in ids]


class _Buffers:
    """Sentinel-filled outputs of one launch over a PackedBatch, and their per-utterance pieces afterwards."""

    def __init__(self, sea, batch, first=None, onset=None):
        torch = _torch()
        lib = sea.load()
        dev = batch.data.device
        self.sea, self.batch = sea, batch
        half = (batch.total // 2 + 7) // 8 * 8
        rows = int(lib.sea_wb_rows(batch.total))
        self.out = torch.full((half,), SENT_I16, dtype=torch.int16, device=dev)
        self.f32 = torch.full((half,), SENT_F32, dtype=torch.float32, device=dev)
        self.hp = torch.full((rows, 3), SENT_F32, dtype=torch.float32, device=dev)
        self.code = torch.full((rows, 9), SENT_F32, dtype=torch.float32, device=dev)
        self.first = first if first is not None else torch.full((batch.n_utt,), SENT_INT, dtype=torch.int32, device=dev)
        self.onset = onset if onset is not None else torch.full((batch.n_utt,), SENT_INT, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(batch.total, batch.n_utt)) // 4 + 4, dtype=torch.float32, device=dev)

    def pieces(self):
        """per utterance of the batch: (out int16, f32 [frames, 80], hp [frames, 3], code [frames, 9])"""
        sea, b = self.sea, self.batch
        out, f32 = sea.wb_split(b, self.out), sea.wb_split(b, self.f32)
        hp, code = sea.wb_rows(b, self.hp), sea.wb_rows(b, self.code)
        return [(out[u], f32[u].reshape(-1, 80), hp[u], code[u]) for u in range(b.n_utt)]


def _one_launch(sea, utts):
    """sea_wb_denoise_batch into sentinel-filled buffers -> per utterance dict"""
    torch = _torch()
    lib = sea.load()
    b = sea.PackedBatch.from_arrays(utts, device="cuda:0")
    B = _Buffers(sea, b)
    rc = lib.sea_wb_denoise_batch(_p(b.data), _p(B.out), _p(B.f32), _p(b.offsets), _p(b.lengths), _p(b.order), _p(B.first),
                                  _p(B.onset), _p(B.hp), _p(B.code), _p(B.scratch), b.total, b.n_utt, None)
    assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    first, onset = B.first.cpu().numpy(), B.onset.cpu().numpy()
    return [dict(out=o, f32=f, hp=h, code=c, first_out=int(first[u]), onset=int(onset[u]))
            for u, (o, f, h, c) in enumerate(B.pieces())]


def _in_slices(sea, utts, bounds):
    """The same utterances (longest first) cut at `bounds` (frames of 160), one sea_wb_denoise_batch_slice per slice; the
    last slice of an utterance carries its ragged tail.  The state starts as NaN: resume = 0 must not read it."""
    torch = _torch()
    lib = sea.load()
    n = len(utts)
    nfr = [len(x) // 160 for x in utts]
    assert nfr == sorted(nfr, reverse=True) and bounds[0] == 0 and bounds[-1] >= nfr[0]
    nstate = int(lib.sea_wb_slice_state_floats())
    state = torch.full((n, nstate), float("nan"), dtype=torch.float32, device="cuda:0")
    first = torch.full((n,), SENT_INT, dtype=torch.int32, device="cuda:0")
    onset = torch.full((n,), SENT_INT, dtype=torch.int32, device="cuda:0")
    got = [dict(out=[], f32=[], hp=[], code=[]) for _ in utts]
    for k in range(len(bounds) - 1):
        b0, b1 = bounds[k], bounds[k + 1]
        act = [u for u in range(n) if nfr[u] > b0]
        assert act == list(range(len(act)))
        parts = [utts[u][160 * b0:160 * b1] if b1 < nfr[u] else utts[u][160 * b0:] for u in act]
        b = sea.PackedBatch.from_arrays(parts, device="cuda:0")
        B = _Buffers(sea, b, first, onset)
        rc = lib.sea_wb_denoise_batch_slice(_p(b.data), _p(B.out), _p(B.f32), _p(b.offsets), _p(b.lengths), _p(b.order),
                                            _p(first), _p(onset), _p(B.hp), _p(B.code), _p(B.scratch), b.total, _p(state),
                                            b.n_utt, b0, 1 if k > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
        torch.cuda.synchronize()
        for u, (o, f, h, c) in zip(act, B.pieces()):
            for key, v in zip(("out", "f32", "hp", "code"), (o, f, h, c)):
                got[u][key].append(v)
    first, onset = first.cpu().numpy(), onset.cpu().numpy()
    return [dict(out=np.concatenate(g["out"]), f32=np.concatenate(g["f32"]), hp=np.concatenate(g["hp"]),
                 code=np.concatenate(g["code"]), first_out=int(first[u]), onset=int(onset[u])) for u, g in enumerate(got)]


def _assert_same_bits(got, want, what):
    assert (got["first_out"], got["onset"]) == (want["first_out"], want["onset"]), \
        f"{what}: first_out / onset {got['first_out']} / {got['onset']}, one launch {want['first_out']} / {want['onset']}"
    assert got["out"].shape == want["out"].shape and np.array_equal(got["out"], want["out"]), \
        f"{what}: {int((got['out'] != want['out']).sum())} low-band samples differ from the one launch"
    for k in ("f32", "hp", "code"):
        assert got[k].shape == want[k].shape, f"{what}: {k} {got[k].shape} != {want[k].shape}"
        bad = int((_u32(got[k]) != _u32(want[k])).sum())
        assert bad == 0, f"{what}: {bad} of {got[k].size} values of {k} differ in bits from the one launch"


def _assert_within_tolerance(got, g, u, what):
    """the checks of tests/test_gpu_wb.py::_compare (without the cepstra) against the reference's recorded outputs"""
    nfr = len(g[f"x{u}"]) // 160
    fo, on = int(g["first_out"][u]), int(g["onset"][u])
    assert got["first_out"] == fo, f"{what}: first_out {got['first_out']} != {fo}"
    assert got["onset"] == on, f"{what}: onset {got['onset']} != {on}"
    nout = nfr - fo if fo >= 0 else 0
    assert len(g[f"hp{u}"]) == nout
    quiet = fo if fo >= 0 else nfr
    want_i16 = g[f"out{u}"]
    assert not got["out"][:80 * quiet].any() and not want_i16[:80 * quiet].any(), f"{what}: non-zero samples before the first output"
    d = np.abs(got["out"].astype(np.int32) - want_i16.astype(np.int32))
    print(f"\n{what}: int16 max |delta| {int(d.max())} LSB, {int((d != 0).sum())} of {d.size} samples differ")
    assert d.max() <= 2, f"{what}: int16 max |delta| {d.max()} LSB"
    assert (d != 0).sum() <= 1e-3 * d.size, f"{what}: {(d != 0).sum()} of {d.size} int16 samples differ"

    def flt(key, a, ref):
        if not ref.size:
            return
        e = np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64)))
        print(f"  {key}: max error {e.max():.3g}, {int((_u32(a) != _u32(ref)).sum())} of {a.size} values differ in bits")
        assert e.max() <= 1e-4, f"{what}: {key}: max error {e.max()}"

    if f"f32_{u}" in g:
        flt("float stream", got["f32"][quiet:], g[f"f32_{u}"])
    flt("high-band rows", got["hp"][quiet:], g[f"hp{u}"])
    flt("code", got["code"][quiet:], g[f"code{u}"])
    # frames without an output: nothing wrote their rows or their float frames
    sent = np.float32(SENT_F32).view(np.uint32)
    for k in ("hp", "code", "f32"):
        assert (_u32(got[k][:quiet]) == sent).all(), f"{what}: {k} of frames without an output was written"


def test_slices_equal_one_launch(gold):
    """All six fixture utterances cut at BOUNDS: cuts in the leading zeros of utterances 1 and 4, at every frame of the
    four-frame latency, single-frame slices, slices past the end of utterance 5 and then of 0 and 1.  Concatenated low band,
    float stream, rows, first_out and onset are the one launch's bit for bit, and within tolerance of the reference's."""
    import speech_enhancement_amd as sea
    ids, utts = _sorted_fixtures(gold)
    want = _one_launch(sea, utts)
    got = _in_slices(sea, utts, BOUNDS)
    for j, u in enumerate(ids):
        _assert_same_bits(got[j], want[j], f"fixture utterance {u}")
    for j, u in enumerate(ids):
        _assert_within_tolerance(got[j], gold, u, f"fixture utterance {u} in slices")
        assert not (got[j]["out"] == SENT_I16).all() and got[j]["out"].size == 80 * FIXTURE[u][0]


def test_one_utterance_in_single_frame_slices(gold):
    """Fixture 2 alone in 300 launches of one frame each: every transition of the high-band VAD, every hang-over count and
    every warm-up count (n < 10, n < 100) is a cut, and every history is shifted by one frame 299 times."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    x = gold["x2"]
    nfr = len(x) // 160
    assert nfr == 300 and len(x) == 160 * nfr
    want = _one_launch(sea, [x])[0]
    dev = "cuda:0"
    d_in = torch.from_numpy(x.copy()).to(dev)
    out = torch.full((80 * nfr,), SENT_I16, dtype=torch.int16, device=dev)
    f32 = torch.full((80 * nfr,), SENT_F32, dtype=torch.float32, device=dev)
    hp = torch.full((nfr + 1, 3), SENT_F32, dtype=torch.float32, device=dev)
    code = torch.full((nfr + 1, 9), SENT_F32, dtype=torch.float32, device=dev)
    first = torch.full((1,), SENT_INT, dtype=torch.int32, device=dev)
    onset = torch.full((1,), SENT_INT, dtype=torch.int32, device=dev)
    meta = torch.tensor([0, 160], dtype=torch.int64, device=dev)  # one frame at offset 0 of whatever the pointers point at
    state = torch.full((1, int(lib.sea_wb_slice_state_floats())), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(160, 1)) // 4 + 4, dtype=torch.float32, device=dev)
    for f in range(nfr):  # frame f: 320 bytes of input, 160 of int16 output, 320 of float output, one row of 12 and of 36 bytes
        rc = lib.sea_wb_denoise_batch_slice(_p(d_in, 320 * f), _p(out, 160 * f), _p(f32, 320 * f), _p(meta), _p(meta, 8), None,
                                            _p(first), _p(onset), _p(hp, 12 * f), _p(code, 36 * f), _p(scratch), 160, _p(state),
                                            1, f, 1 if f > 0 else 0, None)
        assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    got = dict(out=out.cpu().numpy(), f32=f32.cpu().numpy().reshape(nfr, 80), hp=hp.cpu().numpy()[:nfr], code=code.cpu().numpy()[:nfr],
               first_out=int(first.cpu()[0]), onset=int(onset.cpu()[0]))
    _assert_same_bits(got, want, "fixture utterance 2 in 300 slices")
    assert (got["first_out"], got["onset"]) == (4, 0)


def test_slice_arguments_are_checked(gold):
    """NULL state, hp_rows without code_rows, a total that is no multiple of 8, a negative frame_base: non-zero, a message,
    and no launch (the outputs keep their sentinel)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    b = sea.PackedBatch.from_arrays([gold["x5"]], device="cuda:0")
    B = _Buffers(sea, b)
    state = torch.zeros((1, int(lib.sea_wb_slice_state_floats())), dtype=torch.float32, device="cuda:0")

    def call(state=state, hp=B.hp, code=B.code, total=b.total, frame_base=0):
        return lib.sea_wb_denoise_batch_slice(_p(b.data), _p(B.out), _p(B.f32), _p(b.offsets), _p(b.lengths), None, _p(B.first),
                                              _p(B.onset), _p(hp), _p(code), _p(B.scratch), total, _p(state), 1, frame_base, 0, None)

    for what, kw, word in (("NULL state", dict(state=None), "d_state"), ("hp_rows without code_rows", dict(code=None), "come together"),
                           ("code_rows without hp_rows", dict(hp=None), "come together"),
                           ("total_padded_samples not a multiple of 8", dict(total=b.total + 4), "multiple of 8"),
                           ("negative frame_base", dict(frame_base=-1), "frame_base")):
        rc = call(**kw)
        msg = lib.sea_last_error().decode()
        assert rc != 0 and "sea_wb_denoise_batch_slice" in msg and word in msg, f"{what}: rc {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert (B.out.cpu().numpy() == SENT_I16).all() and (B.first.cpu().numpy() == SENT_INT).all(), "a refused call launched something"
    assert call() == 0, lib.sea_last_error()  # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert int(B.first.cpu()[0]) == -1 and int(B.onset.cpu()[0]) == 0 and not B.out.cpu().numpy()[:320].any()


def _batch_rows(sea, utts):
    """sea_wb_denoise_batch through the engine: per utterance (out, hp rows, code rows), rows of frames without an output zero"""
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device="cuda:0")
    r = sea.wb_denoise_batch(b, want_hb=True)
    torch.cuda.synchronize()
    return list(zip(sea.wb_split(b, r["out"]), sea.wb_rows(b, r["hp_rows"]), sea.wb_rows(b, r["code_rows"])))


def test_host_pipeline_equals_one_launch(gold):
    """sea_wb_denoise_utterances on (i) the six fixtures plus 31 short synthetic utterances of 0 .. 40 frames, some ragged,
    one empty, one all-zero, (ii) a list of ONE utterance of 120 s, and (iii) twelve utterances of 2000 .. 0 frames, some ragged
    -- a list that is both cut and ragged, so the slices' active prefix shrinks.  The pipeline must cut (ii) and (iii) into
    several launches: low band and rows are sea_wb_denoise_batch's bit for bit, and a cut list run twice gives the same bits twice."""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    _torch()
    utts = [gold[f"x{u}"] for u in range(6)]
    for i in range(29):
        n = 1 + (i * 11) % 40
        L = 160 * n + (0 if i % 3 else 17 + i)
        utts.append(corpus.synth_wideband(60 + i, L) if i % 2 else corpus.synth_utterance(60 + i, L))
    utts += [np.zeros(0, np.int16), np.zeros(160 * 9 + 5, np.int16)]
    assert len(utts) == 37 and sum(len(x) % 160 != 0 for x in utts) >= 10
    long_one = np.tile(corpus.synth_wideband(3, 16000 * 4), 30)
    assert len(long_one) == 16000 * 120
    ragged = []
    for i, n in enumerate((2000, 1500, 1200, 900, 700, 500, 300, 200, 100, 40, 9, 0)):
        L = 160 * n + (0 if i % 3 else 17 + i)
        ragged.append(corpus.synth_wideband(100 + i, L) if i % 2 else corpus.synth_utterance(100 + i, L))
    assert sum(len(x) // 160 for x in ragged) == 7449 and sum(len(x) % 160 != 0 for x in ragged) == 4
    for name, lst, cut in (("short list", utts, False), ("one long utterance", [long_one], True), ("cut and ragged list", ragged, True)):
        want = _batch_rows(sea, lst)
        got = sea.wb_denoise_utterances(lst, want_hb=True)
        plain = sea.wb_denoise_utterances(lst)
        if cut:
            assert got["slices"] > 1 and plain["slices"] > 1, f"{name}: run as {got['slices']} launch(es)"
            again = sea.wb_denoise_utterances(lst, want_hb=True)
        else:
            again = None
        for u, (o, h, c) in enumerate(want):
            what = f"{name}, utterance {u} ({len(lst[u])} samples)"
            assert got["out"][u].shape == o.shape and np.array_equal(got["out"][u], o), f"{what}: low band != one launch"
            assert np.array_equal(plain["out"][u], o), f"{what}: low band without rows != one launch"
            assert np.array_equal(_u32(got["hp_rows"][u]), _u32(h)), f"{what}: high-band rows != one launch"
            assert np.array_equal(_u32(got["code_rows"][u]), _u32(c)), f"{what}: code rows != one launch"
            if again is not None:
                assert np.array_equal(again["out"][u], got["out"][u]) and np.array_equal(_u32(again["hp_rows"][u]), _u32(got["hp_rows"][u])) \
                    and np.array_equal(_u32(again["code_rows"][u]), _u32(got["code_rows"][u])), f"{what}: two runs differ"
        print(f"\n{name}: {len(lst)} utterance(s), {got['slices']} launch(es), equal to the one launch bit for bit")


def _edge_set():
    """the wideband edge set (tests/ns_edge_cases.signals_wb()), longest first, and the bounds tests/wb_edge_cuts.py derives
    from the reference: -> (names, utterances, bounds)"""
    from tests import ns_edge_cases as E
    from tests import test_gpu_wb as WB
    from tests import wb_edge_cuts as K
    WB._reference()                      # the cuts come from the reference run live: a missing library is a failure
    sig = E.signals_wb()
    names = sorted(sig, key=lambda k: -(len(sig[k]) // 160))
    return names, [sig[k] for k in names], K.bounds()


def test_edge_set_in_slices():
    """The eight signals of the wideband edge set, longest first, cut where the reference says their branches are taken:
    every frame of the first thirteen, one-frame slices across the frames at which the low band's two noise-estimate floors
    (114, 450) and the high band's (1373) are first reached, across the first frame of a hang-over of the high band's VAD,
    two cuts while the estimates sit on their floors and one-frame slices
    across the start of the closing noise, whose rows are the first to show what the high band's estimate holds.  A state that drops the word one of these rules reads changes the
    bits behind the cut: everything equals the one launch bit for bit."""
    import speech_enhancement_amd as sea
    names, utts, bounds = _edge_set()
    assert {1373, 1374, 114, 115, 450, 451, 1510, 1511} <= set(bounds) and bounds[-1] == len(utts[0]) // 160
    want = _one_launch(sea, utts)
    got = _in_slices(sea, utts, bounds)
    words = 0
    for j, name in enumerate(names):
        _assert_same_bits(got[j], want[j], f"edge signal {name}")
        words += sum(got[j][k].size for k in ("out", "f32", "hp", "code")) + 2
    hp = want[names.index("ones_then_zeros_wb")]["hp"]     # the rows that read the floored estimate: the closing noise's
    assert not hp[1400:1500].any() and (hp[1512:1520] > 0).all() and (hp[1512:1520] < SENT_F32).all()
    print(f"\n{len(bounds) - 1} slices, {words} words compared with the one launch, 0 differ")


def test_edge_set_through_the_host_pipeline():
    """The edge set four times over (32 utterances, enough bytes for sea_wb_denoise_utterances to cut the list) against
    sea_wb_denoise_batch: low band and rows bit for bit."""
    import speech_enhancement_amd as sea
    _torch()
    names, utts, _ = _edge_set()
    lst = utts * 4
    want = _batch_rows(sea, lst)
    got = sea.wb_denoise_utterances(lst, want_hb=True)
    assert got["slices"] > 1, f"run as {got['slices']} launch(es)"
    words = 0
    for u, (o, h, c) in enumerate(want):
        what = f"edge signal {names[u % len(names)]} (copy {u // len(names)})"
        assert got["out"][u].shape == o.shape and np.array_equal(got["out"][u], o), f"{what}: low band != one launch"
        assert np.array_equal(_u32(got["hp_rows"][u]), _u32(h)), f"{what}: high-band rows != one launch"
        assert np.array_equal(_u32(got["code_rows"][u]), _u32(c)), f"{what}: code rows != one launch"
        words += o.size + h.size + c.size
    print(f"\n{len(lst)} utterances, {got['slices']} launches, {words} words compared with the one launch, 0 differ")
