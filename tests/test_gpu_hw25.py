"""The Hu-Wang front half on the 25-channel 8 kHz bank on the GPU (csrc/hw25_kernel.hip) against what the reference's own
functions produced (tests/golden/hw25_golden.npz) and, at the shapes the fixture does not hold, the numpy model that the CPU
tests pin to that fixture (tests/hw25_model.py).  Floats are compared bit for bit, NaNs by position.

One batch of seven utterances: the fixture's inputs (a), (b), (c) (1210 samples: 15 frames, not a multiple of 8 or 80), then
79 samples (no frame, no row), the fixture's (d) (80 samples: one frame, every window cut at both ends), 163 samples and 647
samples of white noise (pitch != length, odd row offsets).  Frames 0-3 cut the 400-sample window at the start of the signal,
the last frame of every utterance at its end; the labelling takes all four outcomes on (a)-(c).  Every output buffer is
filled with a sentinel and carries guard rows."""
import ctypes

import numpy as np
import pytest

from tests import hw25_model as M

pytestmark = pytest.mark.gpu

NCH, NDEL = 25, 101
SENT, SENT_I = -7777.25, -77
GUARD_ROWS, GUARD_FLOATS = 3, 64
PERM = [3, 6, 0, 5, 2, 4, 1]
ARRAYS = ("hOut", "hEv", "acf_hc", "acf_ev", "cross_hc", "cross_ev", "pitch", "pRatio", "mark")
FRAME_ARRAYS = ("cross_hc", "cross_ev", "pitch", "pRatio", "mark")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def seven_inputs():
    """the seven utterances of the batch, what each must give (the fixture's arrays or the model's) and the tables; also the
    building blocks of tests/test_gpu_launch_caps.py"""
    g = M.load_golden()
    t = M.tables()
    rng = np.random.default_rng(25)
    n = np.arange(647)
    extra = {3: (40 * np.sin(2 * np.pi * 200 * n[:79] / 8000)).astype(np.float32),
             5: (np.linspace(-300, 900, 163) + rng.uniform(-50, 50, 163)).astype(np.float32),
             6: rng.integers(-2000, 2001, 647).astype(np.float32)}
    utts, want = [], []
    for u, k in enumerate(["a", "b", "c", None, "d", None, None]):
        if k:
            utts.append(g[f"x_{k}"])
            want.append({name: g[f"{name}_{k}"] for name in ARRAYS})
        else:
            utts.append(extra[u])
            want.append(M.frontend(extra[u], t))
    assert [len(x) for x in utts] == [1210, 1210, 1210, 79, 80, 163, 647]
    return utts, want, t


@pytest.fixture(scope="module")
def case():
    """the batch and, computed once, what every utterance must give"""
    import torch
    import speech_enhancement_amd as sea
    utts, want, t = seven_inputs()
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    rows = np.array([len(x) // 80 for x in utts], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    assert rows.tolist() == [15, 15, 15, 0, 1, 2, 8] and offs.tolist() == [0, 15, 30, 45, 45, 46, 48]
    return dict(utts=utts, want=want, batch=batch, rows=rows, offs=offs, d_offs=torch.from_numpy(offs).to("cuda:0"),
                d_perm=torch.tensor(PERM, dtype=torch.int32, device="cuda:0"), tables=t)


def _launch(case, mode, order, want_acf):
    """the C calls on sentinel-filled buffers with guard rows; mode: "group" = sea_hw25_frontend_batch, "two" = the periphery
    and the correlogram call one after the other"""
    import torch
    from speech_enhancement_amd import _lib
    lib = _lib.load()
    b = case["batch"]
    nrows = int(case["rows"].sum())
    dev = b.data.device

    def full(shape, value=SENT, dtype=torch.float32):
        return torch.full(shape, value, dtype=dtype, device=dev)

    o = dict(hout=full((b.total * NCH + GUARD_FLOATS,)), hev=full((b.total * NCH + GUARD_FLOATS,)),
             acf_hc=full((nrows + GUARD_ROWS, NCH, NDEL)) if want_acf else None,
             acf_ev=full((nrows + GUARD_ROWS, NCH, NDEL)) if want_acf else None,
             cross_hc=full((nrows + GUARD_ROWS, NCH)), cross_ev=full((nrows + GUARD_ROWS, NCH)),
             pitch=full((nrows + GUARD_ROWS,), SENT_I, torch.int32), pratio=full((nrows + GUARD_ROWS, NCH)),
             mark=full((nrows + GUARD_ROWS, NCH)))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_order = _ptr(case["d_perm"]) if order else None
    tail = [_ptr(b.offsets), _ptr(b.lengths), _ptr(case["d_offs"]), _ptr(o["acf_hc"]), _ptr(o["acf_ev"]), _ptr(o["cross_hc"]),
            _ptr(o["cross_ev"]), _ptr(o["pitch"]), _ptr(o["pratio"]), _ptr(o["mark"]), None, d_order, b.n_utt, stream]
    if mode == "group":
        _lib.check(lib.sea_hw25_frontend_batch(_ptr(b.data), _ptr(o["hout"]), _ptr(o["hev"]), *tail), "sea_hw25_frontend_batch")
    else:
        _lib.check(lib.sea_hw25_periphery_batch(_ptr(b.data), _ptr(o["hout"]), _ptr(o["hev"]), _ptr(b.offsets), _ptr(b.lengths),
                                                d_order, b.n_utt, stream), "sea_hw25_periphery_batch")
        _lib.check(lib.sea_hw25_correlogram_batch(_ptr(o["hout"]), _ptr(o["hev"]), *tail), "sea_hw25_correlogram_batch")
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


@pytest.fixture(scope="module")
def runs(case):
    return {"group_plain": _launch(case, "group", False, True), "two_permuted": _launch(case, "two", True, True),
            "group_permuted_noacf": _launch(case, "group", True, False)}


def _utterance(case, out, u):
    off, L = int(case["batch"].host_offsets[u]), len(case["utts"][u])
    pitch = (L + 7) // 8 * 8
    r0, n = int(case["offs"][u]), int(case["rows"][u])

    def block(a):
        return a[off * NCH:off * NCH + NCH * pitch].reshape(NCH, pitch)

    def rows(a):
        return None if a is None else a[r0:r0 + n]

    return dict(hOut=block(out["hout"])[:, :L], hEv=block(out["hev"])[:, :L], pad_hOut=block(out["hout"])[:, L:],
                pad_hEv=block(out["hev"])[:, L:], acf_hc=rows(out["acf_hc"]), acf_ev=rows(out["acf_ev"]),
                cross_hc=rows(out["cross_hc"]), cross_ev=rows(out["cross_ev"]), pitch=rows(out["pitch"]), pRatio=rows(out["pratio"]),
                mark=rows(out["mark"]))


@pytest.mark.parametrize("run", ["group_plain", "two_permuted"])
def test_every_array_equals_the_reference_or_the_model(case, runs, run):
    for u, want in enumerate(case["want"]):
        got = _utterance(case, runs[run], u)
        for name in ARRAYS:
            assert M.same_bits(np.ascontiguousarray(got[name]), want[name]), f"{run}, utterance {u}: {name}"
    marks = np.concatenate([case["want"][u]["mark"].ravel() for u in range(3)])
    assert 5 <= marks.sum() <= marks.size - 5


def test_null_acf_pointers_give_the_same_frame_outputs(case, runs):
    a, b = runs["two_permuted"], runs["group_permuted_noacf"]
    assert b["acf_hc"] is None and b["acf_ev"] is None
    for name in ("hout", "hev", "cross_hc", "cross_ev", "pitch", "pratio", "mark"):
        assert M.same_bits(a[name], b[name]), name


def test_the_launch_group_equals_the_two_calls(runs):
    a, b = runs["group_plain"], runs["two_permuted"]
    for name, v in a.items():
        assert M.same_bits(v, b[name]), name


def test_guard_rows_and_padding_are_untouched(case, runs):
    nrows = int(case["rows"].sum())
    total = case["batch"].total
    for run, out in runs.items():
        for name in ("hout", "hev"):
            assert (out[name][total * NCH:] == SENT).all(), f"{run}: {name} guard"
        for name in ("acf_hc", "acf_ev", "cross_hc", "cross_ev", "pratio", "mark"):
            if out[name] is not None:
                assert (out[name][nrows:] == SENT).all(), f"{run}: {name} guard rows"
                assert not (out[name][:nrows] == SENT).any(), f"{run}: {name} has an unwritten row"
        assert (out["pitch"][nrows:] == SENT_I).all() and ((out["pitch"][:nrows] >= 16) & (out["pitch"][:nrows] <= 100)).all()
        for u in range(len(case["utts"])):
            got = _utterance(case, out, u)
            assert (got["pad_hOut"] == SENT).all() and (got["pad_hEv"] == SENT).all(), f"{run}: padding of utterance {u}"
    # the 79-sample utterance has no frame: it owns no row, its neighbours' rows are adjacent
    assert case["rows"][3] == 0 and case["offs"][4] == case["offs"][3]
    assert _utterance(case, runs["group_plain"], 3)["pitch"].size == 0


def test_python_layer_and_single_utterance_form(case, runs):
    import speech_enhancement_amd as sea
    res = sea.hw25_frontend_batch(case["batch"], want_acf=True)
    for u in (1, 3, 4, 5):
        got, want = res.utterance(u), case["want"][u]
        for name in ARRAYS:
            assert M.same_bits(np.ascontiguousarray(got[name]), want[name]), f"hw25_frontend_batch, utterance {u}: {name}"
    assert sea.hw25_frontend_batch(case["batch"]).acf_hc is None
    hout, hev = sea.hw25_periphery_batch(case["batch"], use_order=False)
    assert M.same_bits(sea.hw25_split(case["batch"], hout)[6], case["want"][6]["hOut"])
    assert M.same_bits(sea.hw25_split(case["batch"], hev)[6], case["want"][6]["hEv"])
    for u in (1, 5):  # sea_hw25_frontend equals its row of the batch
        one = sea.hw25_frontend(case["utts"][u])
        for name in ARRAYS:
            assert M.same_bits(one[name], case["want"][u][name]), f"hw25_frontend, utterance {u}: {name}"
    # an int16 batch converts exactly: the white-noise utterance holds integers
    i16 = sea.PackedBatch.from_arrays([case["utts"][6].astype(np.int16)], device="cuda:0")
    got = sea.hw25_frontend_batch(i16).utterance(0)
    for name in FRAME_ARRAYS + ("hOut", "hEv"):
        assert M.same_bits(np.ascontiguousarray(got[name]), case["want"][6][name]), f"int16 batch: {name}"


def test_silent_streams_take_the_zero_rms_branch(case):
    """the correlogram call on streams that ARE zero (the periphery never produces them): ACF 0, RMS 0 and not divided by,
    pRatio 0 / 0 = NaN"""
    import torch
    import speech_enhancement_amd as sea
    stream = np.zeros((NCH, 163), np.float32)
    stream[5] = np.linspace(1, 60, 163, dtype=np.float32)
    stream[6] = np.linspace(60, 1, 163, dtype=np.float32) ** 2
    batch = sea.PackedBatch.from_arrays([np.zeros(163, np.float32)], device="cuda:0", dtype=np.float32)
    block = np.zeros((NCH, 168), np.float32)
    block[:, :163] = stream
    hout = torch.from_numpy(block.ravel().copy()).to("cuda:0")
    hev = torch.from_numpy((block * np.float32(0.5)).ravel().copy()).to("cuda:0")
    got = sea.hw25_correlogram_batch(batch, hout, hev, want_acf=True).utterance(0)
    w = case["tables"]["winsize"]
    a_hc, a_ev = M.acf(stream, w), M.acf(stream * np.float32(0.5), w)
    pitch = M.global_pitch(a_hc)
    want = dict(acf_hc=a_hc, acf_ev=a_ev, cross_hc=M.cross_corr(a_hc), cross_ev=M.cross_corr(a_ev), pitch=pitch,
                pRatio=M.p_ratio(a_hc, pitch))
    want["mark"] = M.initial_mark(want["cross_hc"], a_hc)
    assert np.isnan(want["pRatio"][:, 0]).all() and not want["acf_hc"][:, 0].any()
    for name, v in want.items():
        assert M.same_bits(np.ascontiguousarray(got[name]), v), name


def test_more_utterances_than_a_grid_dimension_y_holds(case):
    """65 537 utterances: the launches must carry the utterance index on grid x (y ends at 65 535).  All are eight zeros (no
    frame) but the last, the fixture's (d); eight zeros give the first eight samples of (d)'s hOut (the chain is causal) and the
    model's hEv (the filter is cut at the end of the signal)."""
    import speech_enhancement_amd as sea
    g = M.load_golden()
    n = 65537
    utts = [np.zeros(8, np.float32)] * (n - 1) + [g["x_d"]]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    res = sea.hw25_frontend_batch(batch, want_acf=True)
    last = res.utterance(n - 1)
    for name in ARRAYS:
        assert M.same_bits(np.ascontiguousarray(last[name]), g[f"{name}_d"]), name
    hout8 = np.ascontiguousarray(g["hOut_d"][:, :8])
    hev8 = M.lowpass(hout8, case["tables"]["lp"])
    for u in (0, 1, 40000, 65535):
        got = res.utterance(u)
        assert M.same_bits(np.ascontiguousarray(got["hOut"]), hout8) and M.same_bits(np.ascontiguousarray(got["hEv"]), hev8), u
        assert got["pitch"].size == 0


# ---- the edge set ------------------------------------------------------------------------------------------------------------
EDGE_PERM = [2, 0, 3, 1]


def test_edge_inputs_in_one_batch_with_present_ones(case):
    """The edge set's audio (tests/hw25_model.EDGE_INPUTS) between the fixture's (b) and the white noise of the batch above:
    edc, whose hair-cell output is exactly 0 over whole ACF windows (both normalising sums 0 and not divided by, pRatio 0 / 0),
    and ewhole, voiced from the first sample to the last.  Every array against tests/golden/hw25_edge_golden.npz, bit for bit
    (the large ones through their CRC32), in plain and permuted launch order, as one launch group and as two calls, with and
    without the ACF outputs; guard rows and padding untouched."""
    import torch
    import speech_enhancement_amd as sea
    from tests import hw_edge as E
    e = E.load("hw25")
    names = [None, "edc", "ewhole", None]
    utts = [case["utts"][1], e["x_edc"], e["x_ewhole"], case["utts"][6]]
    rows = np.array([len(x) // 80 for x in utts], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    c = dict(utts=utts, batch=sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32), rows=rows, offs=offs,
             d_offs=torch.from_numpy(offs).to("cuda:0"), d_perm=torch.tensor(EDGE_PERM, dtype=torch.int32, device="cuda:0"))
    assert int(np.isnan(e["front_pRatio_edc"]).sum()) > 100 and (e["front_cross_hc_edc"] == 0).sum() > 100
    assert e["front_mark_ewhole"].sum() > 100 and e["front_mark_ewhole"][-1].sum() > 0
    runs = {"group_plain": _launch(c, "group", False, True), "two_permuted": _launch(c, "two", True, True),
            "group_permuted_noacf": _launch(c, "group", True, False)}
    nrows = int(rows.sum())
    for run in ("group_plain", "two_permuted"):
        tally = E.Tally(f"hw25 front half, edge set, {run}")
        for u, k in enumerate(names):
            got = _utterance(c, runs[run], u)
            if k:
                E.add_front(tally, got, e, k, k)
            else:
                for name in ARRAYS:
                    tally.add(got[name], case["want"][1 if u == 0 else 6][name], f"utterance {u} {name}")
        tally.done()
    for name in ("hout", "hev", "cross_hc", "cross_ev", "pitch", "pratio", "mark"):
        assert M.same_bits(runs["two_permuted"][name], runs["group_permuted_noacf"][name]), name
    for run, out in runs.items():
        for name in ("hout", "hev"):
            assert (out[name][c["batch"].total * NCH:] == SENT).all(), f"{run}: {name} guard"
        for name in ("acf_hc", "acf_ev", "cross_hc", "cross_ev", "pratio", "mark"):
            if out[name] is not None:
                assert (out[name][nrows:] == SENT).all() and not (out[name][:nrows] == SENT).any(), f"{run}: {name} rows"
        assert (out["pitch"][nrows:] == SENT_I).all()
        for u in range(4):
            got = _utterance(c, out, u)
            assert (got["pad_hOut"] == SENT).all() and (got["pad_hEv"] == SENT).all(), f"{run}: padding of utterance {u}"
