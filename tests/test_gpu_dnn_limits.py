"""The DNN mask estimator at the limits of its contract, every comparison bit for bit as values
against the plain-C model of tests/dnn_model.py on the inputs of tests/dnn_limits_cases.py: eight layers, width 4096 as N and
as K, context 15; the chunked paths of sea_dnn_forward and sea_cochleagram_utterances (SEA_DNN_SCRATCH_MB); utterances of no
row; features that are not finite.  The last of these stands here and not in tests/nonfinite_cases.py, whose table holds
frame streams of the NoiseSup entry points compared against the reference: this entry point's reference is the C model."""
import ctypes

import numpy as np
import pytest

from tests import dnn_limits_cases as L
from tests import dnn_model as M
from tests.test_gpu_dnn import LENGTHS, _device_net, _same, _sea

pytestmark = pytest.mark.gpu


# ---- the limits that are accepted -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.FORWARD_LIMITS + ("context15",))
def test_forward_at_the_limits_equals_the_c_model(name):
    """eight layers (the ping-pong buffers' parity, d_w[4..7]); width 4096 as N (32 N tiles, the dense last-layer store at
    ldy = 4096) and as K (128 K tiles into one accumulator); context 15 (K0 = 1984) on utterances of 1 and 129 rows with the
    network of the launch-cap case"""
    sea = _sea()
    net, feats = (L.sgd_case().net, L.context15_feats()) if name == "context15" else (L.limit_case(name).net, L.forward_feats(name))
    want = M.forward(net, feats)
    got = sea.dnn_forward(_device_net(net), feats)
    for u, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{name}: context {net.context}, {net.dims[1:]}, utterance {u} of {len(w)} rows")


def test_every_stage_of_an_eight_layer_chain_is_timed():
    """the eight-layer network has 64 outputs: the chain on one short utterance fills all eight layer slots of the stage table"""
    sea = _sea()
    lib = sea.load()
    net = L.limit_case("eight").net
    assert len(net.weights) == 8 and net.dims[-1] == 64
    x = (6000 * np.sin(np.arange(1600) * 0.07)).astype(np.int16)
    model = _device_net(net)
    audio, masks = sea.dnn_enhance_utterances(model, [x], masks=True)
    assert sea.dnn_last_chunks() == 1 and audio[0].shape == x.shape
    _same(masks[0], M.forward(net, [M.cochleagram(sea.subbband(x))])[0], "the chain's mask through eight layers")
    times = [lib.sea_dnn_last_stage_ms(s) for s in range(13)]  # SEA_DNN_STAGE_SUBBAND .. SEA_DNN_STAGE_ALL: all exist at 8 layers
    print("stage ms", times)
    assert all(t >= 0 for t in times), times
    assert lib.sea_dnn_last_stage_ms(13) == -1.0


# ---- the chunked host paths and utterances of no row ------------------------------------------------------------------------------
SENTINEL = np.float32(7.0)


def _forward_raw(sea, model, feats):
    """sea_dnn_forward through ctypes: an utterance of no row passes a NULL feature pointer and an output buffer of one row of
    sentinels, which the call must not touch -> (return code, outputs)"""
    n = len(feats)
    outs = [np.full((max(len(f), 1), model.n_out), SENTINEL, np.float32) for f in feats]
    fp = (ctypes.c_void_p * n)(*[f.ctypes.data if len(f) else None for f in feats])
    op = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    rows = (ctypes.c_int * n)(*[len(f) for f in feats])
    return sea.load().sea_dnn_forward(model._handle, fp, rows, n, op), outs


def test_forward_in_chunks_with_utterances_of_no_row(monkeypatch):
    """utterances of 0, 100, 0, 0, 150, 200, 1, 0, 400 and 0 rows at context 2, whole, at 1 MB and at 0 MB.  A row takes
    256 + 4 * 64 + 8 * 320 = 3072 bytes: 1 MB holds 341 rows, so the cuts fall after 150 and after the 1-row utterance's empty
    neighbour, the 400-row utterance passes the budget alone and is a chunk of its own, and the last chunk has no row (the
    skip path).  Every run equals the model; the rows next to a cut differ from the decoy that splices across utterances."""
    sea = _sea()
    net, feats = L.chain_net(), L.forward_zero_row_feats()
    n = len(feats)
    want, decoy = M.forward(net, feats), M.forward(net, feats, decoy=True)
    model = _device_net(net)
    runs, chunks = {}, {}
    for mb in (None, "1", "0"):
        if mb is None:
            monkeypatch.delenv("SEA_DNN_SCRATCH_MB", raising=False)
        else:
            monkeypatch.setenv("SEA_DNN_SCRATCH_MB", mb)
        rc, outs = _forward_raw(sea, model, feats)
        assert rc == 0, sea.load().sea_last_error()
        runs[mb], chunks[mb] = outs, sea.dnn_last_chunks()
        for u, (f, g, w, d) in enumerate(zip(feats, outs, want, decoy)):
            if len(f) == 0:
                assert np.all(g == SENTINEL), f"budget {mb}: the output of the empty utterance {u} was written"
                continue
            _same(g, w, f"budget {mb} MB, utterance {u} of {len(w)} rows")
            if any(len(x) for x in feats[:u]):
                assert not np.array_equal(g[0], d[0]), f"utterance {u}: the first row equals the decoy's"
            if any(len(x) for x in feats[u + 1:]):
                assert not np.array_equal(g[-1], d[-1]), f"utterance {u}: the last row equals the decoy's"
    print("chunks", chunks)
    assert chunks[None] == 1 and chunks["0"] == n and 1 < chunks["1"] < n
    assert chunks["1"] == 4  # (0, 100, 0, 0, 150), (200, 1, 0), (400), (0)
    for mb in ("1", "0"):
        assert all(np.array_equal(a, b) for a, b in zip(runs[mb], runs[None])), f"the result depends on the cut at {mb} MB"


def test_forward_of_a_list_without_a_row_returns_0_and_writes_nothing(monkeypatch):
    sea = _sea()
    monkeypatch.delenv("SEA_DNN_SCRATCH_MB", raising=False)
    model = _device_net(L.chain_net())
    for n in (1, 3):
        rc, outs = _forward_raw(sea, model, [np.zeros((0, 64), np.float32)] * n)
        assert rc == 0 and all(np.all(o == SENTINEL) for o in outs)
    assert all(o.shape == (0, 64) for o in sea.dnn_forward(model, [np.zeros((0, 64), np.float32)] * 2))


def test_cochleagram_utterances_in_chunks(monkeypatch):
    """the lengths of tests/test_gpu_dnn.py whole, at 1 MB and at 0 MB.  An utterance takes 130 bytes per padded sample and
    256 per row: 1 MB holds the first five, and the three long ones pass it alone -- four chunks."""
    sea = _sea()
    rng = np.random.default_rng(12)
    xs = [rng.integers(-20000, 20000, size=n).astype(np.int16) for n in LENGTHS]
    want = [M.cochleagram(sea.subbband(x)) for x in xs]
    runs, chunks = {}, {}
    for mb in (None, "1", "0"):
        if mb is None:
            monkeypatch.delenv("SEA_DNN_SCRATCH_MB", raising=False)
        else:
            monkeypatch.setenv("SEA_DNN_SCRATCH_MB", mb)
        runs[mb], chunks[mb] = sea.cochleagram_utterances(xs), sea.dnn_last_chunks()
        for x, g, w in zip(xs, runs[mb], want):
            _same(g, w, f"budget {mb} MB, L={x.size}")
    print("chunks", chunks)
    assert chunks[None] == 1 and chunks["0"] == len(xs) and 1 < chunks["1"] < len(xs)
    assert chunks["1"] == 4
    for mb in ("1", "0"):
        assert all(np.array_equal(a, b) for a, b in zip(runs[mb], runs[None])), f"the result depends on the cut at {mb} MB"


# ---- features that are not finite -------------------------------------------------------------------------------------------------
def test_features_that_are_not_finite_stay_within_their_context():
    """one NaN, one +Inf and one -Inf in three rows of the middle utterance of three, context 2, a ReLU and a sigmoid layer.
    Every row farther than 2 rows from a poisoned one, and every row of the other utterances, is bit-equal to the same call
    without the poison and equals the model; the rows within reach have the model's class value for value: a NaN where the
    model has one (payload and sign free), otherwise the model's value (the arithmetic on such values
    is IEEE's in both builds, so sea_dnn_forward accepts them)."""
    sea = _sea()
    net, clean, poisoned, affected = L.poison_case()
    want_clean, want = M.forward(net, clean), M.forward(net, poisoned)
    model = _device_net(net)
    got_clean, got = sea.dnn_forward(model, clean), sea.dnn_forward(model, poisoned)
    for u in range(3):
        _same(got_clean[u], want_clean[u], f"without the poison, utterance {u}")
    for u in (0, 2):
        assert got[u].tobytes() == got_clean[u].tobytes(), f"utterance {u} depends on its neighbour's poison"
        _same(got[u], want[u], f"with the poison, utterance {u}")
    assert got[1][~affected].tobytes() == got_clean[1][~affected].tobytes(), "a row out of reach of the poison changed"
    _same(got[1][~affected], want[1][~affected], "with the poison, the rows out of reach")
    differ = L.class_differences(got[1][affected], want[1][affected])
    nans = int(np.isnan(want[1][affected]).sum())
    print(f"with the poison, the rows within reach: {want[1][affected].size} values ({nans} NaN in the model), {differ} differ in class")
    assert differ == 0
