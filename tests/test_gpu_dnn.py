"""The DNN mask estimator on the GPU, every comparison bit for bit as values against the plain-C
model of tests/dnn_model.py: the MFMA lane map on exact integers, the order of the sums on floats spread over 2^12, the splice
at utterance boundaries, the cochleagram (host form and batch path, padding poisoned), and the chain from noisy to enhanced
audio against its composition, whole and in chunks."""
import ctypes

import numpy as np
import pytest

from tests import dnn_model as M

pytestmark = pytest.mark.gpu


def _sea():
    import speech_enhancement_amd as sea
    return sea


def _device_net(net):
    return _sea().DnnMask(net.context, net.shift, net.scale, net.weights, net.biases, net.acts)


def _same(got, want, what):
    differ = int(np.sum(got != want))
    print(f"{what}: {got.size} values, {differ} differ" + (f", largest |delta| {np.nanmax(np.abs(got - want)):.3g}" if differ else ""))
    assert got.shape == want.shape and np.all(np.isfinite(want)), what
    assert np.array_equal(got, want), what  # as values: -0 equals +0


# ---- the lane map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context,block", [(0, 0), (1, 0), (1, 1), (1, 2)])
def test_lane_map_on_exact_integers(context, block):
    """identity activations, one-hot input rows (times a small factor that tells the 200 rows apart), the asymmetric
    W[j][k] = 3 j + 7 k + 1 and b[j] = j: every sum is exact in small integers, so the output is the integer product whatever the
    order -- a swapped row and column, a wrong k half or a misplaced K tile shows here.  At context 1 the scale is 1 in one
    64-wide block of the 192 inputs and 0 elsewhere, which walks the hot k through all six K tiles."""
    sea = _sea()
    k0, n_out, rows = 64 * (2 * context + 1), 130, 200
    j, k = np.arange(n_out)[:, None], np.arange(k0)[None, :]
    scale = np.zeros(k0, np.float32)
    scale[64 * block:64 * block + 64] = 1
    net = M.make_net(context, np.zeros(k0), scale, [3 * j + 7 * k + 1], [np.arange(n_out)], [0])
    feats = np.zeros((rows, 64), np.float32)
    feats[np.arange(rows), np.arange(rows) % 64] = 1 + np.arange(rows) // 64
    x0 = M.splice_numpy(net, feats).astype(np.int64)
    assert np.all((x0 != 0).sum(axis=1) == 1)
    want = (x0 @ net.weights[0].astype(np.int64).T + np.arange(n_out)[None, :]).astype(np.float32)
    model = _device_net(net)
    got = sea.dnn_forward(model, [feats])[0]
    _same(got, want, f"lane map, context {context}, block {block}")
    assert np.array_equal(M.forward(net, [feats])[0], want)  # and the C model agrees with the integers


# ---- the order of the sums --------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 31, 32, 33, 127, 128, 129, 300)
CONTEXTS = (0, 1, 5)
NETS = (((1,), (0,)), ((3,), (1,)), ((33, 64), (2, 1)), ((64,), (2,)), ((130, 3), (1, 0)), ((260, 33, 64), (1, 2, 1)),
        ((260, 130, 64, 33), (2, 2, 0, 1)), ((64, 260), (0, 1)), ((33, 1, 3), (1, 1, 2)))


@pytest.mark.parametrize("context", CONTEXTS)
@pytest.mark.parametrize("rows", ROWS)
def test_forward_equals_the_c_model_where_order_matters(context, rows):
    """floats of either sign over a magnitude range of 2^12 (weights, biases, shift, scale), a denormal weight and a denormal
    input: a sum in another order, a split K, a fused shift and scale or a flushed denormal gives other bits.  Every context
    meets all nine networks (widths 1, 3, 33, 64, 130, 260; one to four layers; every activation), every row count three."""
    sea = _sea()
    widths, acts = NETS[(ROWS.index(rows) + 3 * CONTEXTS.index(context)) % len(NETS)]
    net = M.random_net(1000 * context + rows, context, widths, acts)
    centre = 64 * context  # the input (d = 0, c = 0): unshifted and unscaled, so that a denormal feature stays one
    net.shift[centre], net.scale[centre] = 0.0, 1.0
    net.weights[0][0, 0] = np.float32(1e-40)
    rng = np.random.default_rng(rows)
    cut = rows // 3
    feats = [f for f in (rng.uniform(0, 27, size=(cut, 64)), rng.uniform(0, 27, size=(rows - cut, 64))) if len(f)]
    feats = [f.astype(np.float32) for f in feats]
    feats[0][0, 0] = np.float32(1e-41)
    want = M.forward(net, feats)
    model = _device_net(net)
    got = sea.dnn_forward(model, feats)
    for u, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"context {context}, {rows} rows, {widths} {acts}, utterance {u}")


def test_denormal_products_and_sums_come_through():
    """weights of 1e-40 on inputs of 1 (every product and the sum are denormal) and inputs of 1e-41 on weights of 1024"""
    sea = _sea()
    w = np.stack([np.full(64, 1e-40), np.full(64, 1024.0), M.wide_floats(np.random.default_rng(0), 64)]).astype(np.float32)
    net = M.make_net(0, np.zeros(64), np.ones(64), [w], [np.zeros(3)], [0])
    feats = np.stack([np.ones(64), np.full(64, 1e-41), np.full(64, 3e-39)]).astype(np.float32)
    want = M.forward(net, [feats])[0]
    assert 0 < want[0, 0] < 1e-38 and want[1, 1] > 1e-38 and want[1, 0] == 0
    _same(sea.dnn_forward(_device_net(net), [feats])[0], want, "denormals")


# ---- the splice -------------------------------------------------------------------------------------------------------------------
def test_splice_at_utterance_boundaries():
    """one call, context 5, utterances of 1, 2, 2 C, 2 C + 1 and 17 rows: the rows next to a boundary equal the model and differ
    from the decoy that splices across it"""
    sea = _sea()
    C = 5
    net = M.random_net(55, C, (33, 64), (1, 1), spread=2)
    rng = np.random.default_rng(55)
    net.shift[:] = rng.uniform(-14, -12, size=net.shift.size).astype(np.float32)
    net.scale[:] = rng.uniform(0.05, 0.15, size=net.scale.size).astype(np.float32)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (1, 2, 2 * C, 2 * C + 1, 17)]
    want, decoy = M.forward(net, feats), M.forward(net, feats, decoy=True)
    got = sea.dnn_forward(_device_net(net), feats)
    for u, (g, w, d) in enumerate(zip(got, want, decoy)):
        _same(g, w, f"splice, utterance {u} of {len(w)} rows")
        if u > 0:
            assert not np.array_equal(g[0], d[0]), f"utterance {u}: the first row equals the decoy's"
        if u < len(feats) - 1:
            assert not np.array_equal(g[-1], d[-1]), f"utterance {u}: the last row equals the decoy's"


# ---- the cochleagram --------------------------------------------------------------------------------------------------------------
# the contract's lengths (one frame; L % 8 != 0; a second frame; 16 frames + 5 samples; 17 frames + 5) and this kernel's own
# edges: a wave's tile is 63 frames and a workgroup has four waves -- 63, 64 and 253 frames
LENGTHS = (320, 479, 480, 2725, 2885, 10240, 10405, 40645)


def _streams(kind, L, rng):
    if kind == "square":
        return np.where((np.arange(L)[None, :] // (1 + np.arange(64)[:, None])) % 2 == 0, -32768, 32767).astype(np.int16)
    if kind == "lowest":
        return np.full((64, L), -32768, np.int16)
    if kind == "silence":
        return np.zeros((64, L), np.int16)
    return rng.integers(-32768, 32768, size=(64, L)).astype(np.int16)


@pytest.mark.parametrize("L", LENGTHS)
def test_cochleagram_host_form_equals_the_model_and_ignores_the_padding(L, monkeypatch):
    sea = _sea()
    rng = np.random.default_rng(L)
    for kind in ("square", "lowest", "silence", "random"):
        sub = _streams(kind, L, rng)
        want = M.cochleagram(sub)
        assert want.shape == ((L - 320) // 160 + 1, 64)
        for fill in (None, "-32768", "12345"):  # what the padding of every channel row holds on the device
            if fill is None:
                monkeypatch.delenv("SEA_DNN_PAD_FILL", raising=False)
            else:
                monkeypatch.setenv("SEA_DNN_PAD_FILL", fill)
            _same(sea.cochleagram(sub), want, f"cochleagram {kind} L={L} padding {fill}")
        if kind == "silence":
            assert not want.any()
        if kind == "lowest":
            assert np.all(want == M.lnf(np.float32([320 * 2.0 ** 30 + 1]))[0])


def test_cochleagram_batch_path_equals_the_host_form_and_the_model():
    sea = _sea()
    rng = np.random.default_rng(11)
    xs = [rng.integers(-20000, 20000, size=L).astype(np.int16) for L in LENGTHS]
    xs[1][:] = 0  # silent audio (its subband streams are not: the hair cell model rests at a constant)
    got = sea.cochleagram_utterances(xs)
    for x, g in zip(xs, got):
        sub = sea.subbband(x)
        _same(g, M.cochleagram(sub), f"batch path L={x.size}")
        assert np.array_equal(g, sea.cochleagram(sub))


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def _resynth_utterances(sea, xs, masks, binary):
    lib = sea.load()
    n = len(xs)
    outs = [np.zeros(x.size, np.int16) for x in xs]
    ptrs = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])  # noqa: E731
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    assert lib.sea_resynth_utterances(ptrs(xs), lens, ptrs(masks), binary, ptrs(outs), n) == 0, lib.sea_last_error()
    return outs


@pytest.fixture(scope="module")
def chain():
    sea = _sea()
    rng = np.random.default_rng(21)
    net = M.random_net(21, 2, (96, 64), (1, 1), spread=2)
    net.shift[:] = rng.uniform(-11, -9, size=net.shift.size).astype(np.float32)
    net.scale[:] = rng.uniform(0.05, 0.15, size=net.scale.size).astype(np.float32)
    xs = [(8000 * np.sin(np.arange(L) * (0.05 + 0.01 * i)) + rng.integers(-3000, 3000, size=L)).astype(np.int16)
          for i, L in enumerate((320, 479, 1600, 2725, 4000, 8000, 16000))]
    model = _device_net(net)
    feats = sea.cochleagram_utterances(xs)
    masks = sea.dnn_forward(model, feats)
    want_masks = M.forward(net, [M.cochleagram(sea.subbband(x)) for x in xs])
    return dict(net=net, model=model, xs=xs, masks=masks, want_masks=want_masks)


@pytest.mark.parametrize("binary", [False, True])
def test_chain_equals_its_composition(chain, binary, monkeypatch):
    sea = _sea()
    monkeypatch.delenv("SEA_DNN_SCRATCH_MB", raising=False)
    xs, masks = chain["xs"], chain["masks"]
    for m, w in zip(masks, chain["want_masks"]):
        _same(m, w, "the composition's mask against the model")
        assert 0.01 < m.mean() < 0.99 and (m > 0.5).any() and (m < 0.5).any()
    want = _resynth_utterances(sea, xs, masks, int(binary))
    audio, got_masks = sea.dnn_enhance_utterances(chain["model"], xs, binary=binary, masks=True)
    assert sea.dnn_last_chunks() == 1
    for u, x in enumerate(xs):
        _same(got_masks[u], masks[u], f"chain mask, utterance {u}")
        _same(audio[u], want[u], f"chain audio, utterance {u} ({x.size} samples, binary {binary})")
    assert any(a.any() for a in audio)
    # the same in chunks: 3 MB holds the first four utterances, then one utterance each
    monkeypatch.setenv("SEA_DNN_SCRATCH_MB", "3")
    audio3, masks3 = sea.dnn_enhance_utterances(chain["model"], xs, binary=binary, masks=True)
    chunks = sea.dnn_last_chunks()
    print("chunks", chunks)
    assert chunks >= 3
    for u in range(len(xs)):
        assert np.array_equal(audio3[u], audio[u]) and np.array_equal(masks3[u], got_masks[u]), f"utterance {u} depends on the cut"
    assert all(np.array_equal(a, b) for a, b in zip(sea.dnn_enhance_utterances(chain["model"], xs, binary=binary), audio))


def test_chain_refuses_a_short_utterance_and_writes_nothing(chain):
    sea = _sea()
    lib = sea.load()
    xs = list(chain["xs"][:3]) + [np.ones(319, np.int16)] + [chain["xs"][3]]
    n = len(xs)
    outs = [np.full(x.size, 777, np.int16) for x in xs]
    ms = [np.full((max((x.size - 320) // 160 + 1, 1), 64), 7.0, np.float32) for x in xs]
    ptrs = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])  # noqa: E731
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    assert lib.sea_dnn_enhance_utterances(chain["model"]._handle, ptrs(xs), lens, n, 0, ptrs(outs), ptrs(ms)) != 0
    assert b"319" in lib.sea_last_error()
    assert all(np.all(o == 777) for o in outs) and all(np.all(m == 7.0) for m in ms)
    with pytest.raises(sea.SeaError):
        sea.dnn_enhance_utterances(chain["model"], xs)
    with pytest.raises(sea.SeaError):
        sea.cochleagram_utterances(xs)
    # bit 1 of binary selects L / 160 mask rows: refused; so is a network whose output is not a mask row
    assert lib.sea_dnn_enhance_utterances(chain["model"]._handle, ptrs(xs), lens, 3, 2, ptrs(outs), None) != 0
    narrow = M.random_net(1, 0, (8,), (1,))
    with pytest.raises(sea.SeaError):
        sea.dnn_enhance_utterances(_device_net(narrow), chain["xs"][:1])
