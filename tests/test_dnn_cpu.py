"""The DNN mask estimator without a GPU: the accuracy of the two elementary functions of
csrc/dnn_math.h over every argument that can occur, the cochleagram model against a brute-force integer sum, the plain-C
model of the network (tests/dnn_model_driver.c) against an independent float64 torch model within a bound computed from the
weights, and the new symbols and their refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import dnn_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_dnn_create", "sea_dnn_destroy", "sea_cochleagram64", "sea_cochleagram_utterances", "sea_dnn_forward",
               "sea_dnn_enhance_utterances", "sea_dnn_last_chunks", "sea_dnn_last_stage_ms")


# ---- csrc/dnn_math.h ------------------------------------------------------------------------------------------------------------
def test_lnf_is_within_two_ulps_on_every_float_of_its_domain():
    """every float of [1, 2^39] (39 x 2^23 + 1 of them) against the double log; the cochleagram's argument is 1 + an energy of
    at most 320 x 2^30 < 2^39.  Measured: 0.835 ulps, at 0x1.67cc32p+0."""
    r = M.sweep("lnf_sweep")
    print(f"sea_lnf: {int(r['n'])} arguments, largest error {r['max_ulp']:.6f} ulps at {r['max_ulp_at']}")
    assert r["n"] == 39 * 2 ** 23 + 1
    assert r["max_ulp"] <= 2.0


def test_sigmoid_and_exponential_accuracy_on_every_float_of_the_range():
    """every float z of [-20, 20] (zeros and subnormals included) and a stride of 0.001 through [-88, 88], +-88 and +-100 (the
    clamp).  The exponential is asked for 2^-23 relative (1 ulp) wherever its value is a normal float; exp (-88) = 6.05e-39 is
    subnormal, where one rounding costs up to half a unit of 2^-149 and the bound is 1 such unit.  The sigmoid's bound follows:
    d = 1 + e carries the exponential's error and one rounding, the quotient one more, and |d sigma / d e| = sigma^2 <= 1 with
    e sigma^2 <= 1/4: at most 2^-23 / 4 + 2^-24 + 2^-24 < 2^-22.  Measured: sigmoid 8.93e-8, exponential 7.66e-8 relative,
    0.74 units where subnormal."""
    r = M.sweep("exp_sweep")
    print(f"sigmoid: {int(r['n'])} arguments, |float - double| <= {r['sigmoid_abs']:.4g} at {r['sigmoid_abs_at']}; exponential: "
          f"relative {r['exp_rel']:.4g} at {r['exp_rel_at']}, {r['exp_subnormal_ulps']:.3f} units of 2^-149 where subnormal")
    assert r["n"] >= 2 * (np.float32(20.0).view(np.uint32) + 1) + 176001
    assert r["exp_rel"] <= 2.0 ** -23
    assert r["exp_subnormal_ulps"] <= 1.0
    assert r["sigmoid_abs"] <= M.SIGMOID_ABS == 2.0 ** -22


def test_the_functions_edge_values():
    assert M.lnf(np.float32([1.0]))[0] == 0.0  # silence: E = 0 gives a feature of exactly 0
    z = np.float32([-200.0, -88.0, 0.0, -0.0, 88.0, 200.0, np.inf, -np.inf])
    s = M.act(z, 1)
    assert s[0] == s[1] and s[4] == s[5] == s[6] == 1.0 and s[2] == s[3] == 0.5 and s[7] == s[0] and 0 < s[0] < 1e-38
    assert np.array_equal(M.act(np.float32([-1.5, -0.0, 0.0, 2.5]), 2), np.float32([0, 0, 0, 2.5]))
    assert np.array_equal(M.act(z[:6], 0), z[:6])


# ---- the cochleagram model --------------------------------------------------------------------------------------------------------
def _brute_energy(sub64):
    L = sub64.shape[1]
    F = (L - 320) // 160 + 1
    return [[sum(int(v) * int(v) for v in sub64[c, 160 * f:160 * f + 320]) for c in range(64)] for f in range(F)]


@pytest.mark.parametrize("kind", ["square", "lowest", "silence", "random"])
def test_cochleagram_model_against_python_integers(kind):
    L = 805
    rng = np.random.default_rng(5)
    if kind == "square":  # between the two ends of int16
        sub = np.where((np.arange(L)[None, :] // (1 + np.arange(64)[:, None])) % 2 == 0, -32768, 32767).astype(np.int16)
    elif kind == "lowest":  # the largest energy there is: 320 x 2^30
        sub = np.full((64, L), -32768, np.int16)
    elif kind == "silence":
        sub = np.zeros((64, L), np.int16)
    else:
        sub = rng.integers(-32768, 32768, size=(64, L)).astype(np.int16)
    brute = _brute_energy(sub)
    E = M.frame_energies(sub)
    assert E.shape == (4, 64) and E.tolist() == brute
    feats = M.cochleagram(sub)
    if kind == "lowest":
        assert E.max() == 320 * 2 ** 30
    if kind == "silence":
        assert np.array_equal(feats, np.zeros((4, 64), np.float32))
    else:
        y = np.array([[np.float32(e + 1) for e in row] for row in brute], np.float32)  # Python's int -> float32 rounds to nearest
        want = np.log(y.astype(np.float64))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(feats.astype(np.float64) - want) <= 2 * ulp)


# ---- the C model of the network against float64 torch ---------------------------------------------------------------------------
@pytest.mark.parametrize("context,widths,acts", [(0, (33,), (0,)), (1, (130, 64), (1, 1)), (5, (260, 33, 64), (2, 1, 0)),
                                                 (2, (64, 64, 64, 3), (1, 2, 0, 1))])
def test_c_model_against_float64_torch(context, widths, acts):
    """the bound is computed from the weights (tests/dnn_model.py::torch_float64 derives it) and printed, not chosen"""
    net = M.random_net(100 + context, context, widths, acts, spread=2)
    rng = np.random.default_rng(7)
    # inputs centred and scaled to a few units, as a trained network's normalisation leaves them, so that no sigmoid saturates
    # and the bound stays near the rounding level of every layer
    net.shift[:] = rng.uniform(-14, -12, size=net.shift.size).astype(np.float32)
    net.scale[:] = rng.uniform(0.05, 0.15, size=net.scale.size).astype(np.float32)
    feats = [rng.uniform(0, 26.5, size=(F, 64)).astype(np.float32) for F in (1, 2 * context + 3, 9)]  # ln (2^39) < 27.04
    got = M.forward(net, feats)
    for u, f in enumerate(feats):
        x0 = M.splice_numpy(net, f)
        want, bound = M.torch_float64(net, x0)
        err = np.abs(got[u].astype(np.float64) - want)
        i = np.unravel_index(np.argmax(err / bound), err.shape)
        print(f"C={context} {widths} utterance {u}: largest error {err.max():.3g}, bound there {bound[i]:.3g}, "
              f"largest error / bound {(err / bound).max():.3g}, bounds {bound.min():.3g} .. {bound.max():.3g}")
        assert got[u].shape == want.shape and np.all(np.isfinite(want))
        assert np.all(err <= bound)


def test_c_model_is_clean_under_the_sanitizers():
    """the same driver at -O1 with -fsanitize=address,undefined gives the same bits (a stand-alone program; nothing is loaded
    into python)"""
    net = M.random_net(3, 1, (33, 5), (1, 2))
    rng = np.random.default_rng(1)
    feats = [rng.uniform(0, 26, size=(F, 64)).astype(np.float32) for F in (1, 4)]
    a, b = M.forward(net, feats), M.forward(net, feats, sanitize=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    d = M.forward(net, feats, decoy=True)
    assert not np.array_equal(d[0], a[0]) and not np.array_equal(d[1][:1], a[1][:1]) and np.array_equal(d[1][1:], a[1][1:])


# ---- symbols and refusals ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_bound_and_built_and_none_takes_a_stream():
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import _lib
    from tests import stream_cases as S
    raw = ctypes.CDLL(sea.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype"
        assert f"{name}(" in header, f"{name} is not declared in include/sea_mi355x.h"
        assert not re.search(name + r"\([^;]*\bstream\b[^;]*\);", header), f"{name} takes a stream"
    assert len(S.stream_prototypes()) == 44
    blob = open(sea.LIB_PATH, "rb").read()
    for kernel in (b"cochleagram64_kernel", b"dnn_layer_kernel", b"dnn_splice_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    for name in ("DnnMask", "cochleagram", "cochleagram_utterances", "dnn_forward", "dnn_enhance_utterances", "dnn_last_chunks"):
        assert callable(getattr(sea, name))
    makefile = open(os.path.join(ROOT, "speech_enhancement_amd", "csrc", "Makefile")).read()
    assert "dnn_kernel.hip" in makefile and "dnn_capi.hip" in makefile and "dnn_math.h" in makefile


def test_from_torch_refuses_other_modules():
    import torch.nn as nn
    import speech_enhancement_amd as sea
    shift, scale = np.zeros(64, np.float32), np.ones(64, np.float32)
    for bad in (nn.Sequential(nn.Linear(64, 8), nn.Tanh()), nn.Sequential(nn.Linear(64, 8), nn.Dropout(0.1), nn.Linear(8, 64)),
                nn.Sequential(nn.Sigmoid(), nn.Linear(64, 8)), nn.Sequential(nn.Linear(64, 8, bias=False)), nn.Linear(64, 64),
                nn.Sequential(nn.Linear(64, 8), nn.ReLU(), nn.Sigmoid())):
        with pytest.raises(TypeError):
            sea.DnnMask.from_torch(bad, 0, shift, scale)


def _create(lib, context, dims, weights, biases, acts, shift=None, scale=None):
    k0 = dims[0]
    shift = np.zeros(k0, np.float32) if shift is None else shift
    scale = np.ones(k0, np.float32) if scale is None else scale
    n = len(weights)
    pw = (ctypes.c_void_p * n)(*[w.ctypes.data for w in weights])
    pb = (ctypes.c_void_p * n)(*[b.ctypes.data for b in biases])
    return lib.sea_dnn_create(context, shift.ctypes.data_as(ctypes.c_void_p), scale.ctypes.data_as(ctypes.c_void_p), n,
                              (ctypes.c_int * (n + 1))(*dims), pw, pb, (ctypes.c_int * n)(*acts))


def test_creation_refuses_what_the_header_says_before_any_device_is_touched():
    import speech_enhancement_amd as sea
    lib = sea.load()
    w, b = np.ones((8, 64), np.float32), np.zeros(8, np.float32)
    cases = {
        "a NaN weight": lambda: _create(lib, 0, [64, 8], [np.where(np.eye(8, 64) > 0, np.nan, w).astype(np.float32)], [b], [1]),
        "an infinite bias": lambda: _create(lib, 0, [64, 8], [w], [np.full(8, np.inf, np.float32)], [1]),
        "a NaN shift": lambda: _create(lib, 0, [64, 8], [w], [b], [1], shift=np.full(64, np.nan, np.float32)),
        "dims[0] != K0": lambda: _create(lib, 1, [64, 8], [w], [b], [1], shift=np.zeros(192, np.float32), scale=np.ones(192, np.float32)),
        "context > 15": lambda: _create(lib, 16, [64 * 33, 8], [np.ones((8, 64 * 33), np.float32)], [b], [1]),
        "an unknown activation": lambda: _create(lib, 0, [64, 8], [w], [b], [3]),
        "a dimension above 4096": lambda: _create(lib, 0, [64, 4097], [np.ones((4097, 64), np.float32)], [np.zeros(4097, np.float32)], [0]),
    }
    for what, call in cases.items():
        assert not call(), f"{what} was accepted"
        assert lib.sea_last_error(), what
    with pytest.raises(sea.SeaError):
        sea.DnnMask(0, np.zeros(64), np.ones(64), [np.full((8, 64), np.nan)], [np.zeros(8)], ["sigmoid"])
    with pytest.raises(ValueError):
        sea.DnnMask(1, np.zeros(64), np.ones(64), [w], [b], [1])  # shift and scale of the wrong context


def test_save_and_load_keep_the_network(tmp_path, monkeypatch):
    """the file holds what the constructor takes (the constructor itself is replaced: it would need a device)"""
    import speech_enhancement_amd as sea
    kept = {}
    monkeypatch.setattr(sea.DnnMask, "__init__", lambda self, *a: kept.update(args=a) or setattr(self, "_handle", None))
    net = M.random_net(9, 1, (5, 64), (2, 1))
    m = sea.DnnMask.__new__(sea.DnnMask)
    m.context, m.shift, m.scale, m.weights, m.biases, m.acts, m._handle = 1, net.shift, net.scale, net.weights, net.biases, net.acts, None
    m.save(tmp_path / "net.npz")
    sea.DnnMask.load(tmp_path / "net.npz")
    c, sh, sc, ws, bs, acts = kept["args"]
    assert c == 1 and np.array_equal(sh, net.shift) and np.array_equal(sc, net.scale) and acts == net.acts
    assert all(np.array_equal(a, b) for a, b in zip(ws + bs, net.weights + net.biases))
