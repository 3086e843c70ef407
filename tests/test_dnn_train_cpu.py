"""The DNN mask estimator's trainer without a GPU: the formulae against torch autograd, the plain-C
model (tests/dnn_train_model_driver.c) against their float64 restatement within a bound carried value by value, the proof that
the GPU test's inputs are order-sensitive and dense, the driver under the sanitizers, the new symbols, the refusals and
DnnMask.normaliser."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import dnn_model as M
from tests import dnn_train_model as T

ROOT = M.ROOT
HEADER = os.path.join(ROOT, "include", "sea_mi355x.h")
NEW_SYMBOLS = ("sea_dnn_trainer_create", "sea_dnn_trainer_destroy", "sea_dnn_trainer_run", "sea_dnn_trainer_read", "sea_dnn_get_params",
               "sea_dnn_trainer_stage_ms")
BIG_CASES = [(c, r) for c in T.CONTEXTS for r in T.ROWS if r >= 31]


def _small_case(context, widths, acts, rows, seed):
    net = T.dense_net(seed, context, widths, acts)
    rng = np.random.default_rng(seed)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (rows - 5, 5)]
    targets = [rng.uniform(0, 1, size=(F, widths[-1])).astype(np.float32) for F in (rows - 5, 5)]
    return net, feats, targets


# ---- the formulae -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context,widths,acts", [(0, (33,), (0,)), (1, (130, 64), (1, 1)), (2, (64, 33, 64, 3), (2, 1, 0, 1))])
def test_formulae_equal_torch_autograd(context, widths, acts):
    """step_float64 -- delta_n = e d(y), G = delta^T a, g = the column sums, delta_(l-1) = (delta W) d(a), v = mu v + g,
    w = w - eta v -- against torch float64 autograd of 0.5 * ((net (x) - t)**2).sum () and torch.optim.SGD with momentum over
    two steps (the second has a momentum that is not zero).  Both are float64 sums of at most 320 terms in different orders:
    1e-12 of the tensor's largest magnitude is a thousand times their rounding level."""
    import torch
    import torch.nn as nn
    net, feats, targets = _small_case(context, widths, acts, 23, 11)
    x0 = np.concatenate([M.splice_numpy(net, f) for f in feats])
    t = np.concatenate(targets)
    eta, mu = 2.0 ** -12, 0.9
    layers = []
    for w, b, a in zip(net.weights, net.biases, net.acts):
        lin = nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.astype(np.float64)))
            lin.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        layers.append(lin)
        if a:
            layers.append(nn.Sigmoid() if a == 1 else nn.ReLU())
    seq = nn.Sequential(*layers)
    opt = torch.optim.SGD(seq.parameters(), lr=eta, momentum=mu)
    linears = [m for m in seq if isinstance(m, nn.Linear)]
    W, b, vw, vb = [w.astype(np.float64) for w in net.weights], [v.astype(np.float64) for v in net.biases], None, None
    for step in range(2):
        opt.zero_grad()
        loss = 0.5 * ((seq(torch.from_numpy(x0.astype(np.float64))) - torch.from_numpy(t.astype(np.float64))) ** 2).sum()
        loss.backward()
        s = T.step_float64(W, b, net.acts, x0, t, eta, mu, vw, vb)
        close = lambda got, want: np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)  # noqa: E731
        assert close(np.float64(s.loss), np.float64(loss.item()))
        for l, lin in enumerate(linears):
            assert close(s.G[l + 1], lin.weight.grad.numpy()) and close(s.g[l + 1], lin.bias.grad.numpy()), (step, l)
        opt.step()
        for l, lin in enumerate(linears):
            assert close(s.weights[l], lin.weight.detach().numpy()) and close(s.biases[l], lin.bias.detach().numpy()), (step, l)
        W, b, vw, vb = s.weights, s.biases, s.vw, s.vb
    assert np.abs(vw[0] - s.G[1]).max() > 0  # the second step's momentum was not its gradient alone


# ---- the float model against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context,widths,acts", [(0, (33,), (0,)), (1, (130, 64), (1, 1)), (5, (260, 33, 64), (2, 1, 0)),
                                                 (2, (64, 64, 64, 3), (1, 2, 0, 1))])
def test_c_model_against_float64(context, widths, acts):
    """one step of the float C model against step_float64, every stage within the bound step_float64 derives (its docstring)
    and computes from the values; the largest ratio is printed, nothing is chosen"""
    net, feats, targets = _small_case(context, widths, acts, 37, 100 + context)
    order = np.random.default_rng(context).permutation(37)
    eta, mu = np.float32(2.0 ** -12), np.float32(0.9)
    r = T.train(net, feats, targets, order, 37, eta, mu)
    x0 = np.concatenate([M.splice_numpy(net, f) for f in feats])[order]
    assert np.array_equal(r.act[0], x0)
    s = T.step_float64(net.weights, net.biases, net.acts, x0, np.concatenate(targets)[order], eta, mu)
    n, worst = len(widths), {}

    def within(name, got, want, bound):
        err = np.abs(np.asarray(got, np.float64) - want)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert np.all(np.isfinite(want)) and np.all(err <= bound), f"{name}: error / bound {ratio:.3g}"

    within("loss", r.losses[0], s.loss, s.e_loss)
    for l in range(1, n + 1):
        within("a", r.act[l], s.act[l], s.e_act[l])
        within("delta", r.delta[l], s.delta[l], s.e_delta[l])
        within("G", r.G[l], s.G[l], s.e_G[l])
        within("g", r.g[l], s.g[l], s.e_g[l])
        within("v", r.vw[l - 1], s.vw[l - 1], s.e_vw[l - 1])
        within("W", r.weights[l - 1], s.weights[l - 1], s.e_weights[l - 1])
        within("b", r.biases[l - 1], s.biases[l - 1], s.e_biases[l - 1])
    print(f"C={context} {widths} {acts}: largest error / bound per stage", {k: f"{v:.3g}" for k, v in worst.items()})


# ---- the GPU test's inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context,rows", BIG_CASES)
def test_decoy_differs_and_the_inputs_are_dense(context, rows):
    """on every case with B >= 31 of tests/test_gpu_dnn_train.py's order test the decoy (G summed over m descending, E over j
    descending) differs from the model in at least one value: those inputs tell the order of the sums.  And the density caps
    hold on them: at most 5 % of a sigmoid or identity layer's delta exactly zero, at most 75 % of a ReLU layer's, all finite."""
    zeros = T.check_density(context, rows)
    r, d = T.order_case_model(context, rows), T.order_case_model(context, rows, True)
    n = len(r.weights)
    differ_G = sum(int(np.sum(r.G[l] != d.G[l])) for l in range(1, n + 1))
    differ_delta = sum(int(np.sum(r.delta[l] != d.delta[l])) for l in range(1, n))
    print(f"context {context}, B {rows}: zero deltas {['%.3f' % z for z in zeros]}, decoy: {differ_G} values of G, {differ_delta} of delta differ")
    assert differ_G > 0


def test_density_holds_on_the_small_cases_too():
    for context in T.CONTEXTS:
        for rows in (1, 2):
            T.check_density(context, rows)
    r = T.order_case_model(0, 1)
    assert np.any((np.abs(r.G[1]) > 0) & (np.abs(r.G[1]) < 1e-38))  # the denormal input's product is a value of G_1 at B = 1


def test_driver_is_clean_under_the_sanitizers():
    """the same driver at -O1 with -fsanitize=address,undefined gives the same bits (a stand-alone program; nothing is loaded
    into python)"""
    c = T.order_case(1, 33)
    plain = T.order_case_model(1, 33)
    checked = T.train(c.net, c.feats, c.targets, c.order, c.batch, c.eta, c.mu, sanitize=True)
    for name in ("weights", "biases", "vw", "vb", "act"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(getattr(plain, name), getattr(checked, name))), name
    for name in ("delta", "G", "g"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(getattr(plain, name)[1:], getattr(checked, name)[1:])), name
    assert plain.losses.tobytes() == checked.losses.tobytes()
    short = T.train(c.net, c.feats, c.targets, c.order[:40], 33, c.eta, c.mu, update=False, sanitize=True)  # a short last minibatch
    assert short.last_batch == 7 and all(w.tobytes() == v.tobytes() for w, v in zip(short.weights, c.net.weights))


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
    for kernel in (b"dnn_gather_splice_kernel", b"dnn_delta_out_kernel", b"dnn_loss_kernel", b"dnn_dgrad_kernel", b"dnn_wgrad_kernel",
                   b"dnn_sgd_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
    assert callable(sea.DnnTrainer) and callable(sea.DnnMask.pull) and callable(sea.DnnMask.normaliser)
    for name in ("run", "epoch", "evaluate", "read", "close"):
        assert callable(getattr(sea.DnnTrainer, name))
    makefile = open(os.path.join(ROOT, "speech_enhancement_amd", "csrc", "Makefile")).read()
    assert "dnn_train_kernel.hip" in makefile and "dnn_train_capi.hip" in makefile and "dnn_train_kernels.h" in makefile


def test_refusals_come_before_any_device_is_touched():
    """null arguments, batch and max_batch outside 1..4096, n_order < 1, eta or mu outside the contract, an unknown what: all
    return non-zero with a message where there is no device at all.  The checks that need only the arguments come before any
    use of the handle, so a handle that is never read stands in for a trainer here; the refusals that need a real trainer
    (batch > max_batch, an index outside the set, a layer that does not exist) are in tests/test_gpu_dnn_train.py."""
    import speech_enhancement_amd as sea
    lib = sea.load()
    stand_in = ctypes.create_string_buffer(4096)  # never read: every call below is refused on its arguments alone
    handle = ctypes.cast(stand_in, ctypes.c_void_p)
    order = np.zeros(4, np.int64)
    losses = np.zeros(4, np.float64)
    po, pl = order.ctypes.data_as(ctypes.c_void_p), losses.ctypes.data_as(ctypes.c_void_p)
    feats, targets = np.zeros((4, 64), np.float32), np.zeros((4, 64), np.float32)
    pf, pt = (ctypes.c_void_p * 1)(feats.ctypes.data), (ctypes.c_void_p * 1)(targets.ctypes.data)
    rows, bad_rows = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(-1)
    nan, inf = float("nan"), float("inf")
    cases = {
        "run: a null trainer": lambda: lib.sea_dnn_trainer_run(None, po, 4, 2, 0.1, 0.0, 1, pl),
        "run: a null order": lambda: lib.sea_dnn_trainer_run(handle, None, 4, 2, 0.1, 0.0, 1, pl),
        "run: null losses": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, 0.1, 0.0, 1, None),
        "run: batch 0": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 0, 0.1, 0.0, 1, pl),
        "run: batch 4097": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 4097, 0.1, 0.0, 1, pl),
        "run: n_order 0": lambda: lib.sea_dnn_trainer_run(handle, po, 0, 2, 0.1, 0.0, 1, pl),
        "run: eta NaN": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, nan, 0.0, 1, pl),
        "run: eta infinite": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, inf, 0.0, 1, pl),
        "run: mu NaN": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, 0.1, nan, 1, pl),
        "run: mu 1": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, 0.1, 1.0, 1, pl),
        "run: mu negative": lambda: lib.sea_dnn_trainer_run(handle, po, 4, 2, 0.1, -0.1, 1, pl),
        "read: a null trainer": lambda: lib.sea_dnn_trainer_read(None, 0, 0, pl),
        "read: a null output": lambda: lib.sea_dnn_trainer_read(handle, 0, 0, None),
        "get_params: a null model": lambda: lib.sea_dnn_get_params(None, pf, pt),
        "get_params: null arrays": lambda: lib.sea_dnn_get_params(handle, None, None),
    }
    for what, call in cases.items():
        assert call() != 0, f"{what} was accepted"
        assert lib.sea_last_error(), what
    creations = {
        "create: a null model": lambda: lib.sea_dnn_trainer_create(None, pf, pt, rows, 1, 4),
        "create: null features": lambda: lib.sea_dnn_trainer_create(handle, None, pt, rows, 1, 4),
        "create: null targets": lambda: lib.sea_dnn_trainer_create(handle, pf, None, rows, 1, 4),
        "create: null row counts": lambda: lib.sea_dnn_trainer_create(handle, pf, pt, None, 1, 4),
        "create: max_batch 0": lambda: lib.sea_dnn_trainer_create(handle, pf, pt, rows, 1, 0),
        "create: max_batch 4097": lambda: lib.sea_dnn_trainer_create(handle, pf, pt, rows, 1, 4097),
        "create: no utterance": lambda: lib.sea_dnn_trainer_create(handle, pf, pt, rows, 0, 4),
        "create: a negative row count": lambda: lib.sea_dnn_trainer_create(handle, pf, pt, bad_rows, 1, 4),
    }
    for what, call in creations.items():
        assert not call(), f"{what} was accepted"
        assert lib.sea_last_error(), what
    assert lib.sea_dnn_trainer_stage_ms(None, 0) == -1.0
    lib.sea_dnn_trainer_destroy(None)


# ---- DnnMask.normaliser -----------------------------------------------------------------------------------------------------------
def test_normaliser_equals_a_direct_computation_and_refuses_a_constant_channel():
    import speech_enhancement_amd as sea
    rng = np.random.default_rng(0)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (5, 1, 40)]
    for context in (0, 2):
        shift, scale = sea.DnnMask.normaliser(feats, context)
        rows = np.concatenate(feats).astype(np.float64)
        mean = rows.sum(axis=0) / rows.shape[0]
        std = np.sqrt(((rows - mean) ** 2).sum(axis=0) / rows.shape[0])
        k = np.arange(64 * (2 * context + 1))
        assert shift.dtype == scale.dtype == np.float32 and shift.shape == scale.shape == k.shape
        assert np.allclose(shift, (-mean)[k & 63], rtol=2.0 ** -23, atol=0) and np.allclose(scale, (1.0 / std)[k & 63], rtol=2.0 ** -23, atol=0)
        normed = (rows + shift[:64].astype(np.float64)) * scale[:64].astype(np.float64)
        assert np.abs(normed.mean(axis=0)).max() < 1e-6 and np.abs(normed.std(axis=0) - 1).max() < 1e-6
    feats[2][:, 7] = feats[0][0, 7] = feats[1][0, 7] = 3.25
    feats[0][:, 7] = 3.25
    with pytest.raises(ValueError):
        sea.DnnMask.normaliser(feats, 0)
    with pytest.raises(ValueError):
        sea.DnnMask.normaliser([np.zeros((0, 64), np.float32)], 0)
