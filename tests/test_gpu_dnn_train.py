"""The DNN mask estimator's trainer on the GPU, every comparison bit for bit as values against the
plain-C model of tests/dnn_train_model.py: the lane maps of the two gradient GEMMs on exact integers, the order of every sum on
inputs proven order-sensitive, the gather through an index list, and the trained handle in the inference calls."""
import numpy as np
import pytest

from tests import dnn_model as M
from tests import dnn_train_model as T

pytestmark = pytest.mark.gpu


def _sea():
    import speech_enhancement_amd as sea
    return sea


def _device_net(net):
    return _sea().DnnMask(net.context, net.shift, net.scale, net.weights, net.biases, net.acts)


def _same(got, want, what, failures=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(want)), what
    differ = int(np.sum(got != want))  # as values: -0 equals +0
    print(f"{what}: {got.size} values, {differ} differ"
          + (f", largest |delta| {np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))):.3g}" if differ else ""))
    if failures is None:
        assert differ == 0, what
    elif differ:
        failures.append(what)


def _compare_with_model(trainer, model, losses, r, what):
    """every stage sea_dnn_trainer_read gives of the last step, the losses of all steps, and W, b and the momentum after them;
    all stages are printed before the assertion, so that a failure says which kernel is wrong"""
    n, failures = len(model.weights), []
    _same(losses, r.losses, f"{what}: losses", failures)
    for l in range(n + 1):
        _same(trainer.read("act", l), r.act[l], f"{what}: a_{l}", failures)
    for l in range(n, 0, -1):
        _same(trainer.read("delta", l), r.delta[l], f"{what}: delta_{l}", failures)
        _same(trainer.read("wgrad", l), r.G[l], f"{what}: G_{l}", failures)
        _same(trainer.read("bgrad", l), r.g[l], f"{what}: g_{l}", failures)
    model.pull()
    for l in range(n):
        _same(trainer.read("wmom", l + 1), r.vw[l], f"{what}: momentum of W_{l + 1}", failures)
        _same(trainer.read("bmom", l + 1), r.vb[l], f"{what}: momentum of b_{l + 1}", failures)
        _same(model.weights[l], r.weights[l], f"{what}: W_{l + 1} after the steps", failures)
        _same(model.biases[l], r.biases[l], f"{what}: b_{l + 1} after the steps", failures)
    assert not failures, failures


# ---- 1. the lane maps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("layers", [1, 2])
def test_lane_maps_on_exact_integers(context, layers):
    """identity activations, eta = 1, mu = 0, B = 200 rows in a shuffled order, widths 130 (and 33): one-hot integer input rows
    (times 1..4), the asymmetric W_1[j][k] = (3 j + 7 k + 1) mod 7 - 3 and W_2[i][j] = (3 i + 7 j + 1) mod 3 - 1, integer biases
    and targets.  Every sum of magnitudes is below 2^24 (asserted in int64), so G, g, E and the updated W equal the int64
    numpy products whatever the order -- a transposed operand, a wrong k half or a misplaced reduction tile shows here."""
    sea = _sea()
    k0, rows = 64 * (2 * context + 1), 200
    widths = (130, 33)[:layers]
    dims = [k0] + list(widths)
    mod = (7, 3)
    Ws = [((3 * np.arange(dims[l + 1])[:, None] + 7 * np.arange(dims[l])[None, :] + 1) % mod[l] - mod[l] // 2) for l in range(layers)]
    bs = [np.arange(dims[l + 1]) % 3 for l in range(layers)]
    net = M.make_net(context, np.zeros(k0), np.ones(k0), Ws, bs, [0] * layers)
    feats = np.zeros((rows, 64), np.float32)
    feats[np.arange(rows), np.arange(rows) % 64] = 1 + np.arange(rows) // 64
    targets = (np.arange(rows)[:, None] * 5 + np.arange(widths[-1])[None, :] * 3) % 4
    order = np.random.default_rng(context).permutation(rows)
    x0 = M.splice_numpy(net, feats).astype(np.int64)[order]
    a = [x0]
    for W, b in zip(Ws, bs):
        a.append(a[-1] @ W.T + b[None, :])
    delta = [None] * (layers + 1)
    delta[layers] = a[layers] - targets[order]
    G, g, bound = [None] * (layers + 1), [None] * (layers + 1), 0
    for l in range(layers, 0, -1):
        G[l], g[l] = delta[l].T @ a[l - 1], delta[l].sum(axis=0)
        bound = max(bound, (np.abs(delta[l]).T @ np.abs(a[l - 1])).max(), np.abs(delta[l]).sum(axis=0).max())
        if l > 1:
            delta[l - 1] = delta[l] @ Ws[l - 1]
            bound = max(bound, (np.abs(delta[l]) @ np.abs(Ws[l - 1])).max())
    for l in range(layers):
        bound = max(bound, (np.abs(a[l]) @ np.abs(Ws[l]).T + np.abs(bs[l])[None, :]).max(), np.abs(Ws[l] - G[l + 1]).max())
    r_sq = (delta[layers] ** 2).sum(axis=1)
    print("largest sum of magnitudes", bound, "largest row sum of squares", r_sq.max())
    assert bound < 2 ** 24 and r_sq.max() < 2 ** 24
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, [feats], [targets], max_batch=rows)
    losses = trainer.run(order, rows, 1.0, 0.0)
    failures = []
    _same(losses, [0.5 * r_sq.sum()], "loss", failures)
    for l in range(layers + 1):
        _same(trainer.read("act", l), a[l].astype(np.float32), f"a_{l}", failures)
    model.pull()
    for l in range(layers, 0, -1):
        _same(trainer.read("delta", l), delta[l].astype(np.float32), f"delta_{l} (E for l < n)", failures)
        _same(trainer.read("wgrad", l), G[l].astype(np.float32), f"G_{l}", failures)
        _same(trainer.read("bgrad", l), g[l].astype(np.float32), f"g_{l}", failures)
        _same(model.weights[l - 1], (Ws[l - 1] - G[l]).astype(np.float32), f"updated W_{l}", failures)
        _same(model.biases[l - 1], (bs[l - 1] - g[l]).astype(np.float32), f"updated b_{l}", failures)
    assert not failures, failures
    r = T.train(net, [feats], [targets], order, rows, 1.0, 0.0)  # and the C model agrees with the integers
    assert all(np.array_equal(r.G[l], G[l].astype(np.float32)) for l in range(1, layers + 1))
    assert all(np.array_equal(r.weights[l], (Ws[l] - G[l + 1]).astype(np.float32)) for l in range(layers))


# ---- 2. the order of the sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", T.CONTEXTS)
@pytest.mark.parametrize("rows", T.ROWS)
def test_three_steps_equal_the_c_model_where_order_matters(context, rows):
    """three steps with mu = 0.9 on the inputs of tests/dnn_train_model.py::order_case (all nine networks, every activation,
    widths 1..260, a denormal weight and a denormal input): every read stage of the last step, the losses of all steps, and W,
    b and the momentum after them.  tests/test_dnn_train_cpu.py proves that the decoy (G over m descending, E over j
    descending) differs on every case with B >= 31; the density caps are re-asserted here on the model's values."""
    sea = _sea()
    c, r = T.order_case(context, rows), T.order_case_model(context, rows)
    T.check_density(context, rows)
    model = _device_net(c.net)
    trainer = sea.DnnTrainer(model, c.feats, c.targets, max_batch=rows)
    losses = trainer.run(c.order, c.batch, c.eta, c.mu)
    _compare_with_model(trainer, model, losses, r, f"context {context}, B {rows}, {c.widths} {c.acts}")


def test_denormal_gradients_and_weights_survive():
    """weights of 1e-40 and inputs of 3e-39: every product of the weight gradient, its sums and the updated weights are
    denormal and must not be flushed"""
    sea = _sea()
    net = M.make_net(0, np.zeros(64), np.ones(64), [np.full((3, 64), 1e-40)], [np.zeros(3)], [0])
    feats = np.full((3, 64), 3e-39, np.float32)
    targets = np.full((3, 3), 0.5, np.float32)
    r = T.train(net, [feats], [targets], np.arange(3), 3, 1.0, 0.0)
    assert np.all((np.abs(r.G[1]) > 0) & (np.abs(r.G[1]) < 1e-38)) and np.all((np.abs(r.weights[0]) > 0) & (np.abs(r.weights[0]) < 1e-38))
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, [feats], [targets], max_batch=4)
    _compare_with_model(trainer, model, trainer.run(np.arange(3), 3, 1.0, 0.0), r, "denormals")


# ---- 3. the gather ----------------------------------------------------------------------------------------------------------------
def test_gather_through_an_order_with_repeats_and_a_short_last_minibatch():
    """context 5, utterances of 1, 2, 10, 11 and 17 rows; the order repeats rows, holds the first and the last row of
    utterances and the one-row utterance, and ends in a minibatch of 3 rows where batch is 5 and max_batch 8"""
    sea = _sea()
    net = T.dense_net(77, 5, (33, 64), (1, 1))
    rng = np.random.default_rng(77)
    cuts = (1, 2, 10, 11, 17)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in cuts]
    targets = [rng.uniform(0, 1, size=(F, 64)).astype(np.float32) for F in cuts]
    order = np.array([0, 1, 2, 3, 12, 13, 23, 24, 40, 40, 40, 0, 24])
    r = T.train(net, feats, targets, order, 5, T.ETA, T.MU)
    assert r.last_batch == 3 and r.losses.size == 3
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, feats, targets, max_batch=8)
    losses = trainer.run(order, 5, T.ETA, T.MU)
    _compare_with_model(trainer, model, losses, r, "gather")
    # every minibatch's input rows, one evaluation each: the model's a_0 is the splice of the inference model
    x0 = np.concatenate([M.splice_numpy(net, f) for f in feats])
    for rows in (order[:5], order[5:10], order[10:]):
        trainer.run(rows, 5, 0.0, 0.0, update=False)
        _same(trainer.read("act", 0), x0[rows], f"a_0 of rows {rows.tolist()}")


def test_run_refuses_what_needs_the_trainer_and_leaves_the_state_alone():
    sea = _sea()
    net = T.dense_net(5, 0, (3,), (1,))
    feats, targets = [np.ones((4, 64), np.float32)], [np.zeros((4, 3), np.float32)]
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, feats, targets, max_batch=2)
    for order, batch in (([0, 1, 2], 3), ([0, 4], 2), ([-1], 1)):  # batch > max_batch; an index past the set; a negative index
        with pytest.raises(sea.SeaError):
            trainer.run(order, batch, 0.1)
    for what, layer in (("act", 2), ("delta", 0), ("wgrad", 2), (6, 1), (-1, 1)):
        with pytest.raises(sea.SeaError):
            trainer.read(what, layer)
    model.pull()
    assert model.weights[0].tobytes() == net.weights[0].tobytes() and model.biases[0].tobytes() == net.biases[0].tobytes()


# ---- 4. the trained handle --------------------------------------------------------------------------------------------------------
def _handle_case():
    net = T.dense_net(41, 1, (260, 130, 33), (1, 2, 1))
    rng = np.random.default_rng(41)
    cuts = (9, 1, 30)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in cuts]
    targets = [rng.uniform(0, 1, size=(F, 33)).astype(np.float32) for F in cuts]
    return net, feats, targets


def test_trained_handle_serves_the_forward_call():
    """after two steps sea_dnn_forward on fresh rows equals the C model's forward with the C model's updated weights; widths
    260, 130 and 33 leave tile padding in every layer, which the update must not have written"""
    sea = _sea()
    net, feats, targets = _handle_case()
    order = np.random.default_rng(1).integers(0, 40, size=32)
    r = T.train(net, feats, targets, order, 16, T.ETA, T.MU)
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, feats, targets, max_batch=16)
    losses = trainer.run(order, 16, T.ETA, T.MU)
    _same(losses, r.losses, "losses")
    fresh = [np.random.default_rng(2).uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (7, 130)]
    trained = M.make_net(net.context, net.shift, net.scale, r.weights, r.biases, net.acts)
    assert not np.array_equal(r.weights[0], net.weights[0])
    for u, (got, want) in enumerate(zip(sea.dnn_forward(model, fresh), M.forward(trained, fresh))):
        _same(got, want, f"forward with the trained handle, utterance {u}")


def test_evaluation_touches_nothing_and_gives_the_steps_loss():
    sea = _sea()
    net, feats, targets = _handle_case()
    model = _device_net(net)
    trainer = sea.DnnTrainer(model, feats, targets, max_batch=16)
    order = np.arange(16) * 2
    trainer.run(order, 16, T.ETA, T.MU)  # one real step first, so that the momentum is not zero
    model.pull()
    before = [w.tobytes() for w in model.weights + model.biases]
    before += [trainer.read(what, l).tobytes() for what in ("wmom", "bmom") for l in (1, 2, 3)]
    loss_eval = trainer.run(order, 16, T.ETA, T.MU, update=False)
    total = trainer.evaluate(16)
    model.pull()
    after = [w.tobytes() for w in model.weights + model.biases]
    after += [trainer.read(what, l).tobytes() for what in ("wmom", "bmom") for l in (1, 2, 3)]
    assert before == after
    loss_step = trainer.run(order, 16, T.ETA, T.MU)
    assert loss_eval.tobytes() == loss_step.tobytes() and np.isfinite(total) and total > 0


def test_two_epochs_from_the_same_start_give_identical_bits():
    sea = _sea()
    net, feats, targets = _handle_case()
    results = []
    for _ in range(2):
        model = _device_net(net)
        trainer = sea.DnnTrainer(model, feats, targets, max_batch=16)
        losses = trainer.epoch(3, 16, T.ETA, T.MU)
        model.pull()
        results.append([losses.tobytes()] + [w.tobytes() for w in model.weights + model.biases])
        assert losses.size == 3 and trainer.last_batch == 8
    assert results[0] == results[1]
    want = T.train(net, feats, targets, np.random.default_rng(3).permutation(40), 16, T.ETA, T.MU)
    assert results[0][0] == want.losses.tobytes()
