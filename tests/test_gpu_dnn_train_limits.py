"""The DNN mask estimator's trainer at the limits of its contract, every comparison bit for bit as
values against the plain-C model of tests/dnn_train_model.py on the inputs of tests/dnn_limits_cases.py: dnn_sgd_kernel past
its launch cap (three trips, two trips with Kp != K), eight layers, width 4096 as N and as K, B = max_batch = 4096, utterances
of no row, and return code 2 for a loss that is not finite.  tests/test_dnn_limits_cpu.py proves on the CPU that the inputs
reach those paths, are dense and tell the order of the sums."""
import numpy as np
import pytest

from tests import dnn_limits_cases as L
from tests import dnn_model as M
from tests import launch_caps as LC
from tests.test_gpu_dnn_train import _compare_with_model, _device_net, _same, _sea

pytestmark = pytest.mark.gpu


def _trainer(c, max_batch=None):
    model = _device_net(c.net)
    return model, _sea().DnnTrainer(model, c.feats, c.targets, max_batch=c.batch if max_batch is None else max_batch)


# ---- 1. dnn_sgd_kernel past its launch cap ----------------------------------------------------------------------------------------
def test_sgd_kernel_past_its_launch_cap():
    """context 15, widths (1060, 1000, 64), two steps of B = 40 with momentum on utterances of 16, 0, 1 and 32 rows.  The
    busiest workgroup of dnn_sgd_kernel takes three trips over layer 1's 2 104 100 entries, two over layer 2's 1 061 000 (where
    K = 1060 and Kp = 1088, so that the weight's address j Kp + k is not its flat index), one over layer 3's: the trip counts
    are re-derived here from the parsed cap, and at most 5 % of the entries of a later trip have, in the model, a momentum of
    exactly zero or an unchanged weight, so that a trip that did not run or wrote elsewhere shows in `momentum of W_l` and
    `W_l after the steps`.  Two steps: the second reads the momentum the first one's trips wrote."""
    cap, c, r = LC.parse_sgd(), L.sgd_case(), L.sgd_case_model()
    dims = c.net.dims
    assert tuple(LC.sgd_trips(dims[l + 1], dims[l], cap).busiest for l in range(3)) == L.SGD_TRIPS
    L.check_density(c, r)
    print("untouched per (layer, trip)", L.check_untouched(c, r))
    model, trainer = _trainer(c)
    losses = trainer.run(c.order, c.batch, c.eta, c.mu)
    _compare_with_model(trainer, model, losses, r, f"sgd past the cap, {c.widths}")


# ---- 2. the limits that are accepted ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.LIMITS))
def test_steps_at_the_limits_equal_the_c_model(name):
    """eight layers (layers 5..8, their slots of d_w, of the stage table and of sea_dnn_trainer_read); width 4096 as N (32 N
    tiles forward, 64 in wgrad, ld = 4096) and as K (128 K tiles into one accumulator, dgrad over 64 column tiles, wgrad's ones
    column in a tile of its own); B = max_batch = 4096 (64 reduction steps of wgrad, 64 row tiles of dgrad, 1024 workgroups of
    dnn_delta_out_kernel, 64 terms per lane in dnn_loss_kernel).  Three steps (two at B = 4096) with momentum."""
    c, r = L.limit_case(name), L.limit_case_model(name)
    L.check_density(c, r)
    model, trainer = _trainer(c)
    assert trainer.max_batch == c.batch == L.LIMITS[name][3]
    losses = trainer.run(c.order, c.batch, c.eta, c.mu)
    _compare_with_model(trainer, model, losses, r, f"{name}: B {c.batch}, {c.widths} {c.acts}")
    if name == "eight":
        n = len(c.widths)  # SEA_DNN_TRAIN_STAGE_*: GATHER, FORWARD0 + l - 1, DELTA, DGRAD0 + l - 1 (l >= 2), WGRAD0 + l - 1, UPDATE, ALL
        stages = [0] + [1 + l for l in range(n)] + [9] + [10 + l for l in range(1, n)] + [18 + l for l in range(n)] + [26, 27]
        times = {s: trainer.stage_ms(s) for s in stages}
        print("stage ms", times)
        assert len(times) == 1 + 8 + 1 + 7 + 8 + 2 and all(t >= 0 for t in times.values()), times
        assert trainer.stage_ms(28) == -1.0


# ---- 3. utterances of no row ------------------------------------------------------------------------------------------------------
def test_training_set_with_utterances_of_no_row():
    """utterances of 0, 6, 0, 0, 1, 9 and 0 rows through DnnTrainer (the wrapper passes an empty array as it is): the gather
    bisects a row-offset table with repeated entries.  The order holds the first and the last row of every non-empty utterance;
    every minibatch's a_0 is checked row by row against the numpy splice of the row's own utterance."""
    c, r = L.zero_row_case(), L.zero_row_case_model()
    L.check_density(c, r)
    model, trainer = _trainer(c, max_batch=8)
    assert trainer.total_rows == sum(L.ZERO_ROW_CUTS)
    losses = trainer.run(c.order, c.batch, c.eta, c.mu)
    _compare_with_model(trainer, model, losses, r, "utterances of no row")
    x0 = np.concatenate([M.splice_numpy(c.net, f) for f in c.feats if len(f)])
    for rows in (c.order[:5], c.order[5:10], c.order[10:]):
        trainer.run(rows, 5, 0.0, 0.0, update=False)
        _same(trainer.read("act", 0), x0[rows], f"a_0 of rows {rows.tolist()}")


# ---- 4. a loss that is not finite -------------------------------------------------------------------------------------------------
def test_a_loss_that_is_not_finite_returns_2_and_names_the_step():
    """an identity layer and eta = 2^80: the model's loss of step 0 is finite, that of step 1 is not (asserted on the CPU too).
    sea_dnn_trainer_run returns exactly 2 and names step 1, losses[0] equals the model's; the handle survives, and an
    evaluation on it returns 2 again.  The values after that point are not pinned."""
    from speech_enhancement_amd.engine import _np_ptr
    sea = _sea()
    lib = sea.load()
    c, r = L.overflow_case(), L.overflow_case_model()
    assert np.isfinite(r.losses[0]) and not np.isfinite(r.losses[1])
    model, trainer = _trainer(c)
    order, losses = np.ascontiguousarray(c.order, np.int64), np.full(2, -1.0, np.float64)
    rc = lib.sea_dnn_trainer_run(trainer._handle, _np_ptr(order), order.size, c.batch, float(c.eta), float(c.mu), 1, _np_ptr(losses))
    message = lib.sea_last_error()
    print("return code", rc, "message", message, "losses", losses, "model", r.losses)
    assert rc == 2
    assert b"step 1 " in message and b"not finite" in message
    _same(losses[:1], r.losses[:1], "the loss of step 0")
    assert not np.isfinite(losses[1])
    again = np.full(2, -1.0, np.float64)
    rc = lib.sea_dnn_trainer_run(trainer._handle, _np_ptr(order), order.size, c.batch, float(c.eta), float(c.mu), 0, _np_ptr(again))
    assert rc == 2 and b"not finite" in lib.sea_last_error()
    with pytest.raises(sea.SeaError, match="not finite"):
        trainer.run(c.order, c.batch, c.eta, c.mu, update=False)
    _, fresh = _trainer(c)  # the trainer keeps its model alive
    with pytest.raises(sea.SeaError, match="step 1 is not finite"):
        fresh.run(c.order, c.batch, c.eta, c.mu)
