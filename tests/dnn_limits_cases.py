"""Test infrastructure: the inputs of the DNN estimator's and its trainer's tests at the limits of their contract (DESIGN.md
sections 5.21 and 5.22), shared by the GPU tests (tests/test_gpu_dnn_limits.py, tests/test_gpu_dnn_train_limits.py) and by
the CPU tests that prove those inputs reach what they are meant to reach (tests/test_dnn_limits_cpu.py).

  sgd_case        context 15, widths (1060, 1000, 64): layers whose N K + N entries pass dnn_sgd_kernel's launch cap (three
                  trips, two trips with Kp != K, one trip)
  limit_case      eight layers; width 4096 as N and as K; B = max_batch = 4096
  zero_row_case   a training set with utterances of no row first, last and two in a row
  overflow_case   an identity layer and a finite eta after which the second step's loss is not finite
  poison_case     features with one NaN, one +Inf and one -Inf for sea_dnn_forward

Every model result is computed once per process and is to be treated as read-only."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import dnn_model as M
from tests import dnn_train_model as T
from tests import launch_caps as LC


def _set(rng, cuts, n_out):
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in cuts]
    targets = [rng.uniform(0, 1, size=(F, n_out)).astype(np.float32) for F in cuts]
    return feats, targets


def _case(net, feats, targets, order, batch, widths, acts, eta=T.ETA, mu=T.MU):
    return SimpleNamespace(net=net, feats=feats, targets=targets, order=np.asarray(order, np.int64), batch=int(batch), eta=eta, mu=mu,
                           widths=tuple(widths), acts=tuple(acts))


def _model(c, decoy=False, sanitize=False):
    return T.train(c.net, c.feats, c.targets, c.order, c.batch, c.eta, c.mu, decoy=decoy, sanitize=sanitize)


def check_density(c, r):
    """check_density of tests/dnn_train_model.py on a case of this file, on the MODEL's values of the last step: every value
    finite, at most 5 % of a sigmoid or identity layer's delta exactly zero, at most 75 % of a ReLU layer's"""
    everything = [r.losses] + r.weights + r.biases + r.vw + r.vb + r.act + r.delta[1:] + r.G[1:] + r.g[1:]
    assert all(np.all(np.isfinite(v)) for v in everything), c.widths
    zeros = [float(np.mean(r.delta[l] == 0)) for l in range(1, len(c.acts) + 1)]
    for l, z in enumerate(zeros, 1):
        cap = 0.75 if c.acts[l - 1] == 2 else 0.05
        assert z <= cap, f"{c.widths}, layer {l} (activation {c.acts[l - 1]}): {z:.3f} of delta is zero"
    return zeros


# ---- dnn_sgd_kernel past its launch cap -------------------------------------------------------------------------------------------
SGD_CONTEXT, SGD_WIDTHS, SGD_ACTS, SGD_BATCH, SGD_STEPS, SGD_CUTS = 15, (1060, 1000, 64), (1, 2, 1), 40, 2, (16, 0, 1, 32)
SGD_TRIPS = (3, 2, 1)  # the busiest workgroup's trips per layer, which tests/test_dnn_limits_cpu.py derives from the parsed cap
UNTOUCHED_CAP = 0.05
SGD_SEED = 2  # of seeds 1..8 those at which layer 2's second trip (its last 12 rows, 12 424 entries) meets no dead rectifier: 2, 4, 5, 8


def sgd_case():
    """two steps of B = 40 on four utterances of 16, 0, 1 and 32 rows, the order drawn with repeats.  Layer 1 has
    1984 * 1060 + 1060 = 2 104 100 entries, layer 2 1060 * 1000 + 1000 = 1 061 000 (K = 1060, Kp = 1088), layer 3 64 064."""
    net = T.dense_net(SGD_SEED, SGD_CONTEXT, SGD_WIDTHS, SGD_ACTS)
    rng = np.random.default_rng(SGD_SEED)
    feats, targets = _set(rng, SGD_CUTS, SGD_WIDTHS[-1])
    order = rng.integers(0, sum(SGD_CUTS), size=SGD_STEPS * SGD_BATCH)
    return _case(net, feats, targets, order, SGD_BATCH, SGD_WIDTHS, SGD_ACTS)


@functools.lru_cache(maxsize=None)
def sgd_case_model(decoy=False):
    return _model(sgd_case(), decoy)


def untouched_shares(c, r, cap=None):
    """per layer, per trip t >= 2 of dnn_sgd_kernel's loop: the share of the entries that trip covers (flat index over W row-major,
    then b, in [(t - 1) G, t G) with G = 256 * 4096 = 1 048 576) whose momentum is exactly zero or whose weight equals its initial
    value on the MODEL's result -> {(layer, trip): share}.  A trip that never ran, or that wrote elsewhere, must not be able to
    hide behind such entries: check_untouched holds every share to UNTOUCHED_CAP."""
    cap = LC.parse_sgd() if cap is None else cap
    per_trip = LC.sgd_second_trip_entry(cap)
    shares = {}
    for l, (w0, b0) in enumerate(zip(c.net.weights, c.net.biases)):
        v = np.concatenate([r.vw[l].reshape(-1), r.vb[l]])
        same = np.concatenate([(r.weights[l] == w0).reshape(-1), r.biases[l] == b0])
        quiet = (v == 0) | same
        for t in range(2, (quiet.size + per_trip - 1) // per_trip + 1):
            shares[(l + 1, t)] = float(np.mean(quiet[(t - 1) * per_trip:t * per_trip]))
    return shares


def check_untouched(c, r):
    shares = untouched_shares(c, r)
    for (layer, trip), share in shares.items():
        assert share <= UNTOUCHED_CAP, f"layer {layer}, trip {trip}: {share:.4f} of the entries have zero momentum or an unchanged weight"
    return shares


# ---- the limits that are accepted -------------------------------------------------------------------------------------------------
#         name       context  widths                            acts                      rows  steps  seed
LIMITS = {"eight":   (0, (5, 130, 3, 33, 1, 64, 260, 64), (1, 2, 0, 1, 1, 2, 1, 1), 70, 3, 2),
          "n4096":   (1, (3, 4096), (1, 0), 33, 3, 3),
          "k4096":   (0, (4096, 3), (2, 1), 33, 3, 4),
          "b4096":   (0, (130, 33), (2, 1), 4096, 2, 5)}
FORWARD_LIMITS = ("eight", "n4096", "k4096")  # b4096 is a limit of the trainer alone


def limit_case(name):
    """B = rows, a set of three utterances (one of one row) holding rows + 9 rows, `steps` full minibatches drawn with repeats"""
    context, widths, acts, rows, steps, seed = LIMITS[name]
    net = T.dense_net(seed, context, widths, acts)
    rng = np.random.default_rng(seed)
    total = rows + 9
    cuts = (total // 3, 1, total - total // 3 - 1)
    feats, targets = _set(rng, cuts, widths[-1])
    order = rng.integers(0, total, size=steps * rows)
    return _case(net, feats, targets, order, rows, widths, acts)


@functools.lru_cache(maxsize=None)
def limit_case_model(name, decoy=False):
    return _model(limit_case(name), decoy)


def forward_feats(name):
    """the rows of the inference comparison of a limit case: two utterances holding the table's row count"""
    rows = LIMITS[name][3]
    rng = np.random.default_rng(rows)
    return [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (rows // 3, rows - rows // 3)]


def context15_feats():
    rng = np.random.default_rng(15)
    return [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in (1, 129)]


# ---- utterances of no row ---------------------------------------------------------------------------------------------------------
ZERO_ROW_CUTS = (0, 6, 0, 0, 1, 9, 0)
FORWARD_ZERO_ROW_CUTS = (0, 100, 0, 0, 150, 200, 1, 0, 400, 0)


def zero_row_case():
    """context 2, widths (33, 64); utterances of no row first, last and two in a row between non-empty ones; the order holds the
    first and the last row of every non-empty utterance, repeats, and ends in a minibatch of 4 rows where batch is 5"""
    widths, acts = (33, 64), (2, 1)
    net = T.dense_net(6, 2, widths, acts)
    rng = np.random.default_rng(6)
    feats, targets = _set(rng, ZERO_ROW_CUTS, widths[-1])
    order = [0, 5, 6, 7, 15, 3, 6, 6, 10, 0, 15, 7, 5, 11]
    ends = np.cumsum(ZERO_ROW_CUTS)
    assert all(e - F in order and e - 1 in order for e, F in zip(ends, ZERO_ROW_CUTS) if F)
    return _case(net, feats, targets, order, 5, widths, acts)


@functools.lru_cache(maxsize=None)
def zero_row_case_model():
    return _model(zero_row_case())


def chain_net():
    """the network of tests/test_gpu_dnn.py's chain fixture: context 2, widths (96, 64)"""
    rng = np.random.default_rng(21)
    net = M.random_net(21, 2, (96, 64), (1, 1), spread=2)
    net.shift[:] = rng.uniform(-11, -9, size=net.shift.size).astype(np.float32)
    net.scale[:] = rng.uniform(0.05, 0.15, size=net.scale.size).astype(np.float32)
    return net


def forward_zero_row_feats():
    rng = np.random.default_rng(22)
    return [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in FORWARD_ZERO_ROW_CUTS]


# ---- a loss that is not finite ----------------------------------------------------------------------------------------------------
OVERFLOW_ETA = np.float32(2.0 ** 80)


def overflow_case():
    """an identity layer 64 -> 3, two steps of B = 4 with eta = 2^80 and mu = 0: the first step's loss is that of the initial
    weights; its update leaves weights near 2^80 times the gradient, whose outputs' squares are above FLT_MAX in the second"""
    net = T.dense_net(7, 0, (3,), (0,))
    rng = np.random.default_rng(7)
    feats, targets = _set(rng, (8,), 3)
    return _case(net, feats, targets, np.arange(8), 4, (3,), (0,), eta=OVERFLOW_ETA, mu=np.float32(0.0))


@functools.lru_cache(maxsize=None)
def overflow_case_model():
    return _model(overflow_case())


# ---- features that are not finite -------------------------------------------------------------------------------------------------
POISON_CONTEXT, POISON_CUTS = 2, (12, 40, 9)
POISON = ((5, 7, np.nan), (20, 0, np.inf), (33, 63, -np.inf))  # (row of the middle utterance, channel, value)


def poison_case():
    """-> (net, clean features, poisoned features, the mask [40] of the middle utterance's rows within C rows of a poisoned one)"""
    net = T.dense_net(8, POISON_CONTEXT, (33, 64), (2, 1))
    rng = np.random.default_rng(8)
    clean = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in POISON_CUTS]
    poisoned = [f.copy() for f in clean]
    rows = np.arange(POISON_CUTS[1])
    affected = np.zeros(POISON_CUTS[1], bool)
    for row, chan, value in POISON:
        poisoned[1][row, chan] = np.float32(value)
        affected |= np.abs(rows - row) <= POISON_CONTEXT
    return net, clean, poisoned, affected


def class_differences(got, want):
    """how many values differ in class: a NaN must sit where a NaN sits (payload and sign free: an x86 generates the negative
    quiet NaN, gfx950 the positive one), every other value -- an infinity with its sign, a finite value -- must be equal as a
    value (the rule of tests/nonfinite_cases.py, with -0 equal to +0 as everywhere in the DNN tests)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    nan = np.isnan(want)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.where(nan, ~np.isnan(got), got != want)))
