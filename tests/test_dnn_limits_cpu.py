"""The inputs of the DNN limits tests without a GPU (DESIGN.md sections 5.21 and 5.22): the launch cap of dnn_sgd_kernel parsed
from the sources and the trips it gives, the proof that the earlier DNN GPU tests never left the first trip, the density caps
and the decoy on every new training case, the step at which the overflow case stops being finite, what the poisoned features
do in the model, and the model's new runs under the sanitizers."""
import numpy as np
import pytest

from tests import dnn_limits_cases as L
from tests import dnn_model as M
from tests import dnn_train_model as T
from tests import launch_caps as LC


# ---- the launch cap ---------------------------------------------------------------------------------------------------------------
def test_sgd_cap_is_parsed_and_a_moved_constant_is_named():
    cap = LC.parse_sgd()
    assert cap == LC.SgdCap(256, 4096) and LC.sgd_second_trip_entry(cap) == 1048576
    capi, kernel = open(LC.DNN_TRAIN_CAPI).read(), open(LC.DNN_TRAIN_KERNEL).read()
    assert LC.parse_sgd(capi, kernel) == cap
    for text, other, needle in ((capi.replace("(total + 255) / 256, 4096)", "(total + 255) / 256, kSgdGrid)"), kernel, "launch cap of dnn_sgd_kernel"),
                                (capi.replace("sa.N * sa.K + sa.N", "sa.N * (sa.K + 1)"), kernel, "total"),
                                (capi, kernel.replace("gridDim.x * 256", "gridDim.x * blockDim.x"), "grid-stride loop of dnn_sgd_kernel")):
        with pytest.raises(LookupError, match=needle):
            LC.parse_sgd(text, other)
    with pytest.raises(LookupError, match="piece size disagrees"):
        LC.parse_sgd(capi.replace("(total + 255) / 256, 4096)", "(total + 511) / 512, 4096)"), kernel)


def test_trip_counts_of_the_sgd_case():
    """layer 1: 2 104 100 entries = 8220 pieces, three trips; layer 2: 1 061 000 = 4145 pieces, two trips, with Kp != K; layer 3:
    one trip"""
    cap, c = LC.parse_sgd(), L.sgd_case()
    dims = c.net.dims
    assert dims == [1984, 1060, 1000, 64] and dims[1] % 32 != 0  # K = 1060 of layer 2 is no multiple of the K tile: Kp = 1088
    got = [LC.sgd_trips(dims[l + 1], dims[l], cap) for l in range(3)]
    print(got)
    assert tuple(t.busiest for t in got) == L.SGD_TRIPS == (3, 2, 1)
    assert [t.work for t in got] == [8220, 4145, 251] and got[0].at_least_3 == 28 and got[1].at_least_2 == 49
    assert len(c.feats) == 4 and [len(f) for f in c.feats] == [16, 0, 1, 32] and c.order.size == 2 * c.batch == 80
    assert len(set(c.order.tolist())) < c.order.size  # drawn with repeats


def test_the_earlier_dnn_gpu_tests_never_left_the_first_trip():
    """every network of tests/test_gpu_dnn_train.py (T.NETS x T.CONTEXTS, the handle case, the lane-map and gather cases) is below
    the cap in every layer: the second trip of dnn_sgd_kernel's loop ran in no test before tests/test_gpu_dnn_train_limits.py"""
    cap = LC.parse_sgd()
    nets = [(context, widths) for context in T.CONTEXTS for widths, _ in T.NETS]
    nets += [(1, (260, 130, 33)), (0, (130, 33)), (1, (130, 33)), (5, (33, 64)), (0, (3,))]
    largest = 0
    for context, widths in nets:
        dims = [64 * (2 * context + 1)] + list(widths)
        for l in range(len(widths)):
            largest = max(largest, dims[l + 1] * dims[l] + dims[l + 1])
            assert LC.sgd_trips(dims[l + 1], dims[l], cap).busiest == 1, (context, widths, l)
    print("largest layer of the earlier tests:", largest, "entries; a second trip starts at", LC.sgd_second_trip_entry(cap))
    assert largest == 183300
    for name in L.LIMITS:  # nor do the other limit cases: the trips are the sgd case's alone
        dims = L.limit_case(name).net.dims
        assert all(LC.sgd_trips(dims[l + 1], dims[l], cap).busiest == 1 for l in range(len(dims) - 1)), name


def _decoy_shares(r, d):
    return [float(np.mean(r.G[l] != d.G[l])) for l in range(1, len(r.weights) + 1)]


def test_sgd_case_is_dense_past_the_cap_and_tells_the_order():
    """on the MODEL's result: every value finite, the density caps of the deltas, at most 5 % of the entries of every later trip
    with a momentum of exactly zero or an unchanged weight, and the decoy's G differs in every layer"""
    c, r = L.sgd_case(), L.sgd_case_model()
    zeros, shares = L.check_density(c, r), L.check_untouched(c, r)
    differ = _decoy_shares(r, L.sgd_case_model(True))
    print("zero deltas", zeros, "untouched per (layer, trip)", shares, "decoy: share of G that differs", differ)
    assert sorted(shares) == [(1, 2), (1, 3), (2, 2)]
    assert min(differ) > 0  # one value is enough to tell the order; the shares are printed


@pytest.mark.parametrize("name", list(L.LIMITS))
def test_limit_cases_are_dense_and_tell_the_order(name):
    c, r = L.limit_case(name), L.limit_case_model(name)
    context, widths, acts, rows, steps, _ = L.LIMITS[name]
    assert c.net.dims == [64 * (2 * context + 1)] + list(widths) and c.batch == rows and r.losses.size == steps and r.last_batch == rows
    zeros = L.check_density(c, r)
    differ = _decoy_shares(r, L.limit_case_model(name, True))
    changed = [float(np.mean(w != w0)) for w, w0 in zip(r.weights, c.net.weights)]
    print(name, "zero deltas", zeros, "decoy: share of G that differs", differ, "share of W that moved", changed)
    assert min(differ) > 0 and min(changed) > 0  # every layer's G tells the order and every layer's W moved; the shares are printed


def test_zero_row_case_is_what_it_says():
    c, r = L.zero_row_case(), L.zero_row_case_model()
    rows = [len(f) for f in c.feats]
    assert rows[0] == 0 and rows[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(rows[1:-1], rows[2:-1]))
    L.check_density(c, r)
    assert r.last_batch == 4 and r.losses.size == 3
    x0 = np.concatenate([M.splice_numpy(c.net, f) for f in c.feats if len(f)])
    assert np.array_equal(r.act[0], x0[c.order[-4:]])  # the model's gather skips the empty utterances as the numpy splice does
    # the inference list: the model gives no row for an empty utterance and splices the others as if it were not there
    net, feats = L.chain_net(), L.forward_zero_row_feats()
    want = M.forward(net, feats)
    dense = M.forward(net, [f for f in feats if len(f)])
    assert [len(w) for w in want] == list(L.FORWARD_ZERO_ROW_CUTS)
    assert all(np.array_equal(a, b) for a, b in zip([w for w in want if len(w)], dense))


def test_overflow_case_stops_being_finite_in_step_1():
    """the first step's loss (step 0) is finite, the second's (step 1) is not, with a finite eta: in the MODEL"""
    c, r = L.overflow_case(), L.overflow_case_model()
    assert np.isfinite(c.eta) and c.net.acts == [0] and len(c.net.weights) == 1
    print("losses", r.losses)
    assert r.losses.size == 2 and np.isfinite(r.losses[0]) and r.losses[0] > 0 and not np.isfinite(r.losses[1])
    once = T.train(c.net, c.feats, c.targets, c.order[:4], 4, c.eta, c.mu)
    assert np.all(np.isfinite(once.weights[0])) and np.abs(once.weights[0]).max() > 2.0 ** 70  # finite weights give that loss


def test_poisoned_features_stay_within_the_context_in_the_model():
    net, clean, poisoned, affected = L.poison_case()
    assert net.context == 2 and sorted(net.acts) == [1, 2] and len({row for row, _, _ in L.POISON}) == 3
    assert int(affected.sum()) == 15 and sum(int(np.sum(~np.isfinite(f))) for f in poisoned) == 3 and not np.isfinite(poisoned[1]).all()
    a, b = M.forward(net, clean), M.forward(net, poisoned)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1][~affected], b[1][~affected])
    assert all(np.all(np.isfinite(v)) for v in a)
    changed = (a[1] != b[1]).any(axis=1)
    assert np.array_equal(changed, affected)  # every row within C of a poisoned one does change
    assert np.isnan(b[1]).any() and np.isfinite(b[1][affected]).any()  # both classes occur among the affected rows
    assert L.class_differences(b[1], b[1]) == 0 and L.class_differences(a[1], b[1]) > 0


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------
def test_new_model_runs_are_clean_under_the_sanitizers():
    """the launch-cap case and the eight-layer case (8 layers, context 15 and an utterance of no row are new to the drivers) at
    -O1 with -fsanitize=address,undefined give the same bits (stand-alone programs; nothing is loaded into python)"""
    for c, plain in ((L.sgd_case(), L.sgd_case_model()), (L.limit_case("eight"), L.limit_case_model("eight"))):
        checked = L._model(c, sanitize=True)
        for name in ("weights", "biases", "vw", "vb", "act"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(getattr(plain, name), getattr(checked, name))), name
        for name in ("delta", "G", "g"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(getattr(plain, name)[1:], getattr(checked, name)[1:])), name
        assert plain.losses.tobytes() == checked.losses.tobytes()
    net, feats = L.limit_case("eight").net, L.forward_feats("eight")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(M.forward(net, feats), M.forward(net, feats, sanitize=True)))
    net, feats = L.chain_net(), L.forward_zero_row_feats()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(M.forward(net, feats), M.forward(net, feats, sanitize=True)))
