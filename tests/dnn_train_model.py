"""Test infrastructure: the model of the DNN mask estimator's trainer.  One SGD step -- gather,
forward, loss, deltas, the two gradient chains, back-propagation, momentum update -- is the plain-C program
tests/dnn_train_model_driver.c, which includes csrc/dnn_math.h and is built here with gcc -O2 -ffp-contract=off.  The GPU results
must equal this model bit for bit as values.

Independent of it: step_float64, the formulae in float64 numpy with a running bound on |C model - float64| carried value by
value (tests/test_dnn_train_cpu.py checks the formulae against torch autograd and the C model against the bound).

order_case builds the inputs of the order-of-the-sums cases, shared by the GPU test and by the CPU tests that prove those
inputs are order-sensitive and dense.
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

from tests import dnn_model as M

SOURCE = os.path.join(M.ROOT, "tests", "dnn_train_model_driver.c")
U = M.U

_built = {}


def build_driver(sanitize=False):
    """the driver's path; built once per process (sanitize: with -fsanitize=address,undefined at -O1)"""
    if sanitize not in _built:
        cc = shutil.which("gcc")
        assert cc, "gcc is needed to build tests/dnn_train_model_driver.c"
        d = tempfile.mkdtemp(prefix="dnn_train_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "dnn_train_model_driver")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", M.CSRC, SOURCE, "-o", exe, "-lm"])
        _built[sanitize] = (exe, d)
    return _built[sanitize]


def train(net, feats_list, targets_list, order, batch, eta, mu, update=True, decoy=False, sanitize=False):
    """the C model: the steps over consecutive minibatches of `order` from zero momentum -> losses [steps] float64; weights,
    biases, vw, vb after the steps; of the last step act[0..n], delta[1..n], G[1..n], g[1..n] (index 0 of the last three is None)"""
    feats_list = [np.ascontiguousarray(f, np.float32).reshape(-1, 64) for f in feats_list]
    n, dims = len(net.weights), net.dims
    targets_list = [np.ascontiguousarray(t, np.float32).reshape(-1, dims[-1]) for t in targets_list]
    order = np.ascontiguousarray(order, np.int64).reshape(-1)
    exe, d = build_driver(sanitize)
    src, dst = os.path.join(d, "train_in.bin"), os.path.join(d, "train_out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([net.context, n] + list(dims) + list(net.acts) + [len(feats_list)] + [x.shape[0] for x in feats_list]
                           + [order.size, batch, int(bool(update))], np.int32).tobytes())
        f.write(np.asarray([eta, mu], np.float32).tobytes() + net.shift.tobytes() + net.scale.tobytes())
        for w, b in zip(net.weights, net.biases):
            f.write(w.tobytes() + b.tobytes())
        for x in feats_list + targets_list:
            f.write(x.tobytes())
        f.write(order.tobytes())
    run = subprocess.run([exe, "train", src, dst] + (["decoy"] if decoy else []), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and not run.stderr, f"dnn_train_model_driver exited with {run.returncode}:\n{run.stderr[-2000:]}"
    blob = open(dst, "rb").read()
    steps = (order.size + batch - 1) // batch
    B = order.size - (steps - 1) * batch
    losses = np.frombuffer(blob, np.float64, steps).copy()
    flat = np.frombuffer(blob, np.float32, offset=8 * steps)
    at = [0]

    def take(*shape):
        size = int(np.prod(shape))
        v = flat[at[0]:at[0] + size].reshape(shape).copy()
        at[0] += size
        return v

    r = SimpleNamespace(losses=losses, last_batch=B, weights=[], biases=[], vw=[], vb=[], act=[], delta=[None], G=[None], g=[None])
    for l in range(n):
        r.weights.append(take(dims[l + 1], dims[l])), r.biases.append(take(dims[l + 1]))
        r.vw.append(take(dims[l + 1], dims[l])), r.vb.append(take(dims[l + 1]))
    for l in range(n + 1):
        r.act.append(take(B, dims[l]))
    for l in range(1, n + 1):
        r.delta.append(take(B, dims[l]))
    for l in range(1, n + 1):
        r.G.append(take(dims[l], dims[l - 1])), r.g.append(take(dims[l]))
    assert at[0] == flat.size
    return r


# ---- the inputs of the order-of-the-sums cases ------------------------------------------------------------------------------------
ROWS = (1, 2, 31, 32, 33, 127, 128, 129, 300)
CONTEXTS = (0, 1, 5)
NETS = (((1,), (0,)), ((3,), (1,)), ((33, 64), (2, 1)), ((64,), (2,)), ((130, 3), (1, 0)), ((260, 33, 64), (1, 2, 1)),
        ((260, 130, 64, 33), (2, 2, 0, 1)), ((64, 260), (0, 1)), ((33, 1, 3), (1, 1, 2)))  # those of tests/test_gpu_dnn.py
ETA, MU, STEPS = np.float32(2.0 ** -16), np.float32(0.9), 3


def dense_net(seed, context, widths, acts):
    """weights wide_floats (spread 2) / sqrt (fan_in), biases wide_floats (spread 2) / 4, shift about -13.5 and scale about 0.13:
    features U (0, 27) reach the first layer centred and of unit size, so that no sigmoid saturates and few deltas are zero
    (random_net's spread of 12 drives every sigmoid to exactly 0 or 1: every delta would be zero)"""
    rng = np.random.default_rng(seed)
    k0 = 64 * (2 * context + 1)
    dims = [k0] + list(widths)
    weights = [M.wide_floats(rng, (dims[l + 1], dims[l]), 2) / np.float32(np.sqrt(dims[l])) for l in range(len(widths))]
    biases = [M.wide_floats(rng, dims[l + 1], 2) / np.float32(4) for l in range(len(widths))]
    shift = (-13.5 * rng.uniform(0.8, 1.25, size=k0)).astype(np.float32)
    scale = (0.13 * rng.uniform(0.5, 2.0, size=k0)).astype(np.float32)
    return M.make_net(context, shift, scale, weights, biases, acts)


def order_case(context, rows):
    """the case (context, B = rows): a network of NETS, a training set of three utterances (one of them of one row) holding
    rows + 9 rows, and an order of STEPS full minibatches drawn with repeats.  A denormal weight (W_1[0][0] = 1e-40) and a
    denormal input (row 0, centre frame, channel 0, unshifted and unscaled: 1e-41, whose products with delta_1 are denormal
    terms of G_1) are in every case; row 0 is the last row of the last step.  The step is small (eta = 2^-16 on the summed
    gradient): a larger one kills most rectifiers within the three steps.  The seed base is one at which check_density's caps
    hold: the four-layer network's sigmoid, behind two rectifiers and an identity, saturates to exactly 1 on 4 to 10 % of its
    outputs depending on the seed."""
    widths, acts = NETS[(ROWS.index(rows) + 3 * CONTEXTS.index(context)) % len(NETS)]
    net = dense_net(305000 + 1000 * context + rows, context, widths, acts)
    centre = 64 * context
    net.shift[centre], net.scale[centre] = 0.0, 1.0
    net.weights[0][0, 0] = np.float32(1e-40)
    rng = np.random.default_rng(7000 + 31 * context + rows)
    total = rows + 9
    cuts = (total // 3, 1, total - total // 3 - 1)
    feats = [rng.uniform(0, 27, size=(F, 64)).astype(np.float32) for F in cuts]
    feats[0][0, 0] = np.float32(1e-41)
    targets = [rng.uniform(0, 1, size=(F, widths[-1])).astype(np.float32) for F in cuts]
    order = rng.integers(0, total, size=STEPS * rows)
    order[-1] = 0
    return SimpleNamespace(net=net, feats=feats, targets=targets, order=order, batch=rows, eta=ETA, mu=MU, widths=widths, acts=acts)


@functools.lru_cache(maxsize=None)
def order_case_model(context, rows, decoy=False):
    """the C model's result of that case, computed once per process; treat it as read-only"""
    c = order_case(context, rows)
    return train(c.net, c.feats, c.targets, c.order, c.batch, c.eta, c.mu, decoy=decoy)


def check_density(context, rows):
    """what keeps the order-of-the-sums comparison honest, on the MODEL's values of the last step: every value finite; in the
    cases with B >= 31 at most 5 % of a sigmoid or identity layer's delta exactly zero, at most 75 % of a ReLU layer's"""
    c, r = order_case(context, rows), order_case_model(context, rows)
    everything = [r.losses] + r.weights + r.biases + r.vw + r.vb + r.act + r.delta[1:] + r.G[1:] + r.g[1:]
    assert all(np.all(np.isfinite(v)) for v in everything), (context, rows)
    zeros = [float(np.mean(r.delta[l] == 0)) for l in range(1, len(c.acts) + 1)]
    if rows >= 31:
        for l, z in enumerate(zeros, 1):
            cap = 0.75 if c.acts[l - 1] == 2 else 0.05
            assert z <= cap, f"context {context}, B {rows}, layer {l} (activation {c.acts[l - 1]}): {z:.3f} of delta is zero"
    return zeros


# ---- the formulae in float64, with the bound on the float model's distance from them ------------------------------------------------
def _rounded(value, prop):
    """one float operation whose exact result is within prop of value: fl (x) = x (1 + d), |d| <= u, |x| <= |value| + prop"""
    return prop + U * (np.abs(value) + prop)


def _gamma(k):
    return k * U / (1 - k * U)


def _product(a, ea, b, eb):
    """|a' b' - a b| for |a' - a| <= ea, |b' - b| <= eb: the product rule"""
    return np.abs(a) * eb + np.abs(b) * ea + ea * eb


def _delta64(E, eE, a, ea, z, ez, act):
    """delta = E d (a) and its bound.  Sigmoid: 1 - a and a (1 - a) and E d are three float operations on bounded factors.  ReLU:
    the float model's a > 0 is the float64's z > 0 unless |z| <= ez; there the two may pick different branches and the bound
    is |E| + eE.  Where z < -ez both give 0."""
    if act == 1:
        om, eom = 1.0 - a, _rounded(1.0 - a, ea)
        d, ed = a * om, _rounded(a * om, _product(a, ea, om, eom))
        return E * d, _rounded(E * d, _product(E, eE, d, ed))
    if act == 2:
        sure_on, sure_off = z > ez, z < -ez
        return np.where(z > 0, E, 0.0), np.where(sure_on, eE, np.where(sure_off, 0.0, np.abs(E) + eE))
    return E, eE


def step_float64(weights, biases, acts, x0, t, eta, mu, vw=None, vb=None):
    """One step in float64 numpy on the float32 input rows x0 [B][K0] and targets t [B][n_out], from the momentum vw, vb (zero
    when None) -> a namespace of values (act, loss, delta, G, g, vw, vb, weights, biases; layer-indexed as train's) and, under
    the same names with the prefix e_, the bound on |C model - float64| of each, derived as follows.

    A float chain of K fmaf terms from a start s differs from the exact s + sum x w by at most gamma_{K+1} (|s| + sum |x| |w|)
    (Higham, Accuracy and Stability, section 3.1; gamma_n = n u / (1 - n u), u = 2^-24); with the factors themselves off by ex
    and ew the exact sum moves by at most sum (|x| ew + |w| ex + ex ew) (the product rule), and the magnitudes under gamma are at
    most |x| + ex, |w| + ew.  Through a sigmoid an error e becomes e / 4 + 2^-22 (tests/dnn_model.py); ReLU and the identity are
    1-Lipschitz.  A single float operation adds u times its result's magnitude (_rounded).  The double sums of the loss add
    gamma64 terms that are below 2^-40 of the float terms and are covered by the factor 1 + 2^-30 on the loss bound."""
    n = len(weights)
    W = [w.astype(np.float64) for w in weights]
    b = [v.astype(np.float64) for v in biases]
    B = x0.shape[0]
    a, ea, z, ez = [x0.astype(np.float64)], [np.zeros(x0.shape)], [None], [None]
    for l in range(1, n + 1):
        K = W[l - 1].shape[1]
        zz = a[l - 1] @ W[l - 1].T + b[l - 1]
        e = _gamma(K + 1) * (np.abs(b[l - 1])[None, :] + (np.abs(a[l - 1]) + ea[l - 1]) @ np.abs(W[l - 1]).T) + ea[l - 1] @ np.abs(W[l - 1]).T
        z.append(zz), ez.append(e)
        if acts[l - 1] == 1:
            a.append(1.0 / (1.0 + np.exp(-np.clip(zz, -700.0, 700.0)))), ea.append(e / 4 + M.SIGMOID_ABS)
        elif acts[l - 1] == 2:
            a.append(np.maximum(zz, 0.0)), ea.append(e)
        else:
            a.append(zz), ea.append(e)
    t = t.astype(np.float64)
    n_out = t.shape[1]
    err = a[n] - t
    e_err = _rounded(err, ea[n])
    loss = 0.5 * np.sum(err * err)
    e_loss = 0.5 * np.sum(_product(err, e_err, err, e_err) + _gamma(n_out + 1) * (np.abs(err) + e_err) ** 2) * (1 + 2.0 ** -30)
    delta, e_delta = [None] * (n + 1), [None] * (n + 1)
    delta[n], e_delta[n] = _delta64(err, e_err, a[n], ea[n], z[n], ez[n], acts[n - 1])
    G, e_G, g, e_g = [None] * (n + 1), [None] * (n + 1), [None] * (n + 1), [None] * (n + 1)
    for l in range(n, 0, -1):
        d, ed, x, ex = delta[l], e_delta[l], a[l - 1], ea[l - 1]
        G[l] = d.T @ x
        e_G[l] = np.abs(d).T @ ex + ed.T @ np.abs(x) + ed.T @ ex + _gamma(B + 1) * ((np.abs(d) + ed).T @ (np.abs(x) + ex))
        g[l] = d.sum(axis=0)
        e_g[l] = ed.sum(axis=0) + _gamma(B + 1) * (np.abs(d) + ed).sum(axis=0)
        if l > 1:
            N = W[l - 1].shape[0]
            E = d @ W[l - 1]
            eE = ed @ np.abs(W[l - 1]) + _gamma(N + 1) * ((np.abs(d) + ed) @ np.abs(W[l - 1]))
            delta[l - 1], e_delta[l - 1] = _delta64(E, eE, x, ex, z[l - 1], ez[l - 1], acts[l - 2])
    eta, mu = float(eta), float(mu)
    out = SimpleNamespace(act=a, e_act=ea, loss=loss, e_loss=e_loss, delta=delta, e_delta=e_delta, G=G, e_G=e_G, g=g, e_g=e_g,
                          weights=[], e_weights=[], biases=[], e_biases=[], vw=[], e_vw=[], vb=[], e_vb=[])
    for l in range(1, n + 1):
        for grad, e_grad, w, v0, names in ((G[l], e_G[l], W[l - 1], None if vw is None else vw[l - 1], ("vw", "weights")),
                                           (g[l], e_g[l], b[l - 1], None if vb is None else vb[l - 1], ("vb", "biases"))):
            v0 = np.zeros(grad.shape) if v0 is None else v0.astype(np.float64)  # the same float32 momentum in both: no error
            mv, e_mv = mu * v0, _rounded(mu * v0, 0.0)
            v1, e_v1 = mv + grad, _rounded(mv + grad, e_mv + e_grad)
            ev, e_ev = eta * v1, _rounded(eta * v1, abs(eta) * e_v1)
            w1, e_w1 = w - ev, _rounded(w - ev, e_ev)
            getattr(out, names[0]).append(v1), getattr(out, "e_" + names[0]).append(e_v1)
            getattr(out, names[1]).append(w1), getattr(out, "e_" + names[1]).append(e_w1)
    return out
