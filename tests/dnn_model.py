"""Test infrastructure: the model of the DNN mask estimator.  The network, its splice and the two
elementary functions are the plain-C program tests/dnn_model_driver.c, which includes csrc/dnn_math.h -- the header the device
code includes -- and is built here with gcc -O2 -ffp-contract=off; the cochleagram's energies are numpy int64.  The GPU results
must equal this model bit for bit as values.

Independent of it: splice_numpy (the splice in numpy float32) and torch_float64 (the layers as a float64 nn.Sequential) with the
error bound that follows from the weights, for the cross-check of the C model itself (tests/test_dnn_cpu.py).
"""
import atexit
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "dnn_model_driver.c")
U = 2.0 ** -24  # unit roundoff of float32
SIGMOID_ABS = 2.0 ** -22  # |sigmoid_float - sigmoid_double|: an exponential good to 2^-23 relative, one add, one divide

_built = {}


def build_driver(sanitize=False):
    """the driver's path; built once per process (sanitize: with -fsanitize=address,undefined at -O1)"""
    if sanitize not in _built:
        cc = shutil.which("gcc")
        assert cc, "gcc is needed to build tests/dnn_model_driver.c"
        d = tempfile.mkdtemp(prefix="dnn_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "dnn_model_driver")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", CSRC, SOURCE, "-o", exe,
                                                                                                    "-lm", "-lpthread"])
        _built[sanitize] = (exe, d)
    return _built[sanitize]


def _run(args, sanitize=False, timeout=600):
    exe, _ = build_driver(sanitize)
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0 and not run.stderr, f"dnn_model_driver exited with {run.returncode}:\n{run.stderr[-2000:]}"
    return run.stdout


def sweep(which):
    """'lnf_sweep' or 'exp_sweep' -> dict of the figures the driver prints (floats; `at` values as strings)"""
    out = {}
    key = None
    for tok in _run([which]).split():
        k, v = tok.split("=")
        if k == "at":
            out[key + "_at"] = v
        else:
            key = k
            out[k] = float(v)
    return out


def make_net(context, shift, scale, weights, biases, acts):
    weights = [np.ascontiguousarray(w, np.float32) for w in weights]
    return SimpleNamespace(context=int(context), shift=np.ascontiguousarray(shift, np.float32), scale=np.ascontiguousarray(scale, np.float32),
                           weights=weights, biases=[np.ascontiguousarray(b, np.float32) for b in biases], acts=[int(a) for a in acts],
                           dims=[weights[0].shape[1]] + [w.shape[0] for w in weights])


def wide_floats(rng, shape, spread=12):
    """random floats of either sign over a magnitude range of 2^spread: the order of a sum of them matters"""
    return (rng.choice([-1.0, 1.0], size=shape) * rng.uniform(1.0, 2.0, size=shape) * 2.0 ** rng.uniform(-spread / 2, spread / 2, size=shape)
            ).astype(np.float32)


def random_net(seed, context, widths, acts, spread=12):
    """a seeded network 64 (2 C + 1) -> widths[0] -> .. with weights, biases, shift and scale spread over 2^spread"""
    rng = np.random.default_rng(seed)
    k0 = 64 * (2 * context + 1)
    dims = [k0] + list(widths)
    weights = [wide_floats(rng, (dims[l + 1], dims[l]), spread) / np.float32(np.sqrt(dims[l])) for l in range(len(widths))]
    biases = [wide_floats(rng, dims[l + 1], spread) for l in range(len(widths))]
    return make_net(context, wide_floats(rng, k0, spread), wide_floats(rng, k0, spread), weights, biases, acts)


def forward(net, feats_list, decoy=False, sanitize=False):
    """the C model on a list of feature arrays [F_u][64] -> list of [F_u][dims[-1]] float32"""
    feats_list = [np.ascontiguousarray(f, np.float32).reshape(-1, 64) for f in feats_list]
    _, d = build_driver(sanitize)
    src, dst = os.path.join(d, "net.bin"), os.path.join(d, "out.bin")
    n = len(net.weights)
    with open(src, "wb") as f:
        f.write(np.asarray([net.context, n] + list(net.dims) + list(net.acts) + [len(feats_list)] + [x.shape[0] for x in feats_list],
                           np.int32).tobytes())
        f.write(net.shift.tobytes() + net.scale.tobytes())
        for w, b in zip(net.weights, net.biases):
            f.write(w.tobytes() + b.tobytes())
        for x in feats_list:
            f.write(x.tobytes())
    _run(["forward", src, dst] + (["decoy"] if decoy else []), sanitize)
    flat = np.fromfile(dst, np.float32).reshape(-1, net.dims[-1])
    cuts = np.cumsum([0] + [x.shape[0] for x in feats_list])
    return [flat[cuts[i]:cuts[i + 1]].copy() for i in range(len(feats_list))]


def _map(mode, values, *extra):
    values = np.ascontiguousarray(values, np.float32)
    _, d = build_driver()
    src, dst = os.path.join(d, "map_in.bin"), os.path.join(d, "map_out.bin")
    values.tofile(src)
    _run([mode, src, dst] + list(extra))
    return np.fromfile(dst, np.float32).reshape(values.shape)


def lnf(y):
    """sea_lnf of csrc/dnn_math.h on an array of floats >= 1"""
    return _map("lnf", y)


def act(z, kind):
    """sea_dnn_act of csrc/dnn_math.h"""
    return _map("act", z, int(kind))


def frame_energies(sub64):
    """[64][L] int16 -> int64 [F][64]: the exact sum of the 320 squares of every frame, F = (L - 320) // 160 + 1"""
    s = np.asarray(sub64).astype(np.int64)
    L = s.shape[1]
    F = (L - 320) // 160 + 1
    csum = np.concatenate([np.zeros((64, 1), np.int64), np.cumsum(s * s, axis=1)], axis=1)
    starts = 160 * np.arange(F)
    return (csum[:, starts + 320] - csum[:, starts]).T.copy()


def cochleagram(sub64):
    """the model's features: sea_lnf ((float)(E + 1)); numpy converts int64 to float32 by round-to-nearest-even, as C does"""
    return lnf((frame_energies(sub64) + 1).astype(np.float32))


def splice_numpy(net, feats):
    """the network's input rows in numpy float32, independently of the driver: a float add, then a float multiply"""
    feats = np.ascontiguousarray(feats, np.float32).reshape(-1, 64)
    F, C = feats.shape[0], net.context
    idx = np.clip(np.arange(F)[:, None] + np.arange(-C, C + 1)[None, :], 0, F - 1)
    x = feats[idx].reshape(F, 64 * (2 * C + 1))
    return ((x + net.shift[None, :]).astype(np.float32) * net.scale[None, :]).astype(np.float32)


def torch_float64(net, x0):
    """the layers as a float64 nn.Sequential on the float32 input rows x0 -> (output float64 [F][n_out], bound [F][n_out]).

    The bound on |C model - float64| follows from the weights.  A chain acc = b, acc = fmaf (x[k], W[k], acc) over K terms
    performs K roundings, so (Higham, Accuracy and Stability, section 3.1) it differs from the exact b + sum x W by at most
    gamma_{K+1} (|b| + sum |x| |W|), gamma_n = n u / (1 - n u), u = 2^-24; we keep the n = K + 1 of the usual statement.  With the
    inputs themselves off by e_in the exact sum moves by at most sum e_in |W|, and the |x| of the first term are at most the
    float64 values' magnitudes plus e_in.  Through the sigmoid an error e becomes e / 4 (its largest slope) + SIGMOID_ABS
    (tests/test_dnn_cpu.py measures that figure on every argument); ReLU and the identity are 1-Lipschitz and exact."""
    import torch
    import torch.nn as nn
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
    with torch.no_grad():
        y = seq(torch.from_numpy(x0.astype(np.float64))).numpy()
        # the bound, layer by layer, from the float64 activations
        x = x0.astype(np.float64)
        e = np.zeros_like(x)
        for w, b, a in zip(net.weights, net.biases, net.acts):
            w64, b64 = np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64))
            K = w.shape[1]
            gamma = (K + 1) * U / (1 - (K + 1) * U)
            z = x @ w.astype(np.float64).T + b.astype(np.float64)
            e = gamma * (b64[None, :] + (np.abs(x) + e) @ w64.T) + e @ w64.T
            if a == 1:
                x, e = 1.0 / (1.0 + np.exp(-np.clip(z, -700.0, 700.0))), e / 4 + SIGMOID_ABS
            elif a == 2:
                x = np.maximum(z, 0.0)
            else:
                x = z
    return y, e
