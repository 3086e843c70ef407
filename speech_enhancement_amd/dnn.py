"""The DNN mask estimator over libsea_mi355x.so (csrc/dnn_kernel.hip, csrc/dnn_capi.hip): noisy
16 kHz audio -> 64 subband streams -> cochleagram -> feed-forward network -> mask rows -> resynthesis, the reference's headline
workflow with its network and features on the GPU.

  DnnMask                  the network: context, shift, scale, weights, biases, activations; from_torch, load, save; normaliser
                           (shift and scale from training features), pull (the trained weights back from the device)
  DnnTrainer               minibatch SGD with momentum on the device, in place in a DnnMask's weights
  cochleagram(sub64)       one utterance's [64][L] subband streams -> [F][64] features, F = (L - 320) // 160 + 1
  cochleagram_utterances   subbands + cochleagram for a list of int16 utterances (with make_trainset's `noisy` outputs these
                           are the training set's inputs; its `irm` outputs are the targets, row for row)
  dnn_forward              the network on lists of feature rows
  dnn_enhance_utterances   the whole chain on the device: audio in, enhanced audio (and the mask) out

All arguments are host arrays; all compute is in the HIP library.  Every result is pinned bit for bit by the plain-C model
of tests/dnn_model_driver.c; there is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib
from .engine import _np_ptr

DNN_NCHAN = 64
DNN_ACTS = {"identity": 0, "sigmoid": 1, "relu": 2}


def _ptr_array(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _i16_list(xs):
    xs = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in xs]
    return xs, (ctypes.c_long * max(len(xs), 1))(*[x.size for x in xs])


def dnn_rows(length):
    """mask / feature rows of an utterance of `length` samples: (length - 320) // 160 + 1 (0 below one frame)"""
    return (int(length) - 320) // 160 + 1 if length >= 320 else 0


class DnnMask:
    """A feed-forward mask network on the current device.  context C (0..15): the input row is the 2 C + 1 feature rows around
    a frame, clamped to the utterance, (feat + shift) * scale; weights[l] [out][in] as torch.nn.Linear.weight, biases[l] [out],
    acts[l] 0 / 1 / 2 or "identity" / "sigmoid" / "relu".  Values that are not finite, a first layer whose input is not
    64 (2 C + 1) wide and dimensions above 4096 are refused."""

    def __init__(self, context, shift, scale, weights, biases, acts):
        self._handle = None
        self.context = int(context)
        self.shift = np.ascontiguousarray(shift, dtype=np.float32).reshape(-1)
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        self.acts = [DNN_ACTS[a] if isinstance(a, str) else int(a) for a in acts]
        n = len(self.weights)
        if n == 0 or len(self.biases) != n or len(self.acts) != n:
            raise ValueError("DnnMask: one weight matrix, one bias vector and one activation per layer")
        if any(w.ndim != 2 for w in self.weights):
            raise ValueError("DnnMask: a weight matrix is [out][in]")
        self.dims = [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]
        k0 = DNN_NCHAN * (2 * self.context + 1)
        if self.shift.size != k0 or self.scale.size != k0:
            raise ValueError(f"DnnMask: shift and scale hold {k0} values at context {self.context}")
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.shape[1] != self.dims[l] or b.size != w.shape[0]:
                raise ValueError(f"DnnMask: layer {l} is {w.shape} with {b.size} biases after {self.dims[l]} values")
        lib = _lib.load()
        dims = (ctypes.c_int * (n + 1))(*self.dims)
        acts_c = (ctypes.c_int * n)(*self.acts)
        handle = lib.sea_dnn_create(self.context, _np_ptr(self.shift), _np_ptr(self.scale), n, dims, _ptr_array(self.weights),
                                    _ptr_array(self.biases), acts_c)
        if not handle:
            _lib.check(1, "sea_dnn_create")
        self._handle = handle

    def close(self):
        if self._handle:
            _lib.load().sea_dnn_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_out(self):
        return self.dims[-1]

    @classmethod
    def from_torch(cls, module, context, shift, scale):
        """An nn.Sequential of Linear (with bias), Sigmoid and ReLU modules; anything else is refused."""
        import torch.nn as nn
        if not isinstance(module, nn.Sequential):
            raise TypeError(f"DnnMask.from_torch: an nn.Sequential, not {type(module).__name__}")
        weights, biases, acts = [], [], []
        for layer in module:
            if isinstance(layer, nn.Linear):
                if layer.bias is None:
                    raise TypeError("DnnMask.from_torch: a Linear without bias")
                weights.append(layer.weight.detach().cpu().numpy().astype(np.float32))
                biases.append(layer.bias.detach().cpu().numpy().astype(np.float32))
                acts.append(0)
            elif type(layer) in (nn.Sigmoid, nn.ReLU):
                if not acts or acts[-1] != 0:
                    raise TypeError(f"DnnMask.from_torch: {type(layer).__name__} does not follow a Linear")
                acts[-1] = 1 if isinstance(layer, nn.Sigmoid) else 2
            else:
                raise TypeError(f"DnnMask.from_torch: {type(layer).__name__} is not Linear, Sigmoid or ReLU")
        return cls(context, shift, scale, weights, biases, acts)

    def pull(self):
        """Refresh weights and biases from the device (a DnnTrainer updates them there), so that save() writes the trained
        network.  The arrays are new ones: the constructor may have kept the caller's own."""
        weights, biases = [np.zeros_like(w) for w in self.weights], [np.zeros_like(b) for b in self.biases]
        _lib.check(_lib.load().sea_dnn_get_params(self._handle, _ptr_array(weights), _ptr_array(biases)), "sea_dnn_get_params")
        self.weights, self.biases = weights, biases
        return self

    @staticmethod
    def normaliser(feats_list, context):
        """(shift, scale) for the constructor from training features [F_u][64]: per channel c the mean and the standard
        deviation over all rows in float64, shift[k] = -mean[k & 63], scale[k] = 1 / std[k & 63], rounded to float32 once.  A
        channel that does not vary is refused."""
        rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, DNN_NCHAN) for f in feats_list], axis=0)
        if rows.shape[0] == 0:
            raise ValueError("DnnMask.normaliser: no feature row")
        mean, std = rows.mean(axis=0), rows.std(axis=0)
        if not np.all(np.isfinite(mean)) or not np.all(std > 0):
            raise ValueError(f"DnnMask.normaliser: channel {int(np.argmin(std > 0))} does not vary (or a feature is not finite)")
        reps = 2 * int(context) + 1
        return np.tile(-mean, reps).astype(np.float32), np.tile(1.0 / std, reps).astype(np.float32)

    def save(self, path):
        arrays = dict(context=np.int32(self.context), shift=self.shift, scale=self.scale, acts=np.asarray(self.acts, np.int32))
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            arrays[f"W{l}"], arrays[f"b{l}"] = w, b
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            n = len(z["acts"])
            return cls(int(z["context"]), z["shift"], z["scale"], [z[f"W{l}"] for l in range(n)], [z[f"b{l}"] for l in range(n)],
                       [int(a) for a in z["acts"]])


class DnnTrainer:
    """Minibatch SGD with momentum on 1/2 sum (y - t)^2 (Kaldi nnet1's MSE), on the device, in place in `model`'s weights: the
    model serves dnn_forward and dnn_enhance_utterances between and after runs, and model.pull() fetches the weights.
    feats_list[u] [F_u][64] (cochleagram_utterances of make_trainset's `noisy`), targets_list[u] [F_u][model.n_out] (its `irm`).
    The whole set is uploaded once.  lr multiplies the gradient SUMMED over the minibatch, as in nnet1: a rate meant for the mean
    gradient is lr / batch.  Every value is pinned bit for bit by tests/dnn_train_model_driver.c."""

    WHAT = {"act": 0, "delta": 1, "wgrad": 2, "bgrad": 3, "wmom": 4, "bmom": 5}

    def __init__(self, model, feats_list, targets_list, max_batch=1024):
        self._handle = None
        self.model = model
        feats = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, DNN_NCHAN) for f in feats_list]
        targets = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1, model.n_out) for t in targets_list]
        if len(feats) != len(targets) or any(f.shape[0] != t.shape[0] for f, t in zip(feats, targets)):
            raise ValueError("DnnTrainer: one target row per feature row, utterance by utterance")
        self.total_rows = int(sum(f.shape[0] for f in feats))
        self.max_batch = int(max_batch)
        self.last_batch = 0
        n_rows = (ctypes.c_int * max(len(feats), 1))(*[f.shape[0] for f in feats])
        handle = _lib.load().sea_dnn_trainer_create(model._handle, _ptr_array(feats), _ptr_array(targets), n_rows, len(feats),
                                                    self.max_batch)
        if not handle:
            _lib.check(1, "sea_dnn_trainer_create")
        self._handle = handle

    def close(self):
        if self._handle:
            _lib.load().sea_dnn_trainer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, order, batch, lr, momentum=0.0, update=True):
        """Steps over consecutive minibatches of `batch` rows of `order` (global rows; the last minibatch may be shorter) ->
        the loss of every step, float64.  update=False: forward and loss only.  A loss that is not finite raises."""
        order = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
        batch = int(batch)
        losses = np.zeros((order.size + batch - 1) // batch if batch > 0 else 0, np.float64)
        rc = _lib.load().sea_dnn_trainer_run(self._handle, _np_ptr(order), order.size, batch, float(lr), float(momentum),
                                             int(bool(update)), _np_ptr(losses))
        _lib.check(rc, "sea_dnn_trainer_run")
        self.last_batch = order.size - (losses.size - 1) * batch
        return losses

    def epoch(self, seed, batch, lr, momentum=0.0):
        """One pass over the set in the order np.random.default_rng(seed).permutation(total_rows)."""
        return self.run(np.random.default_rng(seed).permutation(self.total_rows), batch, lr, momentum)

    def evaluate(self, batch=None):
        """The summed loss over all rows in natural order, nothing updated (a cross-validation pass)."""
        batch = self.max_batch if batch is None else batch
        return float(self.run(np.arange(self.total_rows), batch, 0.0, 0.0, update=False).sum())

    def read(self, what, layer):
        """The last step's values: "act" a_layer [B][dims[layer]] (layer 0..n), "delta" [B][dims[layer]], "wgrad"
        [dims[layer]][dims[layer - 1]], "bgrad", "wmom", "bmom" (layer 1..n)."""
        code = self.WHAT[what] if isinstance(what, str) else int(what)
        lib = _lib.load()
        dims, layer = self.model.dims, int(layer)
        if not (0 <= code <= 5) or not ((0 if code == 0 else 1) <= layer < len(dims)):
            _lib.check(lib.sea_dnn_trainer_read(self._handle, code, layer, _np_ptr(np.zeros(1, np.float32))), "sea_dnn_trainer_read")
            raise ValueError(f"DnnTrainer.read: what {what!r}, layer {layer}")
        last = self.last_batch
        shape = (last, dims[layer]) if code < 2 else (dims[layer], dims[layer - 1]) if code in (2, 4) else (dims[layer],)
        out = np.zeros(shape, np.float32)
        _lib.check(lib.sea_dnn_trainer_read(self._handle, code, layer, _np_ptr(out)), "sea_dnn_trainer_read")
        return out

    def stage_ms(self, stage):
        """device time in ms of a stage (SEA_DNN_TRAIN_STAGE_* of the header) of the last step of the last run"""
        return float(_lib.load().sea_dnn_trainer_stage_ms(self._handle, int(stage)))


def cochleagram(sub64):
    """One utterance's subband streams [64][L] (int16, as subbband() gives them) -> float32 [F][64]: the natural log of one
    plus the energy of 320-sample frames every 160."""
    sub64 = np.ascontiguousarray(sub64, dtype=np.int16)
    if sub64.ndim != 2 or sub64.shape[0] != DNN_NCHAN:
        raise ValueError("cochleagram: [64][L] subband streams")
    L = sub64.shape[1]
    feats = np.zeros((dnn_rows(L), DNN_NCHAN), np.float32)
    _lib.check(_lib.load().sea_cochleagram64(_np_ptr(sub64), L, _np_ptr(feats)), "sea_cochleagram64")
    return feats


def cochleagram_utterances(xs):
    """A list of int16 utterances (16 kHz, at least 320 samples each) -> the list of their features [F_u][64]."""
    lib = _lib.load()
    xs, lens = _i16_list(xs)
    feats = [np.zeros((dnn_rows(x.size), DNN_NCHAN), np.float32) for x in xs]
    _lib.check(lib.sea_cochleagram_utterances(_ptr_array(xs), lens, len(xs), _ptr_array(feats)), "sea_cochleagram_utterances")
    return feats


def dnn_forward(model, feats_list):
    """The network on a list of feature arrays [F_u][64] -> the list of its outputs [F_u][model.n_out]."""
    lib = _lib.load()
    feats = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, DNN_NCHAN) for f in feats_list]
    n_rows = (ctypes.c_int * max(len(feats), 1))(*[f.shape[0] for f in feats])
    out = [np.zeros((f.shape[0], model.n_out), np.float32) for f in feats]
    _lib.check(lib.sea_dnn_forward(model._handle, _ptr_array(feats), n_rows, len(feats), _ptr_array(out)), "sea_dnn_forward")
    return out


def dnn_enhance_utterances(model, xs, binary=False, masks=False):
    """Noisy int16 utterances in, enhanced int16 utterances out, the network's output as the mask of the 64-band resynthesis;
    nothing but audio crosses the bus.  binary: threshold the mask as resyth_64sub_IBM does.  masks=True: (audio, masks), the
    masks [F_u][64] as the network wrote them."""
    lib = _lib.load()
    xs, lens = _i16_list(xs)
    out = [np.zeros(x.size, np.int16) for x in xs]
    ms = [np.zeros((dnn_rows(x.size), DNN_NCHAN), np.float32) for x in xs] if masks else None
    rc = lib.sea_dnn_enhance_utterances(model._handle, _ptr_array(xs), lens, len(xs), int(bool(binary)), _ptr_array(out),
                                        _ptr_array(ms) if masks else None)
    _lib.check(rc, "sea_dnn_enhance_utterances")
    return (out, ms) if masks else out


def dnn_last_chunks():
    """How many chunks the last list call of this thread was cut into (SEA_DNN_SCRATCH_MB sets the budget)."""
    return int(_lib.load().sea_dnn_last_chunks())
