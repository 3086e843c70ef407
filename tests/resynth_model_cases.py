"""tests/resynth_model_cases.py -- TEST INFRASTRUCTURE ONLY: the inputs and the thresholds that
tests/test_resynth_model_cpu.py (oracle vs the float64 model of tests/gammatone_model.py) and
tests/test_gpu_resynth_model.py (kernels vs the same model) share, so that both judge exactly the same material.

Lengths sit around the resynthesis kernel's 16-sample tile (320, 321, 335, 336, 337, 479, 480, 481, 127*16+1) and its
8-rows-in-flight pipeline, masks leave [0, 1) (zero rows, entries of exactly 0.5, negative entries, entries in (1, 3],
all ones, all zeros), amplitudes go up to full scale and, once, past it: `loud_wrap` with a mask in (1, 1.5] drives the
channel sum beyond int16 so that the (short) wrap of extractwav.cpp:120-121 is exercised.

THRESHOLDS.  Measured on the CPU, restatement (oracle/resynth_oracle.c) against the model, on exactly these inputs; the
figures are in the module docstring of tests/test_resynth_model_cpu.py.  The GPU tests use the same thresholds: the
kernels are bit-identical to the restatement, so no device margin is added.
"""
import functools

import numpy as np

from speech_enhancement_amd import corpus
from tests import gammatone_model as G

# float streams (gammatone): max |delta| / channel peak.  4 x the measured worst (1.2525e-5, all 64 channels, the four
# inputs of stream_inputs()); must stay <= 1/10 of the smallest mutant distance on the same inputs (1.9e-2).
STREAM_TOL = 5.01e-5
# int16: the project's own limit in wrapped arithmetic (measured: 1)
INT16_MAX_LSB = 2
# share of differing samples, per case family: 2 x the worst per-case share measured on the CPU; never above 5 %
SHARE_CAP = {
    "resynth_soft": 2 * 0.022875,          # measured worst: loud_wrap_48000
    "resynth_ibm": 2 * 0.018938,           # loud_wrap_48000
    "resynth_soft_l160": 2 * 0.022917,     # loud_wrap_48000
    "resynth_ibm_l160": 2 * 0.018938,      # loud_wrap_48000
    "subband": 2 * 0.000361,               # loud_1600
}
SHARE_CEILING = 0.05
TABLE_RTOL = 1e-5          # float32 rounding of a double expression (measured <= 1.0e-6)
DERIVATION_RTOL = 1e-10
MIN_PEAK = 1000            # non-vacuity: every non-silent case's model output reaches this


def family(binary, frames_l_over_160):
    return "resynth_" + ("ibm" if binary else "soft") + ("_l160" if frames_l_over_160 else "")


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _square(L, period=40):
    return np.where((np.arange(L) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)


def _loud(u, L, factor):
    return np.clip(corpus.synth_utterance(u, L).astype(np.int64) * factor, -32768, 32767).astype(np.int16)


def _loud_passage(u, L, lo=6400, hi=8000, factor=8):
    """a corpus utterance with one passage far too loud: with a mask above 1 the channel sum leaves int16 there"""
    x = corpus.synth_utterance(u, L).astype(np.int64)
    x[lo:hi] *= factor
    return np.clip(x, -32768, 32767).astype(np.int16)


def _burst(u, L, n_on=400):
    x = np.zeros(L, np.int16)
    x[:n_on] = _loud(u, n_on, 4)
    return x


def stream_inputs():
    """float inputs of 16 000 samples for gammaToneFilter, every channel: corpus, wideband, a full-scale square wave, a
    burst followed by silence (the filter's tail decays through the whole float range)"""
    n = 16000
    return {"corpus": corpus.synth_utterance(31, n).astype(np.float32), "wideband": corpus.synth_wideband(2, n).astype(np.float32),
            "square": _square(n).astype(np.float32), "burst": _burst(33, n).astype(np.float32)}


def _mask(kind, F, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((F, 64)).astype(np.float32)
    if kind == "ones":
        m[:] = 1.0
    elif kind == "zeros":
        m[:] = 0.0
    elif kind == "sparse_negatives":
        # a few units kept ((0.5, 1]: they survive the IBM threshold too), the rest nearly shut: with a full-scale square
        # wave behind it the sum stays inside int16, where the share of truncation-boundary disagreements is meaningful
        m *= np.float32(0.1)
        hi = rng.random((F, 64)) < 0.2
        m[hi] = (np.float32(1.0) - np.float32(0.5) * rng.random((F, 64)).astype(np.float32))[hi]
        m[rng.random((F, 64)) < 0.3] *= np.float32(-1.0)
    elif kind == "above_one":
        m = (np.float32(1.0) + np.float32(2.0) * m).astype(np.float32)          # (1, 3]
        m[m <= 1.0] = 3.0
    elif kind == "just_above_one":
        m = (np.float32(1.5) - np.float32(0.5) * m).astype(np.float32)          # (1, 1.5]
    elif kind == "halves":
        m[rng.random((F, 64)) < 0.4] = 0.5          # exactly at the IBM threshold: skipped by '> 0.5'
    elif kind == "zero_rows":
        m[::2] = 0.0
    elif kind == "mixed":
        m[rng.random((F, 64)) < 0.15] = 0.5
        m[rng.random((F, 64)) < 0.15] *= np.float32(-1.0)
        m[rng.random((F, 64)) < 0.10] += np.float32(1.5)
        m[3::7] = 0.0
    else:
        assert kind == "random"
    return np.ascontiguousarray(m, dtype=np.float32)


# name, length, input, mask kind, silent.  corpus seeds avoid multiples of 5 (those start with 400 zeros).
_RESYNTH = (
    ("corpus_ones_320", 320, lambda L: corpus.synth_utterance(21, L), "ones", False),
    ("wideband_random_321", 321, lambda L: corpus.synth_wideband(3, L), "random", False),
    ("square_sparse_negatives_335", 335, _square, "sparse_negatives", False),
    ("corpus_above_one_336", 336, lambda L: corpus.synth_utterance(22, L), "above_one", False),
    ("loud_halves_337", 337, lambda L: _loud(23, L, 6), "halves", False),
    ("wideband_zeros_479", 479, lambda L: corpus.synth_wideband(4, L), "zeros", True),
    ("corpus_zero_rows_480", 480, lambda L: corpus.synth_utterance(24, L), "zero_rows", False),
    ("wideband_ones_481", 481, lambda L: corpus.synth_wideband(7, L), "ones", False),
    ("corpus_mixed_2033", 127 * 16 + 1, lambda L: corpus.synth_utterance(26, L), "mixed", False),
    ("wideband_halves_3277", 3277, lambda L: corpus.synth_wideband(5, L), "halves", False),
    ("burst_ones_8000", 8000, lambda L: _burst(27, L), "ones", False),
    ("loud_wrap_48000", 48000, lambda L: _loud_passage(28, L), "just_above_one", False),
)
WRAP_CASE = "loud_wrap_48000"


@functools.lru_cache(maxsize=None)
def resynth_cases(frames_l_over_160=False):
    """tuple of (name, x int16 [L], mask float32 [F][64], silent)"""
    out = []
    for i, (name, L, make, kind, silent) in enumerate(_RESYNTH):
        F = G.Model.frame_count(L, frames_l_over_160)
        out.append((name, np.ascontiguousarray(make(L), dtype=np.int16), _mask(kind, F, 1000 + i), silent))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def resynth_model(frames_l_over_160, binary):
    """the default model's float64 channel sum of every case of resynth_cases(), computed once per process"""
    return tuple(G.resynth(x, m, binary, frames_l_over_160) for _, x, m, _ in resynth_cases(frames_l_over_160))


@functools.lru_cache(maxsize=None)
def subband_cases():
    """tuple of (name, x int16 [L], check_peak).  One sample gives the hair cell's rest rate (about 50) whatever the input."""
    return (("square_1", _square(1), False), ("square_15", _square(15, 8), True), ("square_16", _square(16, 8), True),
            ("square_17", _square(17, 8), True), ("corpus_4800", corpus.synth_utterance(81, 4800), True),
            ("wideband_3277", corpus.synth_wideband(6, 3277), True), ("square_2033", _square(2033), True),
            ("loud_1600", _loud(82, 1600, 10), True), ("burst_8000", _burst(83, 8000), True))


@functools.lru_cache(maxsize=None)
def subband_model():
    return tuple(G.subband(x) for _, x, _ in subband_cases())


def check_int16(got, model_f64, fam, what):
    """got (int16) against the cast of the model's float64 values: both limits of the family; prints the figures first"""
    want = G.cast_short(model_f64)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.int16, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    lsb, share = G.int16_figures(got, want)
    cap = SHARE_CAP[fam]
    print(f"{what}: n={got.size} max|d|={lsb} LSB, {share * 100:.3f} % of samples differ (cap {cap * 100:.3f} %)")
    assert cap <= SHARE_CEILING
    assert lsb <= INT16_MAX_LSB, f"{what}: max |delta| {lsb} LSB against the float64 model"
    assert share <= cap, f"{what}: {share * 100:.3f} % of samples differ from the float64 model (cap {cap * 100:.3f} %)"
    return lsb, share
