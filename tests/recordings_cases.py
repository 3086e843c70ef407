"""Test infrastructure: the recordings and tap sets of tests/test_recordings_cpu.py and tests/test_gpu_recordings.py (DESIGN.md
5.20), and the model's results for them, computed once per process.

chunk = 1600 samples (20 frames).  The lengths: 100 (skipped), 320, 1000 (T = 0, S % 80 != 0), 1600 (T = 1, R = 0: the last chunk
is 320 samples that yield nothing), 1640 (R < 80), 3200 + 1234, 4800, 16 000 + 57; by hand: one whose first 2000 samples are
zero (a whole zero chunk, and the zero-frame gate inside the next), one all zero (factor inf), one quiet with two spikes of
+-30 000 (the levelled product leaves int16 and wraps)."""
import functools

import numpy as np

from speech_enhancement_amd import corpus
from tests import recordings_model as M

CHUNK = 1600
LEVEL = 3000.0
LENGTHS = (100, 320, 1000, 1600, 1640, 3200 + 1234, 4800, 16000 + 57)
LONGEST = LENGTHS.index(max(LENGTHS))


@functools.lru_cache(maxsize=None)
def recordings():
    xs = [corpus.synth_utterance(11 + k, L) for k, L in enumerate(LENGTHS)]
    lead = corpus.synth_utterance(7, 5000)
    lead[:2000] = 0
    rng = np.random.default_rng(20141106)
    quiet = rng.integers(-3, 4, 3000).astype(np.int16)
    quiet[1500], quiet[1700] = 30000, -30000
    xs += [lead, np.zeros(2400, np.int16), quiet]
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def tap_sets():
    rng = np.random.default_rng(255)
    sets = {"none": None, "one": np.ones(1, np.float32)}
    for k in (33, 300, 4096):
        sets[str(k)] = (rng.standard_normal(k) / 4).astype(np.float32)
    return sets


@functools.lru_cache(maxsize=None)
def stitched(level=LEVEL):
    """per recording (des, factor, status) before the band-pass: the model over the oracle's etsi_denoise"""
    from oracle import oracle as O
    den = M.oracle_denoise(O.Oracle())
    return tuple(M.denoise_recording(x, CHUNK, level, None, den) for x in recordings())


def expected(name, level=LEVEL, only=None):
    """the model's audio for tap set `name` (of recording `only`, or of all)"""
    taps = tap_sets()[name]
    idx = range(len(recordings())) if only is None else [only]
    out = []
    for r in idx:
        des, _, status = stitched(level)[r]
        out.append(des if taps is None or status else M.fir(des, taps))
    return out
