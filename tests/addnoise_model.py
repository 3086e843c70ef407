"""A numpy model of addnoise() (enhancement_extract_subband_linux/cpp/extractwav.cpp:6-35) as g++ on x86-64 compiles it, and
the inputs the training-set tests share.  Independent of the library: tests/addnoise_restatement.c pins it to what the compiler
does with the reference's expression shapes (tests/test_trainset_cpu.py), the GPU tests compare the kernels against it.

  sums    two float accumulators, for every sample in order  s = float32 (float64 (s) + x * x)  (x * x an integer < 2^31, the
          double sum exact, so each step is one correctly rounded float addition)
  gain    sqrt ((pure / noise) / float32 (pow (10.0, db / 10.0))) in float32
  scaled  (short)((float) noise[i] * gain), DEFINED as: int32 truncating toward zero, low 16 bits kept; NaN or a product of
          magnitude >= 2^31 give 0
  noisy   low 16 bits of clean[i] + scaled[i]
"""
import math

import numpy as np

from speech_enhancement_amd import corpus


def sum_in_order(x):
    sq = (np.asarray(x, dtype=np.int64) ** 2).astype(np.float64)
    s = np.float32(0.0)
    for v in sq:
        s = np.float32(np.float64(s) + v)
    return s


def snr_lin(db):
    assert int(db) == db
    return np.float32(math.pow(10.0, int(db) / 10.0))


def gain_of(pure, noise, db):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((np.float32(pure) / np.float32(noise)) / snr_lin(db), dtype=np.float32)


def to_short(p):
    """The conversion rule above on a float32 array."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(p) < np.float32(2147483648.0)      # False for NaN
    v = np.zeros(p.shape, np.int64)
    v[ok] = np.trunc(p[ok].astype(np.float64)).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16)


def scale_and_mix(clean, noise, gain):
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.asarray(noise, dtype=np.int16).astype(np.float32) * np.float32(gain)
    scaled = to_short(prod)
    noisy = ((np.asarray(clean, np.int16).astype(np.int64) + scaled.astype(np.int64)) & 0xFFFF).astype(np.uint16).view(np.int16)
    return scaled, noisy, prod


def addnoise(clean, noise, db):
    """-> dict: sums float32[2] (pure, noise), gain float32, scaled int16[L], noisy int16[L], prod float32[L]."""
    pure, nsum = sum_in_order(clean), sum_in_order(noise)
    gain = gain_of(pure, nsum, db)
    scaled, noisy, prod = scale_and_mix(clean, noise, gain)
    return dict(sums=np.array([pure, nsum], np.float32), gain=gain, scaled=scaled, noisy=noisy, prod=prod)


# ---------------------------------------------------------------------------------------------------------------------
# the shared inputs: five noise recordings and ten utterances.  Sizes: 320 is the shortest the pipeline takes; 477, 1677 and 8005
# are no multiple of 8 (the packed layout's pad), of 256 (the sums kernel's tile) or of 2048 (the scaling kernel's chunk); ten
# utterances make two groups of the sums kernel; 33001 samples make the scaling kernel's blocks loop a second time.
# ---------------------------------------------------------------------------------------------------------------------
def recordings():
    third = lambda u, n: (corpus.synth_utterance(u, n).astype(np.int32) // 3).astype(np.int16)
    return [third(300, 12000), third(301, 9000), np.zeros(2000, np.int16),
            (corpus.synth_utterance(303, 1600).astype(np.int32) // 40).astype(np.int16), third(304, 34000)]


def cases():
    """-> list of dicts: clean int16[L], rec, off, db, tag."""
    out = []
    plan = [(320, 0, 1000, 0, "silent clean"), (477, 1, 137, -5, "odd offset"), (1677, 0, 12000 - 1677, 0, "last offset that fits"),
            (4800, 1, 9000 - 4800, -5, "last offset that fits"), (8005, 0, 1001, 0, "plain")]
    for i, (L, rec, off, db, tag) in enumerate(plan):
        out.append(dict(clean=corpus.synth_utterance(200 + i, L), rec=rec, off=off, db=db, tag=tag))
    out.append(dict(clean=corpus.synth_utterance(206, 1600), rec=2, off=3, db=-5, tag="silent noise"))
    loud = np.clip(corpus.synth_utterance(207, 1600).astype(np.int32) * 4, -32768, 32767).astype(np.int16)
    out.append(dict(clean=loud, rec=3, off=0, db=-5, tag="wrap"))
    out.append(dict(clean=corpus.synth_utterance(208, 2400), rec=1, off=0, db=0, tag="plain"))
    out.append(dict(clean=corpus.synth_utterance(209, 333), rec=0, off=4001, db=-5, tag="plain"))
    out.append(dict(clean=corpus.synth_utterance(211, 33001), rec=4, off=999, db=0, tag="long"))
    return out


def stretch(recs, case):
    L = len(case["clean"])
    return recs[case["rec"]][case["off"]:case["off"] + L]


def noise_layout(recs):
    """All recordings back to back, and each one's base index."""
    base = np.concatenate(([0], np.cumsum([len(r) for r in recs])[:-1])).astype(np.int64)
    return np.concatenate(recs), base
