"""tests/hw64_am_model.py -- TEST INFRASTRUCTURE ONLY: the numpy model of the Hu-Wang estimator's AM labels and final grouping
(computeAM, finalSeg and the binarisation, HuWang.cpp:1146-1494, :99-106, with the tools of :1553-1677) at 16 kHz on the
64-channel bank, that is at the constants of resyth_64sub_IBM/cpp/HuWang.h: NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320,
SAMPLING_FREQUENCY 16000.

The reference's source is the same at both rates and holds no literal channel count or rate in these functions, and so does
the model: the functions of tests/hw25_am_model.py read the bank's constants from their module's globals, so this file loads
a second instance of that module and gives it the 64-band constants, as tests/hw64_pitch_model.py does with the pitch model.
That the instance, which holds no literal, equals the reference on every array of the fixture is the proof that no literal
hides in the reference's stage.  Restated here: the largest pitch am_stage accepts (200, the 25-band model says 100), the
inputs of the fixture and the hand-made cases at [F][64].

tests/test_hw64_am_cpu.py pins the model against tests/golden/hw64_am_golden.npz (tools/gen_hw64_am_golden.py);
tests/test_gpu_hw64_am.py uses it where the fixture holds nothing.  The undefined cases are defined as in
tests/hw25_am_model.py.
"""
import importlib.util
import os

import numpy as np

from tests import hw25_am_model as _A25
from tests import hw64_pitch_model as PM

FS, NCH, HOP, WINDOW, MAX_PITCH = 16000, 64, 160, 320, 200
PI, THETAC, THETAT, THETAE = _A25.PI, _A25.THETAC, _A25.THETAT, _A25.THETAE
MIN_SEG_LENGTH, MAX_SEG, MAX_LEN = _A25.MIN_SEG_LENGTH, _A25.MAX_SEG, _A25.MAX_LEN
FINAL_TOO_MANY_SEGMENTS, AM_TOO_LONG, AM_BAD_PITCH = _A25.FINAL_TOO_MANY_SEGMENTS, _A25.AM_TOO_LONG, _A25.AM_BAD_PITCH
FINAL_STAGES, SAMPLES = _A25.FINAL_STAGES, _A25.SAMPLES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw64_am_golden.npz")
F32 = np.float32
MAX_TAPS = 1120  # SEA_HW64_AM_MAXTAPS


def _second_instance():
    spec = importlib.util.spec_from_file_location("tests._hw25_am_model_at_64_bands", _A25.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.FS, m.NCH, m.HOP, m.WINDOW, m.GOLDEN, m.PM = FS, NCH, HOP, WINDOW, GOLDEN, PM
    return m


_B = _second_instance()
(kaiser_constants, fft_log2, n_at_pow2, twiddles, gout, kaiser_bandpass, block_mean_pitch, am_patt, fft, normalised, am_rate,
 re_segmentation, develope, closure, final_seg, crc32, channel_crcs, sample_index, load_golden, hand_prune, hand_minus2,
 hand_empty, many_final_segments_case) = (
    _B.kaiser_constants, _B.fft_log2, _B.n_at_pow2, _B.twiddles, _B.gout, _B.kaiser_bandpass, _B.block_mean_pitch, _B.am_patt,
    _B.fft, _B.normalised, _B.am_rate, _B.re_segmentation, _B.develope, _B.closure, _B.final_seg, _B.crc32, _B.channel_crcs,
    _B.sample_index, _B.load_golden, _B.hand_prune, _B.hand_minus2, _B.hand_empty, _B.many_final_segments_case)


def am_stage(g, pitch):
    """computeAM on gOut [64][L] and Pitch [F] -> dict ampatt, am [64][L], seng, ratio, amcrn [F][64], status: the 25-band
    model's am_stage with a pitch of 201 or more refused"""
    L = g.shape[1]
    nfr = L // HOP
    pitch = np.asarray(pitch, np.int32)
    out = dict(ampatt=np.zeros((NCH, L), np.float32), am=np.zeros((NCH, L), np.float32), status=0,
               **{k: np.zeros((nfr, NCH), np.float32) for k in ("seng", "ratio", "amcrn")})
    if L > MAX_LEN:
        out["status"] = AM_TOO_LONG
        return out
    if (pitch > MAX_PITCH).any():
        out["status"] = AM_BAD_PITCH
        return out
    if nfr < 3 or not (pitch > 0).any():
        return out
    out["ampatt"] = am_patt(g, pitch)
    out["am"] = normalised(out["ampatt"])
    out["seng"], out["ratio"], out["amcrn"] = am_rate(out["am"], pitch)
    return out


def filter_length(mp):
    """kaiserPara (0.01, 0.4 / mp)'s fLength, in its float arithmetic"""
    return len(kaiser_bandpass(mp)) - 1


def reachable_mean_pitches():
    """every mp amPatt can compute from one to five pitches in 32..200: the float sum of integers (exact) over the float count"""
    return sorted({float(F32(F32(s) / F32(c))) for c in range(1, 6) for s in range(32 * c, MAX_PITCH * c + 1)})


# ---- the inputs of the fixture ------------------------------------------------------------------------------------------------
AUDIO_CASES = ("p11900", "w4096", "lo", "hi", "t16")


def voiced16(L, f0, amp, nharm, tilt=1.0, top=7600):
    """tests/hw25_pitch_model.voiced at 16 kHz with harmonics up to `top` Hz; f0: per-sample Hz, 0 = silent"""
    ph = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(L)
    for h in range(1, nharm + 1):
        x += (amp / h ** tilt) * np.sin(h * ph) * (f0 * h < top)
    x[f0 == 0] = 0
    return x


def audio_inputs():
    """What each input is there for (tools/gen_hw64_am_golden.py asserts that it gets there):
      p11900  input p of the pitch fixture read at 16 kHz, 11900 samples: N = 14, so the FFT leaves LDS; 74 frames and 60
              samples over (neither a multiple of 5 nor of 160); 15 blocks of five frames, so the pattern kernel's eight
              workgroups per channel make a second trip; blocks without a voiced frame before and after the voiced ones
      w4096   4096 samples of input q, exactly a power of two: N = 12, the FFT never leaves LDS
      lo      a voice at 81 Hz over the whole of 3000 samples: block means near 200, the longest filter, whose window reaches
              past both ends of the utterance
      hi      a voice at 470 Hz with a vibrato (without it the estimator settles on a multiple of the period): block means
              of 32..36, the shortest filters
      t16     a voice with harmonics up to 7.6 kHz: AM labels in channels 40..63 and mask units there that only develope adds
    NO BLOCK WITHOUT A VOICED FRAME BETWEEN VOICED ONES comes out of createIBM: linearEstimate (:1110-1142) interpolates Pitch
    over every run of unvoiced frames that has a voiced frame on either side, unless the only voiced frame before the run is
    frame 0 (`else if (sd)`).  That case is made by hand instead (gap_pitch) and goes through the model, which the fixture
    pins to the reference on every block of the inputs above, voiced or not."""
    xs = PM.audio_inputs()
    rng = np.random.default_rng(20141107)
    out = {"p11900": xs["p"][:11900], "w4096": xs["q"][3000:7096]}
    L = 3000
    out["lo"] = voiced16(L, np.full(L, 81.0), 2500, 40, 0.7) + rng.normal(0, 30, L)
    out["hi"] = voiced16(L, 470 * (1 + 0.06 * np.sin(2 * np.pi * 9 * np.arange(L) / FS)), 2500, 12, 0.7) + rng.normal(0, 30, L)
    L = 4000
    f0 = 150 + 20 * np.sin(2 * np.pi * 2 * np.arange(L) / FS)
    out["t16"] = voiced16(L, f0, 3000, 50, 0.4) + rng.normal(0, 100, L)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def gap_pitch(nfr):
    """a hand-made pitch contour [nfr] with a block of five frames (5..9) without a voiced frame between voiced ones, a block
    at the largest pitch and one at the smallest, and unvoiced frames at the end"""
    p = np.zeros(nfr, np.int32)
    p[0:5] = 200
    p[10:15] = 32
    p[15:max(nfr - 3, 15)] = 77
    return p


def _blank(nfr):
    return _B._blank(nfr)


def hand_sweeps():
    """tests/hw25_am_model.hand_sweeps over the 64 channels: develope (m, 1) grows along a snake through channels 1..30 and
    develope (m, -1) along one through channels 33..63, each running down the channels, back in time, up the channels and
    forward in time again, so that the reference's in-place sweep needs several passes in either direction"""
    c = _blank(20)

    def snake(lo, hi):
        path = []
        for turn, f in enumerate(range(17, 1, -3)):
            path += [(f, ch) for ch in (range(lo, hi + 1) if turn % 2 == 0 else range(hi, lo - 1, -1))]
            if f - 3 >= 2:
                end = hi if turn % 2 == 0 else lo
                path += [(f - 1, end), (f - 2, end)]
        return path

    for f, ch in snake(1, 30):
        c["amcrn"][f, ch], c["cross_ev"][f, ch] = 1, 0.5
    c["grp"][15:20, 0], c["pratio"][15:20, 0] = 1, 0.9
    for i, (f, ch) in enumerate(snake(33, 63)):
        c["grp"][f, ch], c["pratio"][f, ch] = 1, (0.9 if i % 2 == 0 else 0.5)
    c["grp"][15:20, 32], c["pratio"][15:20, 32] = 1, 0.5
    return c


def hand_wide():
    """growth along one frame across channel 31 / 32 up to channel 63 and back down from it, in both developes: a ballot, a
    mask or a shift that is 32 bits wide stops at channel 31.  Frame 3: labelled units in channels 1..63 beside a + segment in
    channel 0; frame 9: labelled units in channels 0..62 beside a + segment in channel 63; frame 16: + units in channels 0..62
    whose pRatio alternates (each a component of its own, so -2) beside a segment below THETAT in channel 63, which is -1"""
    c = _blank(22)
    c["grp"][1:6, 0], c["pratio"][1:6, 0] = 1, 0.9
    c["amcrn"][3, 1:64], c["cross_ev"][3, 1:64] = 1, 0.5
    c["grp"][7:12, 63], c["pratio"][7:12, 63] = 1, 0.9
    c["amcrn"][9, 0:63], c["cross_ev"][9, 0:63] = 1, 0.5
    c["grp"][14:19, 63], c["pratio"][14:19, 63] = 1, 0.5
    c["grp"][16, 0:63] = 1
    c["pratio"][16, 0:63] = np.where(np.arange(63) % 2 == 0, 0.9, 0.5)
    return c


HAND_CASES = {"prune": hand_prune, "sweeps": hand_sweeps, "minus2": hand_minus2, "empty": hand_empty, "wide": hand_wide}
# the edge case of tests/hw25_am_model.py at this bank's channels (the same docstring holds)
EDGE_HAND_CASES = _B.EDGE_HAND_CASES
