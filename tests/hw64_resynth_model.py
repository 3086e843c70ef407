"""tests/hw64_resynth_model.py -- TEST INFRASTRUCTURE ONLY: the numpy restatement of the Hu-Wang estimator's resynthesis
(HuWang.cpp:1498-1549) at 16 kHz on the 64-channel bank, that is at the constants of resyth_64sub_IBM/cpp/HuWang.h:
NUMBER_CHANNEL 64, OFFSET 160, WINDOW 320.

The reference's source is the same at both rates and holds no literal channel count, hop or window in this function, and so does
the model: the functions of tests/hw25_resynth_model.py read the bank's constants and its two neighbour models from their
module's globals, so this file loads a second instance of that module and gives it NCH, HOP, WINDOW = 64, 160, 320 and the
64-band M / AM modules, as tests/hw64_am_model.py does with the AM model.  That the instance equals the reference on every
case of the fixture (tools/gen_hw64_resynth_golden.py asserts it) is the proof that no literal hides in the reference's stage.

What the constants change.  WINDOW is exactly 2 * OFFSET: a set frame f adds up[o] on [160 (f - 1), 160 f) (not for f = 0) and
down[o] on [160 f, 160 f + 160), and nothing rises again.  A sample 160 k + o receives at most two terms, in the frame loop's
order: down[o] from frame k, then up[o] from frame k + 1 -- two bits per channel, not three.  The largest index frame F - 1
writes is 160 (F - 1) + 159 = 160 F - 1 <= L - 1: the reference never leaves weight[], the instance's drop rule (`keep = idx <
L`) never drops anything, in_bounds() is true of every mask, and the reference pins every case, masks whose last row is set
included.  Restated here: the inputs and masks of the fixture, and weight_table() for two bits.

tests/test_hw64_resynth_cpu.py pins the model against tests/golden/hw64_resynth_golden.npz; tests/test_gpu_hw64_resynth.py uses
it at the shapes the fixture does not hold.
"""
import importlib.util
import os

import numpy as np

from tests import hw25_resynth_model as _R25
from tests import hw64_am_model as AM
from tests import hw64_model as M

NCH, HOP, WINDOW = 64, 160, 320
PI = _R25.PI
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw64_resynth_golden.npz")
F32 = np.float32
AUDIO_CASES = AM.AUDIO_CASES  # every one with createIBM's own mask: nothing is out of the reference's bounds on this bank
HAND_INPUTS = ("w4096", "t3200")
HAND_MASKS = ("ones", "checker", "frame0", "last", "single", "high", "soft")
TEXT_CASES = ("a_w4096", "h_t3200_checker")  # the cases whose text file the fixture keeps whole; the others as a CRC32


def hand_input(name):
    """w4096: L % 160 = 96, a tail of 96 samples behind the last frame; t3200: the first 3200 samples of t16, L % 160 = 0, where
    frame 19's last index 160 * 19 + 159 is exactly L - 1"""
    xs = _B._audio()
    return {"w4096": xs["w4096"], "t3200": np.ascontiguousarray(xs["t16"][:3200])}[name]


def hand_mask(name, nfr):
    """float32 [nfr][64]; `soft` holds 0.3 and 0.7 beside 0 (every other mask is 0 / 1); `single` is one unit at channel 47 and
    `high` the channels 32..63 alone: what a ballot or a shift 32 bits wide would lose"""
    m = np.zeros((nfr, NCH), np.float32)
    f, c = np.indices(m.shape)
    if name == "ones":
        m[:] = 1
    elif name == "checker":
        m[(f + c) % 2 == 0] = 1
    elif name == "frame0":
        m[0] = 1
    elif name == "last":
        m[nfr - 1] = 1
    elif name == "single":
        m[nfr // 2, 47] = 1
    elif name == "high":
        m[:, 32:] = 1
    elif name == "soft":
        m[(f + 2 * c) % 3 == 0] = 0.3
        m[(f + 2 * c) % 3 == 1] = 0.7
    else:
        raise KeyError(name)
    return m


def reference_cases(am_golden):
    """name -> (x, mask float32 [F][64] of 0 / 1) for every case of the fixture: the audio cases with createIBM's own mask (as
    tests/golden/hw64_am_golden.npz holds it), then the hand-made masks; `soft` goes to the reference as mark > 0"""
    out = {}
    for k in AUDIO_CASES:
        out[f"a_{k}"] = (_B._audio()[k], am_golden[f"mask_{k}"].astype(np.float32))
    for i in HAND_INPUTS:
        x = hand_input(i)
        for name in HAND_MASKS:
            out[f"h_{i}_{name}"] = (x, (hand_mask(name, len(x) // HOP) > 0).astype(np.float32))
    return out


def case_input(k):
    """the named input of a fixture case a_<input> or h_<input>_<mask>"""
    return k.split("_")[1]


def weight_table():
    """float32 [160][4]: the weight at position o of a hop for the four states of the frames k, k + 1 (bit 0, 1), read off
    weights() on four-frame masks at frame k = 1 -- independent of how the engine's host table is built"""
    out = np.zeros((HOP, 4), np.float32)
    for bits in range(4):
        m = np.zeros((4, NCH), bool)
        for b in range(2):
            m[1 + b, 0] = bool(bits >> b & 1)
        out[:, bits] = weights(m, 4 * HOP)[0, HOP:2 * HOP]
    return out


def _second_instance():
    spec = importlib.util.spec_from_file_location("tests._hw25_resynth_model_at_64_bands", _R25.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.NCH, m.HOP, m.WINDOW, m.GOLDEN, m.M, m.AM = NCH, HOP, WINDOW, GOLDEN, M, AM
    m.hand_input = hand_input  # _reverse_of_input looks a hand input up by name
    return m


_B = _second_instance()
(in_bounds, ola_tables, weights, gammatone_rows, reverse_pass, resynth_from_reverse, resynth, resynth_input, to_short, text,
 load_golden) = (_B.in_bounds, _B.ola_tables, _B.weights, _B.gammatone_rows, _B.reverse_pass, _B.resynth_from_reverse, _B.resynth,
                 _B.resynth_input, _B.to_short, _B.text, _B.load_golden)
