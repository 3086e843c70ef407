"""tests/hw64_pitch_model.py -- TEST INFRASTRUCTURE ONLY: the numpy model of the Hu-Wang estimator's initial grouping and pitch
tracking (initGroup and pitchDtm, HuWang.cpp:466-1142) at 16 kHz on the 64-channel bank, that is at the constants of
resyth_64sub_IBM/cpp/HuWang.h: NUMBER_CHANNEL 64, MAX_DELAY 201, MIN_DELAY 32, OFFSET 160.

The reference's source is the same at both rates, and so is the model's: the functions of tests/hw25_pitch_model.py read the
bank's constants from their module's globals, so this file loads a second instance of that module and gives it the 64-band
constants, as tests/hw64_model.py does with the front half.  What the channel count changes in the reference's behaviour is
restated here and put into that instance:

  * leftDevelope and rightDevelope say `if (chan<40)` where they compute chan_mark and `for(chan=0; chan<40; chan++)` where they
    count number2 (HuWang.cpp:969, 1009, 1047, 1087).  On the bank of 25 that reads fifteen ghost channels past the frame; on the
    bank of 64 there are no ghost channels and no `cross` is read: channels 40..63 never enter chan_mark, so they never reach
    chan_mark2, number or the sumAuto inside a Develope, and they are not counted in number2.
  * BOUNDS is the reference's behaviour: 40 at all four places.  pitch_stage (.., bounds=...) moves any of them (to 64: what a
    port that replaces 25 by 64 throughout would compute); it is there only to prove that the fixture separates the two.

tests/test_hw64_pitch_cpu.py pins the model against what the reference's own functions produced (tests/golden/
hw64_pitch_golden.npz, written by tools/gen_hw64_pitch_golden.py); tests/test_gpu_hw64_pitch.py uses it as the expected value
where the fixture holds nothing.  The undefined cases are defined as in tests/hw25_pitch_model.py; its fourth (ghost channels
on the last frame) does not exist on this bank.
"""
import importlib.util
import os

import numpy as np

from tests import hw25_pitch_model as _P25

FS, NCH, NDEL, MIN_DELAY, MAX_DELAY, HOP = 16000, 64, 201, 32, 201, 160
THETAP, THETAT, MAX_SEG = _P25.THETAP, _P25.THETAT, _P25.MAX_SEG
TOO_MANY_SEGMENTS, CHANMARK_UNSET = _P25.TOO_MANY_SEGMENTS, _P25.CHANMARK_UNSET
PITCH_STAGES, GRP_STAGES = _P25.PITCH_STAGES, _P25.GRP_STAGES
STAGE_WORDS = 5 + 2 * NCH
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hw64_pitch_golden.npz")
F32 = np.float32
BOUND_NAMES = ("left_mark", "left_number2", "right_mark", "right_number2")  # HuWang.cpp:969, 1009, 1047, 1087
BOUNDS = dict.fromkeys(BOUND_NAMES, 40)
ALL_64 = dict.fromkeys(BOUND_NAMES, NCH)


def _second_instance():
    spec = importlib.util.spec_from_file_location("tests._hw25_pitch_model_at_64_bands", _P25.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.FS, m.NCH, m.NDEL, m.MIN_DELAY, m.MAX_DELAY, m.HOP, m.GOLDEN = FS, NCH, NDEL, MIN_DELAY, MAX_DELAY, HOP, GOLDEN
    return m


_B = _second_instance()
(rect_case, segmentation, init_group, re_group, sum_auto, find_pitch, time_crn, pitch_crn, check_pitch, linear_estimate,
 many_segments_case, crc32, load_golden) = (
    _B.rect_case, _B.segmentation, _B.init_group, _B.re_group, _B.sum_auto, _B.find_pitch, _B.time_crn, _B.pitch_crn,
    _B.check_pitch, _B.linear_estimate, _B.many_segments_case, _B.crc32, _B.load_golden)


# ---- what the channel count changes: the Developes ----------------------------------------------------------------------------
_bounds = dict(BOUNDS)


def _below(n):
    return np.arange(NCH) < n


def _number2(acf, cross, pratio, grp, frame, p, bound):
    """number2 of the Developes (:1009-1018, :1087-1096): the frame's channels 0..39 with Grp > 0 whose ratio passes.  Forty real
    channels, no ghosts: cross, pratio and the next frame are not read."""
    return int(((grp[frame] > 0) & _B._ratio_above(acf[frame], p, _B._mvalue(acf[frame])) & _below(bound)).sum())


def _develope(acf, cross, pratio, grp, pitch, buf, start, stop, step, own_mark):
    """leftDevelope:954-1030 (step -1) / rightDevelope:1032-1108 (step +1) as tests/hw25_pitch_model.py has them, with chan_mark
    zero from channel 40 on (:969, :1047) and number2 over 40 channels.  True when chan_mark was read before it was computed."""
    side = "left" if step < 0 else "right"
    mark_bound, n2_bound = _bounds[side + "_mark"], _bounds[side + "_number2"]
    chan_mark = np.zeros(NCH, bool)
    valid = unset = False
    frame = start
    while (frame >= stop) if step < 0 else (frame <= stop):
        nb = frame - step
        if pitch[nb]:
            chan_mark = (grp[nb] > 0) & _B._ratio_above(acf[nb], int(pitch[nb]), _B._mvalue(acf[nb])) & _below(mark_bound)
            valid = True
        if pitch_crn(int(buf[frame]), int(buf[nb])):
            pitch[frame] = buf[frame]
        else:
            unset = unset or not valid
            mark2 = own_mark(grp[frame]) & chan_mark
            number = int(mark2.sum())
            if number:
                k1, k2 = _B._window(int(buf[nb]))
                pitch[frame] = sum_auto(mark2.astype(np.float32), acf[frame], k1, k2)
                keep = False
                if pitch_crn(int(pitch[frame]), int(buf[nb])):
                    keep = _number2(acf, cross, pratio, grp, frame, int(pitch[frame]), n2_bound) * 2 > number
                if keep:
                    buf[frame] = pitch[frame]
                else:
                    pitch[frame] = 0
                    buf[frame] = buf[nb]
            else:
                buf[frame] = buf[nb]
        frame += step
    return unset


_B._develope = _develope


def pitch_stage(acf, pratio, mark, bounds=None):
    """The whole stage on one utterance: acf [F][64][201], the front half's pratio and mark [F][64] -> dict with pitch, grp,
    pratio, status and the stage arrays (PITCH_STAGES, GRP_STAGES).  bounds: a dict over BOUND_NAMES that replaces the
    reference's 40 at the places it names."""
    _bounds.update(BOUNDS)
    _bounds.update(bounds or {})
    try:
        return _B.pitch_stage(acf, pratio, mark)
    finally:
        _bounds.update(BOUNDS)


# ---- the inputs of the fixture ------------------------------------------------------------------------------------------------
AUDIO_CASES = ("p", "q", "r", "m9", "t16")


def audio_inputs():
    """p, q, r, s, t, m9: the samples of the 25-band fixture read as 16 kHz audio (every pitch twice as high); t16: input t
    synthesised at 16 kHz.  75, 75, 87, 50, 62, 62 and 62 frames.  The fixture holds AUDIO_CASES; s (noise) has one segment on
    this bank, not none."""
    out = dict(_P25.audio_inputs())
    out["t16"] = _B.audio_inputs()["t"]
    return out


def handmade_case():
    """tests/hw25_pitch_model.py's hand-made input at [36][64][201]: reaches `number == 0` in both Developes"""
    return rect_case(36, [(5, 30, 0, 3, 50, 0.5), (8, 12, 10, 12, 40, 0.99), (13, 19, 18, 20, 70, 0.99), (20, 24, 14, 16, 40, 0.99)])


def vote_case():
    """tests/hw25_pitch_model.py's vote case at [16][64][201]: frame 3 loses findPitch's vote outside the outermost frame that
    keeps its pitch, and lFrame = 3 all the same"""
    return rect_case(16, [(3, 12, 4, 5, 40, 0.99), (4, 7, 10, 12, 70, 0.99), (3, 3, 10, 11, 70, 0.99)])


def no_streak_case():
    """tests/hw25_pitch_model.py's case with delays this bank has (its 30 is below MIN_DELAY here): one segment whose per-frame
    peak delay alternates between 40 and 80, so that checkPitch keeps nothing and rightDevelope starts with Pitch[1] == 0"""
    acf, pratio, mark = rect_case(12, [(1, 10, 4, 7, 0, 0.99)])
    acf[:, :, 0] = 5000
    for f in range(12):
        acf[f, 4:8, 40 if f % 2 else 80] = 1500
    return acf, pratio, mark


def _mirror(case):
    """the same case with the frames in reverse order: what leftDevelope met at frame 3 rightDevelope meets at frame 12"""
    return tuple(np.ascontiguousarray(a[::-1]) for a in case)


def mark_bound_left():
    """Separates `chan<40` from `chan<64` where leftDevelope computes chan_mark (:969).  Two segments over frames 3..12, channels
    4-5 and 44-46, all peaking at delay 80, but in frame 3 the upper three peak at 120.  findPitch gives frame 3 the delay 120,
    which is not consistent with 80, so the streak is 4..12 and leftDevelope re-estimates frame 3 from chan_mark2.  With
    channels 44-46 kept out of chan_mark, sumAuto sees channels 4-5 alone and finds 80, which number2 confirms: Pitch[3] = 80.
    With them in, sumAuto finds 120, pitchCrn refuses it: Pitch[3] = 0."""
    acf, pratio, mark = rect_case(16, [(3, 12, 4, 5, 80, 0.99), (3, 12, 44, 46, 80, 0.99)])
    acf[3, 44:47, 80], acf[3, 44:47, 120] = 100, 1100
    return acf, pratio, mark


def number2_bound_left():
    """Separates 40 from 64 in leftDevelope's number2 loop (:1009).  Channels 4-7 and 44-45 over frames 3..12 peak at delay 80;
    in frame 4 the upper two peak at 120, so they fail the ratio test there and chan_mark is channels 4-7 whatever the bound.
    In frame 3 channel 4 peaks at 70 (1200), channels 5, 6, 7 at 72, 74, 76 and channels 44-45 at 70: findPitch finds 70 and
    its vote (3 of 6) zeroes it, so leftDevelope reaches frame 3.  sumAuto over channels 4-7 finds 70; number = 4.  number2
    counts channel 4 alone below 40 (2 > 4 fails: Pitch[3] = 0), and channels 4, 44, 45 over all 64 (6 > 4: Pitch[3] = 70)."""
    acf, pratio, mark = rect_case(16, [(3, 12, 4, 7, 80, 0.99), (3, 12, 44, 45, 80, 0.99)])
    acf[3, 4:8, 80] = 100
    acf[3, 4, 70], acf[3, 5, 72], acf[3, 6, 74], acf[3, 7, 76] = 1200, 1100, 1100, 1100
    acf[3, 44:46, 80], acf[3, 44:46, 70] = 100, 1100
    acf[4, 44:46, 80], acf[4, 44:46, 120] = 100, 1100
    return acf, pratio, mark


HAND_CASES = {"h": handmade_case, "v": vote_case, "ml": mark_bound_left, "nl": number2_bound_left,
              "mr": lambda: _mirror(mark_bound_left()), "nr": lambda: _mirror(number2_bound_left())}
# the hand-made case that tells 40 from 64 at each of the four places, the frame where it shows and Pitch there at 40 / at 64
SEPARATES = {"left_mark": ("ml", 3, 80, 0), "left_number2": ("nl", 3, 0, 70), "right_mark": ("mr", 12, 80, 0),
             "right_number2": ("nr", 12, 0, 70)}


# the edge cases of tests/hw25_pitch_model.py at this bank's channels and delays (the same docstrings hold)
EDGE_HAND_CASES = _B.EDGE_HAND_CASES


def hand_inputs(k):
    """acf [F][64][201], pratio, mark [F][64] of a hand-made case"""
    return {**HAND_CASES, **EDGE_HAND_CASES}[k]()
