#!/usr/bin/env python3
"""tools/gen_wb_afe_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/wb_afe_golden.npz: the six utterances of tools/gen_wb_golden.py and a quiet one, at 16 kHz, and what THE
REFERENCE ITSELF makes of them when its wideband mode runs the whole feature chain (oracle/_ref/libetsi_ref.so driven by
tests/wb_afe_reference.py; data only, no reference source):

    make -C oracle ref && python tools/gen_wb_afe_golden.py

Per utterance u: x{u} the input, feat_cc{u} / feat_pp{u} [nceps, 14] after WaveProc + CompCeps / after PostProc, feat15_{u}
[nemit, 15] the emitted frames (c1..c12, c0, logE, VAD flag), flags{u} [nout] the speech-flag byte per frame with a NoiseSup
output, bypass{u} [nceps] WaveProc's low-energy bypass; counts [7, 6] = frames, cepstral frames, emitted frames, null vectors
of the all-zero lead, emitted frames flagged speech, bypassed cepstral frames; first_out, onset [7].  The float NoiseSup
stream is not stored: tests/golden/wb_golden.npz pins it.

The six never leave the loud branches (WaveProc always runs, PostProc's weight is always above 1); the quiet utterance is
there for the others.  COVERAGE below is asserted here and again, on the committed file, by tests/test_wb_afe_cpu.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from speech_enhancement_amd import corpus  # noqa: E402
from tests import wb_afe_reference as A  # noqa: E402
import gen_wb_golden  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "wb_afe_golden.npz")
QUIET = 6            # index of the quiet utterance
WIDE_3S = (2, 3, 4)
MIN_SHARE = 0.10
COUNT_NAMES = ("frames", "cepstral frames", "emitted", "null lead", "flag 1", "bypass")


def utterances():
    return gen_wb_golden.utterances() + [corpus.synth_wideband(3, 32000) // 128]  # 2 s, quiet: floor division on int16


def coverage(data):
    """The conditions the fixture is there for, as a list of (what, share) that must each be >= MIN_SHARE."""
    out = []
    bypass, w = data[f"bypass{QUIET}"], A.pp_weight(data[f"feat_cc{QUIET}"][:, 13])
    n = max(len(bypass), 1)
    out += [("quiet: bypass taken", bypass.sum() / n), ("quiet: bypass not taken", (~bypass).sum() / n),
            ("quiet: weight < 0", (w < 0).sum() / n), ("quiet: weight in [0, 1]", ((w >= 0) & (w <= 1)).sum() / n),
            ("quiet: weight > 1", (w > 1).sum() / n)]
    for u in (QUIET,) + WIDE_3S:
        vad = data[f"feat15_{u}"][:, 14]
        out += [(f"utterance {u}: VAD 1", (vad == 1).sum() / max(len(vad), 1)), (f"utterance {u}: VAD 0", (vad == 0).sum() / max(len(vad), 1))]
    return out


def generate():
    data = {}
    counts, first, onset = [], [], []
    for u, x in enumerate(utterances()):
        t = A.trace(x)
        data[f"x{u}"] = x
        data[f"feat_cc{u}"], data[f"feat_pp{u}"], data[f"feat15_{u}"] = t["feat_cc"], t["feat_pp"], t["feat15"]
        data[f"flags{u}"], data[f"bypass{u}"] = t["flags"], t["bypass"]
        counts.append([len(x) // 160, len(t["feat_cc"]), len(t["feat15"]), t["n_null"], int((t["feat15"][:, 14] == 1).sum()),
                       int(t["bypass"].sum())])
        first.append(t["first_out"])
        onset.append(t["onset"])
    data["counts"] = np.array(counts, np.int64)
    data["first_out"] = np.array(first, np.int32)
    data["onset"] = np.array(onset, np.int32)
    for what, share in coverage(data):
        assert share >= MIN_SHARE, f"{what}: {share:.3f} of the frames"
    return data


if __name__ == "__main__":
    d = generate()
    np.savez_compressed(PATH, **d)
    print(PATH, os.path.getsize(PATH), "bytes")
    print("utterance", COUNT_NAMES)
    for u, c in enumerate(d["counts"]):
        print(u, c.tolist(), "first_out", d["first_out"][u], "onset", d["onset"][u])
    for what, share in coverage(d):
        print(f"{what}: {share:.3f}")
