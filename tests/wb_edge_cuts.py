"""TEST INFRASTRUCTURE ONLY: where the time-slice tests cut the wideband edge set (tests/ns_edge_cases.signals_wb()).

A cut tests the state a slice hands to the next, so the cuts lie inside the stretches the signals exist for, and their
positions come from the reference, not from a guess:

  FIRST_TAKEN   the input frame (of 160 samples) at which the reference first takes the outcome a signal is there for, found
                with `tools/wb_oracle_coverage.py --only NAME --first FILE:LINE:INDEX`; tests/test_wb_edge_coverage_cpu.py
                holds every entry against the instrumented library (the prefix up to the frame takes it, one frame less not)
  hb_hangover_frame / vad_hangover_frame
                the first frame inside a hang-over of the high band's VAD (tests/wb_reference.py: vad16k()) and of the
                frame-dropping VAD (tests/wb_afe_reference.py: the emitted flag is 1 while the ring of seven holds no speech
                frame), from the reference run live on oracle/_ref/libetsi_ref.so

bounds() puts one-frame slices from two frames before to two after each of these, every frame of the first thirteen (the
first ten frames' rules, the four-frame latency, the first cepstral frame and the first emission), two cuts in the long
stretches in which the low band's estimates, then also the high band's, sit on their floors, and one-frame slices across the
start of the closing noise that reads them."""
import functools

import numpy as np

# signal -> {(file, function, line, gcov branch index): frame}
FIRST_TAKEN = {
    "ones_then_zeros_wb": {("NoiseSup.c", "FilterCalc", 515, 0): 114, ("NoiseSup.c", "FilterCalc", 543, 0): 450,
                           ("16kHzProcessing.c", "DoSpecSub16k", 461, 0): 1373},
    "square8_burst_wb": {("WaveProc.c", "GetMaximaPositions", 145, 3): 16, ("WaveProc.c", "GetMaximaPositions", 155, 1): 16,
                         ("VAD.c", "DoVADProc", 249, 6): 17, ("WaveProc.c", "GetMaximaPositions", 130, 3): 34,
                         ("WaveProc.c", "GetMaximaPositions", 140, 1): 34},
    "low_tone_after_burst_wb": {("VAD.c", "DoVADProc", 249, 3): 34},
    "short_onset_wb": {("VAD.c", "DoVADFlush", 394, 0): 10},      # an outcome of the flush: the shortest utterance that takes it
}
ON_THE_FLOORS = (700, 1440)    # between the low band's second floor (450) and the high band's (1373); behind the latter


def hb_hangover_frame(x):
    """the first frame of x after which the reference's high-band VAD is inside a hang-over (no speech run, 0 < hangOver16k),
    or None"""
    from tests import wb_reference as W
    x = np.ascontiguousarray(x, dtype=np.int16)
    ref = W.WbReference()
    den, feat = np.zeros(80, np.int16), np.zeros(16, np.float32)
    found = None
    for f in range(x.size // 160):
        sig = x[f * 160:(f + 1) * 160].copy()
        ref.lib.DoAdvProcess(sig.ctypes.data, den.ctypes.data, feat.ctypes.data, ref.fe)
        s = ref.vad16k()
        if s["nbSpeech"] == 0 and s["hangOver"] > 0:
            found = f
            break
    ref.close()
    return found


def vad_hangover_frame(x):
    """the first frame of x at which the reference's frame-dropping VAD emits 1 while its ring of seven holds no speech frame
    (so a countdown alone holds the flag), or None.  The rows DoVADProc emits are those of the last n - 6 of its n calls."""
    from tests import wb_afe_reference as A
    t = A.trace(x)
    ring = (t["flags"][2:] != 0).astype(np.int64)          # one DoVADProc call per cepstral frame: from the third output on
    frames = t["out_frames"][2:]
    n = len(ring)
    m = max(n - 6, 0)
    rows = t["feat15"][t["n_null"]:t["n_null"] + m, 14]
    assert len(rows) == m
    for j in range(m):
        c = n - m + j
        if c >= 6 and rows[j] == 1.0 and not ring[c - 6:c + 1].any():
            return int(frames[c])
    return None


@functools.lru_cache(maxsize=None)
def bounds():
    """the slice bounds (frames of 160) for the whole set run as one list, longest utterance first; ends at its length"""
    from tests import ns_edge_cases as E
    sig = E.signals_wb()
    nfr = max(len(x) // 160 for x in sig.values())
    at = [f for per in FIRST_TAKEN.values() for f in per.values()]
    hb = [hb_hangover_frame(x) for x in sig.values()]
    vad = [vad_hangover_frame(x) for x in sig.values()]
    assert any(f is not None for f in hb), "no signal of the set puts the reference's high-band VAD into a hang-over"
    assert any(f is not None for f in vad), "no signal of the set puts the reference's frame-dropping VAD into a hang-over"
    at += [f for f in hb + vad if f is not None]
    at.append(E.WB_TAIL_START)          # ones_then_zeros_wb's closing noise: its rows read the estimate the zeros left on its floor
    b = set(range(14)) | set(ON_THE_FLOORS) | {nfr}
    for f in at:
        b |= {g for g in range(f - 1, f + 3) if 0 < g < nfr}
    return tuple(sorted(b))
