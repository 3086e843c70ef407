"""CPU test: the inputs of the wideband (16 kHz) GPU tests, together with the wideband edge signals of
tests/ns_edge_cases.signals_wb(), take every branch outcome of the REFERENCE's own wideband data path that an input can take
(tools/wb_oracle_coverage.py: the reference library built by `make -C oracle refcov` at -O0 --coverage with the parity flags,
both trace modules run on it in a child process, gcov -b -c).  The wideband GPU tests compare the kernels with that code bit
for bit, and such a comparison sees only the outcomes its inputs take; the older inputs alone leave the high band's noise
floor, both floors of the low band's noise estimate, WaveProc's search without a neighbouring maximum, speech found by one
measure alone and the flush's raised hang-over untaken, which is asserted too, as the record of why the edge set exists.

A branch is named by the reference's file, function, line and gcov's branch index -- never by its text.  Measured with gcc /
gcov 11.4: on the older inputs 108 of 128 (16kHzProcessing.c), 262 of 280 (NoiseSup.c), 51 of 66 (CompCeps.c), 89 of 100
(VAD.c), 75 of 82 (WaveProc.c), 10 of 12 (PostProc.c) outcomes; with the edge set 109, 264, 51, 92, 79 and 10.  Another
compiler may number branches differently; the counts are printed, not asserted.

Needs gcc and gcov: a missing tool is a failure, not a skip; so is a missing oracle/_ref/cov/libetsi_ref_cov.so."""
import functools

import pytest

# the functions that may leave reachable outcomes unreached (at most four, each naming the inputs tried); every other
# data-path function of the six files has every outcome taken but for UNREACHABLE
LOOSE = {"VAD.c": ("focalpoint", "DoVADProc", "DoVADFlush"), "WaveProc.c": ("GetMaximaPositions", "GetTeagerFilter", "DoWaveProc"),
         "PostProc.c": ("DoPostProc",)}

_ALLOC = "a failed malloc"
_WIDE = "configuration: Do16kHzProc is 1 on every call of a front end allocated for 16 kHz"
_QMF = "configuration: the QMF's input length (160) against its filter length (118), both constants"

# outcomes no input of the wideband entry points can take: (file, function, line, gcov branch index) -> reason
UNREACHABLE = {
    ("16kHzProcessing.c", "MergeSSandCoded", 117, 1): "configuration: the number of high bands is the constant 3",
    ("16kHzProcessing.c", "Do16kProcessing", 756, 0): _QMF,
    ("16kHzProcessing.c", "Do16kProcessing", 757, 0): _QMF,
    ("16kHzProcessing.c", "Do16kProcessing", 757, 1): _QMF,
    ("16kHzProcessing.c", "Do16kProcessing", 759, 0): _QMF,
    ("16kHzProcessing.c", "Do16kProcessing", 759, 1): _QMF,
    ("NoiseSup.c", "VAD", 376, 1): "the frame counter saturating needs 2^31 - 1 frames in one utterance",
    ("NoiseSup.c", "DoNoiseSup", 1104, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1113, 0): _ALLOC,
    ("NoiseSup.c", "DoNoiseSup", 1166, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1216, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1307, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1340, 1): "the stage index is 0 or 1: the second test of an else-if whose first test was `stage is 0`",
    ("NoiseSup.c", "DoNoiseSup", 1372, 1): "the count of frames in the first stage was incremented at line 1139 of the same call and never falls",
    ("NoiseSup.c", "DoNoiseSup", 1378, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1392, 1): _WIDE,
    ("NoiseSup.c", "DoNoiseSup", 1402, 1): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 388, 0): _ALLOC,
    ("CompCeps.c", "WI8CompCeps", 392, 1): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 418, 0): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 419, 0): _WIDE + " (the 8 kHz energy floor, behind the test of line 418)",
    ("CompCeps.c", "WI8CompCeps", 419, 1): _WIDE + " (the 8 kHz energy floor, behind the test of line 418)",
    ("CompCeps.c", "WI8CompCeps", 464, 1): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 488, 1): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 518, 1): _WIDE,
    ("CompCeps.c", "WI8CompCeps", 526, 0):
        "the wideband log-energy floor: CorrectEnergy adds exp of the three merged high bands to a sum of squares >= 0.  Each is "
        "0.7 of a decoded band plus 0.3 of a subtracted band floored at -10; a decoded band is a weighted mean of low bands "
        "floored at -10 minus codes, and a code is at most the log of the largest coding-band energy an int16 frame can give "
        "(below 38) plus 10.  So each band is above 0.7 (-58) + 0.3 (-10) = -43.6 and the sum above 3 e^-44.3, never below e^-50",
    ("CompCeps.c", "WI8CompCeps", 544, 1): "the buffer pointer is not NULL after the malloc of line 388 succeeded",
    ("VAD.c", "focalpoint", 80, 0): "a negative ring index: both callers pass a focus >= 0 and an offset >= 1",
    ("VAD.c", "DoVADProc", 293, 4): "`Trigger >= 3` true after both countdowns were 0: line 283 sets the short countdown to 5 whenever Trigger >= 3",
    ("VAD.c", "DoVADFlush", 411, 4): "`Trigger >= 3` true after both countdowns were 0: line 401 sets the short countdown to 5 whenever Trigger >= 3",
    ("WaveProc.c", "GetTeagerFilter", 261, 0): "the ring index after 195 steps modulo 9 is 6 for the constant frame length of 200, never 0",
    ("WaveProc.c", "DoWaveProc", 422, 0): _ALLOC,
    ("PostProc.c", "DoPostProc", 129, 0): "configuration: the Noc0 select; the front end of every wideband test runs with Noc0 = 0",
}

# reachable outcomes of LOOSE that no input of either set reaches: (file, function, line, branch) -> inputs tried.  Empty:
# square8_burst_wb takes GetMaximaPositions' four exits and VADNS alone, low_tone_after_burst_wb the mel measure alone,
# short_onset_wb the flush's raised hang-over.
UNREACHED = {}

# what the edge set is there for: untaken by the older inputs, taken with the edge set
TARGETS = (
    ("16kHzProcessing.c", "DoSpecSub16k", 461, 0),
    ("NoiseSup.c", "FilterCalc", 515, 0), ("NoiseSup.c", "FilterCalc", 543, 0),
    ("WaveProc.c", "GetMaximaPositions", 130, 3), ("WaveProc.c", "GetMaximaPositions", 140, 1),
    ("WaveProc.c", "GetMaximaPositions", 145, 3), ("WaveProc.c", "GetMaximaPositions", 155, 1),
    ("VAD.c", "DoVADProc", 249, 3), ("VAD.c", "DoVADProc", 249, 6),
    ("VAD.c", "DoVADFlush", 394, 0),
)


@functools.lru_cache(maxsize=None)
def _measured():
    from tools import wb_oracle_coverage as C
    try:
        return C.measure(("wb-tests", "both"))
    except (RuntimeError, FileNotFoundError) as e:     # gcc / gcov missing; the library missing (`make -C oracle refcov`)
        pytest.fail(str(e))


def _key(b):
    return (b.file, b.function, b.line, b.index)


def _fmt(bs):
    return "; ".join(f"{b.file} {b.function} :{b.line} branch {b.index}" for b in bs)


def test_both_sets_take_every_outcome_of_the_wideband_data_path():
    from tools import wb_oracle_coverage as C
    both = _measured()["both"]
    for f in C.FILES:
        t, n = C.share(both[f])
        print(f"{f}: {t} of {n} outcomes taken by the wideband GPU tests' inputs and the edge set")
    assert len(UNREACHED) <= 4 and all(UNREACHED.values())
    for f in C.FILES:
        found = {b.function for b in both[f]}
        assert set(LOOSE.get(f, ())) <= found, f"{f}: gcov reports no branches for {sorted(set(LOOSE[f]) - found)}"
        left = [b for b in C.untaken(both[f]) if _key(b) not in UNREACHABLE]
        strict = [b for b in left if b.function not in LOOSE.get(f, ())]
        assert not strict, "outcomes of the data path never taken: " + _fmt(strict)
        extra = [b for b in left if _key(b) not in UNREACHED]
        assert not extra, "unlisted outcomes never taken: " + _fmt(extra)
    # the tables hold nothing that is in fact taken (a stale entry would hide a later loss), and nothing gcov does not report
    untaken_keys = {_key(b) for f in C.FILES for b in C.untaken(both[f])}
    stale = [k for k in list(UNREACHABLE) + list(UNREACHED) if k not in untaken_keys]
    assert not stale, f"listed as never taken, but taken (or not reported under this file, function, line and index): {stale}"
    taken_keys = {_key(b) for f in C.FILES for b in both[f] if b.taken}
    missing = [k for k in TARGETS if k not in taken_keys]
    assert not missing, f"the edge set no longer takes what it is there for: {missing}"


def test_the_older_wideband_inputs_alone_do_not():
    from tools import wb_oracle_coverage as C
    old = _measured()["wb-tests"]
    for f in C.FILES:
        t, n = C.share(old[f])
        print(f"{f}: {t} of {n} outcomes taken by the wideband GPU tests' inputs alone")
    untaken_keys = {_key(b) for f in C.FILES for b in C.untaken(old[f])}
    taken = [k for k in TARGETS if k not in untaken_keys]
    assert not taken, f"the older inputs now take {taken}: the record in this file's docstring is out of date"
    left = [b for f in C.FILES for b in C.untaken(old[f]) if _key(b) not in UNREACHABLE]
    print("  untaken by the older inputs: " + _fmt(left))
    assert {_key(b) for b in left} == set(TARGETS)


def test_recorded_first_frames_are_the_references():
    """tests/wb_edge_cuts.FIRST_TAKEN, where the time-slice tests put their one-frame slices: the signal's prefix up to and
    including the recorded frame takes the outcome, the prefix one frame shorter does not; every target has an entry."""
    from tests import wb_edge_cuts as K
    from tools import wb_oracle_coverage as C
    assert {k for per in K.FIRST_TAKEN.values() for k in per} == set(TARGETS)
    try:
        cr = C.CoverageRun()
    except (RuntimeError, FileNotFoundError) as e:
        pytest.fail(str(e))
    with cr:
        for name, per in K.FIRST_TAKEN.items():
            for f in sorted(set(per.values())):
                before, upto = C.takes(cr, name, f), C.takes(cr, name, f + 1)
                for key, at in per.items():
                    if at == f:
                        assert key not in before and key in upto, f"{name}: {key} is not first taken at frame {f}"


def test_wideband_edge_set_stays_small():
    from tests import ns_edge_cases as E
    s = E.signals_wb()
    total = sum(len(x) for x in s.values())
    print(f"{len(s)} signals, {total} samples at 16 kHz")
    assert total < 800000
    assert all(x.dtype.name == "int16" for x in s.values())
    assert list(s)[:4] == list(E.WB_CARRIED) and [len(s[k]) for k in E.WB_CARRIED] == [3200, 16000, 33600, 24000]
    assert all(f.__doc__ and f.__name__ in s for f in E._SIGNALS_WB)
