"""CPU test: the inputs of the eight tools/gen_hw*_golden.py and of the Hu-Wang GPU tests, together with the edge inputs of
tests/hw25_model.py, tests/hw64_model.py and their _pitch / _am siblings, take every branch outcome of the REFERENCE's own
HuWang.cpp that an input can take, at both banks (tools/hw_oracle_coverage.py: HuWang.cpp built unmodified by `make -C oracle
hwcov` at -O0 --coverage -ffp-contract=off, once against the 25-channel 8 kHz header and once against the 64-channel 16 kHz
one, the tools' own drivers linked against it, gcov -b -c).  The Hu-Wang kernels are compared bit for bit with what that code
produced, and such a comparison sees only the outcomes its inputs take; the older inputs alone leave both zero-sum guards of
the correlogram's normalisation untaken at both banks and, at 25 channels, the segment search at frame 0, pitchCrn decided by
its last test, rightDevelope's delay clamp, amPatt past the signal's end and finalSeg's develope at frame 0, which is asserted
too, as the record of why the edge set exists.

An outcome is named by bank, function, line and gcov's branch index -- never by its text.  Outcomes on lines that allocate or
release and exception edges are not counted.  Measured with g++ / gcov 11.4, per bank over HuWang.cpp:1-465, :466-1142,
:1146-1494, :1498-1549 and :1553-1677: on the older inputs 109 / 289 / 182 / 24 / 27 (hw25) and 108 / 294 / 184 / 24 / 27
(hw64) of 115 / 295 / 186 / 24 / 30 outcomes; with the edge set 111 / 292 / 184 / 24 / 27 and 110 / 294 / 184 / 24 / 27.
Another compiler may number branches differently; the counts are printed, not asserted.

Needs g++ and gcov: a missing tool is a failure, not a skip; so is a missing oracle/_ref/hwcov."""
import functools

import pytest

BANKS = ("hw25", "hw64")

_KT = ("the permeability kt is at most G dt = 2000 / fs, a quarter at 8 kHz and an eighth at 16 kHz, and 0 where the argument "
       "is not positive")
_DELTA = "kaiserPara's delta is the constant 0.01 at both of its calls (lowPass, amPatt), so a = 40: above 21, not above 50"


def _both(function, line, index, reason):
    return {(bank, function, line, index): reason for bank in BANKS}


# outcomes no input of createIBM, resynthesis or the stages' entry points can take: (bank, function, line, index) -> reason
UNREACHABLE = {
    **_both("loudnessLevelInPhons", 190, 0, "constants: the centre frequencies lie between MINCF >= 50 and MAXCF <= 8000, inside "
            "the table's 20..12500 Hz"),
    **_both("hairCell", 289, 0, "q < 0 after the update: " + _KT + ", so q loses at most kt q < q to the cleft while replenish "
            "and reprocess are not negative; the float difference of q and a smaller product is not negative"),
    ("hw64", "hairCell", 292, 0): "c < 0 after the update: c loses (L + R) dt c = 9080 / 16000 c < c at 16 kHz and gains kt q >= 0 "
                                  "(at 8 kHz the factor is 1.135 and the outcome is taken)",
    **_both("hairCell", 295, 0, "w < 0 after the update: w loses X dt w = 66.31 / fs w < w and gains R dt c >= 0"),
    **_both("pitchCrn", 897, 5, "the third test fails only after the second held: with d1 > d2 that asks d1 < 1.2 d2 and "
            "d2 <= 0.8 d1, so d1 < 0.96 d1; with d1 <= d2 it asks d2 <= 0.8 d2, so d2 <= 0, and then the first test, "
            "d1 > 0.8 d2 with 0 <= d1 <= d2, has failed; delays are integers up to 200, far from where float rounding could "
            "decide"),
    ("hw25", "leftDevelope", 969, 1): "`chan<40` at 25 bands: chan runs below NUMBER_CHANNEL = 25",
    ("hw25", "rightDevelope", 1047, 1): "`chan<40` at 25 bands: chan runs below NUMBER_CHANNEL = 25",
    **_both("amPatt", 1203, 1, "f >= 0: the block's centre frame starts at 2 and f at the centre frame - 2"),
    **_both("kaiserPara", 1559, 0, _DELTA),
    **_both("kaiserPara", 1560, 1, _DELTA),
    **_both("bessi0", 1609, 1, "|x| <= beta = 3.395 (from a = 40) < 3.75: the argument is beta times a square root of at most 1"),
}

# reachable outcomes that no input of either set reaches: (bank, function, line, index) -> the inputs tried.  The same line at
# both banks counts once: two lines.
UNREACHED = {
    **_both("hairCell", 281, 1, "q >= M = 1, the replenishment switched off.  Tried: steps to -1e4 and to -1e6 held for 36 000 "
            "samples at both rates (kt = 0, so q only fills): in float q stops short of 1, where Y dt (1 - q) falls below "
            "half an ulp of q; every fixture and edge input.  No input was found that returns more to q than it took from it "
            "while q is that close to 1"),
    **_both("sinModel", 1304, 1, "pa == 0 exactly, with energy in the window: the float sum over a window of WINDOW products of "
            "cosf and the normalised pattern.  Every unit of every fixture and edge input was tried; "
            "computeAMRate is reached through createIBM alone, so no array can be handed to it"),
}

# what the edge set is there for: untaken by the older inputs, taken with the edge set
TARGETS = (
    ("hw25", "crossCorr", 408, 1), ("hw25", "crossCorr", 413, 1), ("hw64", "crossCorr", 408, 1), ("hw64", "crossCorr", 413, 1),
    ("hw25", "search", 590, 1), ("hw25", "pitchCrn", 897, 7), ("hw25", "rightDevelope", 1077, 0),
    ("hw25", "amPatt", 1221, 1), ("hw25", "develope", 1456, 1),
)


@functools.lru_cache(maxsize=None)
def _measured():
    from tools import hw_oracle_coverage as C
    try:
        return C.measure(("hw-tests", "both"))
    except (RuntimeError, FileNotFoundError) as e:     # g++ / gcov missing; the build missing (`make -C oracle hwcov`)
        pytest.fail(str(e))


def _key(b):
    return (b.bank, b.function, b.line, b.index)


def _fmt(bs):
    return "; ".join(f"{b.bank} {b.function} :{b.line} branch {b.index}" for b in bs)


def _print_counts(per_bank, what):
    from tools import hw_oracle_coverage as C
    for bank in BANKS:
        for lo, hi in C.RANGES:
            t, n = C.share([b for b in per_bank[bank] if C.range_of(b.line) == (lo, hi)])
            print(f"{bank} HuWang.cpp:{lo}-{hi}: {t} of {n} outcomes taken by {what}")


def test_both_sets_take_every_outcome_of_the_hu_wang_chain():
    """every outcome of HuWang.cpp -- the data path of :1-1549 and the window code of :1553-1677, and whatever else the file
    holds -- is taken, listed in UNREACHABLE with a reason, or one of the at most four lines of UNREACHED"""
    from tools import hw_oracle_coverage as C
    both = _measured()["both"]
    _print_counts(both, "the older inputs and the edge set")
    assert len({k[1:3] for k in UNREACHED}) <= 4 and all(UNREACHED.values()) and all(UNREACHABLE.values())
    for bank in BANKS:
        assert {lo for lo, hi in C.RANGES} == {C.range_of(b.line)[0] for b in both[bank] if C.range_of(b.line)}, "a range has no outcome"
        left = [b for b in C.untaken(both[bank]) if _key(b) not in UNREACHABLE and _key(b) not in UNREACHED]
        assert not left, "outcomes never taken and not listed: " + _fmt(left)
    # the tables hold nothing that is in fact taken (a stale entry would hide a later loss), and nothing gcov does not report
    untaken_keys = {_key(b) for bank in BANKS for b in C.untaken(both[bank])}
    stale = [k for k in list(UNREACHABLE) + list(UNREACHED) if k not in untaken_keys]
    assert not stale, f"listed as never taken, but taken (or not reported under this bank, function, line and index): {stale}"
    taken_keys = {_key(b) for bank in BANKS for b in both[bank] if b.taken}
    missing = [k for k in TARGETS if k not in taken_keys]
    assert not missing, f"the edge set no longer takes what it is there for: {missing}"


def test_the_older_hu_wang_inputs_alone_do_not():
    from tools import hw_oracle_coverage as C
    old = _measured()["hw-tests"]
    _print_counts(old, "the older inputs alone")
    left = [b for bank in BANKS for b in C.untaken(old[bank]) if _key(b) not in UNREACHABLE and _key(b) not in UNREACHED]
    print("  untaken by the older inputs: " + _fmt(left))
    assert {_key(b) for b in left} == set(TARGETS)


def test_hu_wang_edge_set_stays_small():
    from tools import hw_oracle_coverage as C
    for bank in BANKS:
        e = C.edge_inputs(bank)
        total = sum(len(x) for x in e["audio"].values())
        frames = [a[0].shape[0] for a in e["pitch_hand"].values()] + [c["grp"].shape[0] for c in e["final"].values()]
        print(f"{bank}: {len(e['audio'])} audio inputs, {total} samples; hand-made cases of {frames} frames")
        assert total < 200000 and max(frames) <= 36       # 36 frames: the largest of the present hand-made cases
        assert all(x.dtype.name == "float32" for x in e["audio"].values())
    from tests import hw25_am_model, hw25_model, hw25_pitch_model
    for table in (hw25_model.EDGE_INPUTS, hw25_pitch_model.EDGE_HAND_CASES, hw25_am_model.EDGE_HAND_CASES):
        assert all(make.__doc__ and "HuWang.cpp:" in make.__doc__ for make in table.values())
