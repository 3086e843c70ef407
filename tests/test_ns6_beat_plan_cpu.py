"""CPU test of csrc/ns6_beat_plan.h, the table from which the six-wave NoiseSup kernels (ns_pipe6_kernel.hip) take the beats on which a
role runs its flag-free steady copy: tests/ns6_beat_plan_driver.cpp, compiled with the address and undefined-behaviour sanitizers as a
stand-alone program, prints the table and both ends of the steady range over a sweep of onsets and frame counts.

What a role does with frame i - d at beat i hangs on "the frame exists and has tick >= k":  i - d < nfr and i - d - (k - 1) >= onset.
The flags are restated here, role by role, from the kernel's tick_ge calls; the steady range must be exactly the beats of
[0, nfr + 9) on which all of them hold (for FA also i + 1 < nfr, the prefetch of the next frame), less the first one for S, which
notes the index of its first output frame at the first beat that produces one and must do so in the general copy."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
MAX_ONSET, MAX_NFR = 40, 80
DEPTH = 9
FD, LIGHT, DIFG1 = 1, 2, 4
VARIANTS = {"plain": LIGHT | DIFG1, "dense": 0, "fd": FD | LIGHT | DIFG1}
ROLES = ("FA", "FB", "B0", "N1", "G1", "S")


def _flags(variant, role):
    """(d, k) of every tick_ge the role evaluates in that variant of ns_pipe6_body"""
    light, fd = bool(variant & LIGHT), bool(variant & FD)
    return {
        "FA": [(0, 3), (3, 5)] + ([(2, 1)] if light else []),   # own frame into stage 0, stage 1 of i-3; LIGHT: VAD log of i-2
        "FB": [(1, 3), (4, 5)],                                 # one beat behind FA
        "B0": [(2, 3)],
        "N1": [(5, 5), (7, 5)],                                 # noise tracking, gain-factor scalars
        "G1": [(8, 5)],
        "S": [(1, 1), (3, 3), (6, 5), (9, 5)] + ([(9, 5)] if fd else []),   # VAD sum, den sum, noise sum, output; FD: speech flags
    }[role]


def _all_true(variant, role, i, onset, nfr):
    if onset is None:
        return False
    ok = all(i - d < nfr and i - d - (k - 1) >= onset for d, k in _flags(variant, role))
    return ok and (role != "FA" or i + 1 < nfr)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/ns6_beat_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("ns6_beat_plan") / "ns6_beat_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "ns6_beat_plan_driver.cpp"), "-o", exe])
    run = subprocess.run([exe, str(MAX_ONSET), str(MAX_NFR)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    table, ranges, depth = {}, {}, None
    for ln in run.stdout.splitlines():
        tok = ln.split()
        if tok[0] == "depth":
            depth = int(tok[1])
        elif tok[0] == "flags":
            table[int(tok[1]), int(tok[2])] = (int(tok[3]), int(tok[4]), [tuple(map(int, t.split(":"))) for t in tok[5:]])
        else:
            v, role, onset, nfr, b, e = map(int, tok[1:])
            ranges[v, role, None if onset < 0 else onset, nfr] = (b, e)
    return depth, table, ranges


def test_ns6_beat_plan_table_is_the_kernels(sweep):
    depth, table, _ = sweep
    assert depth == DEPTH
    for v in VARIANTS.values():
        for r, role in enumerate(ROLES):
            ahead, settle, flags = table[v, r]
            assert sorted(flags) == sorted(_flags(v, role)), f"variant {v}, {role}: {flags}"
            assert ahead == (1 if role == "FA" else 0) and settle == (1 if role == "S" else 0), f"variant {v}, {role}"


def test_ns6_steady_range_is_exactly_the_beats_with_every_flag_true(sweep):
    _, _, ranges = sweep
    assert len(ranges) == 3 * 6 * (MAX_ONSET + 2) * (MAX_NFR + 1)
    trips = {role: set() for role in ROLES}
    for (v, r, onset, nfr), (b, e) in ranges.items():
        role, niter = ROLES[r], nfr + DEPTH
        what = f"variant {v}, {role}, onset {onset}, nfr {nfr}: [{b}, {e})"
        e = min(e, niter)                       # as the kernel's loop takes it
        steady = list(range(b, e))              # empty when e <= b
        true_beats = [i for i in range(niter) if _all_true(v, role, i, onset, nfr)]
        assert true_beats == list(range(true_beats[0], true_beats[-1] + 1)) if true_beats else True, what
        want = true_beats[1:] if role == "S" else true_beats      # S: the first such beat sets firstOut, in the general copy
        assert steady == want, f"{what}, every flag is true on {true_beats[:1]} .. {true_beats[-1:]}"
        if steady:
            assert 0 <= b and e <= niter, what                     # a sub-range of [0, niter)
            assert all(_all_true(v, role, i, onset, nfr) for i in steady), what
            if role == "FA":
                assert e + 0 <= nfr - 1, f"{what}: the prefetch of frame i + 1 would leave the utterance"
            if role == "S":                                        # produced at beat b - 1: frame onset + 4 at beat onset + 13
                assert b - 1 == onset + 13 and _all_true(v, role, b - 1, onset, nfr), what
            # the general copy runs [0, b) and [e, niter): with the steady range they partition the role's beats
            assert sorted(list(range(0, b)) + steady + list(range(e, niter))) == list(range(niter)), what
        if onset is None:
            assert not steady, what
        else:
            trips[role].add(max(e - b, 0))
    # too short an utterance: the range is empty, and the sweep meets every small trip count of every role
    for role in ROLES:
        assert set(range(0, 34)) <= trips[role], f"{role}: trip counts {sorted(trips[role])[:40]}"


def test_ns6_steady_range_named_cases(sweep):
    """Both ends as numbers, dense variant: the range starts once the deepest flag holds and ends with the shallowest."""
    _, _, ranges = sweep
    lead = {"FA": 7, "FB": 8, "B0": 4, "N1": 11, "G1": 12, "S": 14}
    tail = {"FA": -1, "FB": 1, "B0": 2, "N1": 5, "G1": 8, "S": 1}
    for r, role in enumerate(ROLES):
        assert ranges[0, r, 3, 60] == (3 + lead[role], 60 + tail[role]), role
        b, e = ranges[0, r, 10, 10 + lead[role] - tail[role]]      # nfr - onset one short of a single steady beat
        assert e <= b, role
        b, e = ranges[0, r, 10, 10 + lead[role] - tail[role] + 1]
        assert e == b + 1, role
        b, e = ranges[0, r, None, 60]
        assert b >= 60 + DEPTH, role
    # LIGHT adds FA's flag of frame i - 2, which moves neither end; FD's fifth flag of S is the fourth's
    for v in VARIANTS.values():
        assert ranges[v, 0, 0, 50] == (7, 49) and ranges[v, 5, 0, 50] == (14, 51)
