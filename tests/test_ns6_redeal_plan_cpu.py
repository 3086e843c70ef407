"""CPU test of csrc/ns6_beat_plan.h for the variant the dense six-wave NoiseSup kernel takes since its feed-forward work was re-dealt
(ns_pipe6_kernel.hip, REDEAL; ns6plan::kVariantDenseRedeal): FA also filters stage 0 of frame i-3 from tick 3 on, N1 also takes the VAD
log-energy of frame i-2.  tests/ns6_redeal_plan_driver.cpp, compiled with the address and undefined-behaviour sanitizers as a
stand-alone program, prints that variant's table and both ends of every role's steady range over a sweep of onsets and frame counts.

The flags are restated here, role by role, from the kernel's beat_flag calls of that variant; the steady range must be exactly the
beats of [0, nfr + 9) on which all of them hold (for FA also i + 1 < nfr, the prefetch of the next frame), less the first one for S.
tests/test_ns6_beat_plan_cpu.py does the same for the three variants from before, whose tables the new bit must not touch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
MAX_ONSET, MAX_NFR = 40, 80
DEPTH = 9
REDEAL = 8
ROLES = ("FA", "FB", "B0", "N1", "G1", "S")
FLAGS = {
    "FA": [(0, 3), (3, 5), (3, 3)],           # own frame into stage 0, stage 1 of i-3; the stage-0 filter of i-3
    "FB": [(1, 3), (4, 5)],
    "B0": [(2, 3)],
    "N1": [(5, 5), (7, 5), (2, 1)],           # noise tracking, gain-factor scalars; the VAD log-energy of i-2
    "G1": [(8, 5)],
    "S": [(1, 1), (3, 3), (6, 5), (9, 5)],    # VAD sum, den sum, noise sum, output
}
LEAD = {"FA": 7, "FB": 8, "B0": 4, "N1": 11, "G1": 12, "S": 14}
TAIL = {"FA": -1, "FB": 1, "B0": 2, "N1": 2, "G1": 8, "S": 1}     # N1: 2, where the dense variant before had 5


def _all_true(role, i, onset, nfr):
    if onset is None:
        return False
    ok = all(i - d < nfr and i - d - (k - 1) >= onset for d, k in FLAGS[role])
    return ok and (role != "FA" or i + 1 < nfr)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/ns6_redeal_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("ns6_redeal_plan") / "ns6_redeal_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "ns6_redeal_plan_driver.cpp"), "-o", exe])
    run = subprocess.run([exe, str(MAX_ONSET), str(MAX_NFR)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    variant, table, ends, ranges = None, {}, {}, {}
    for ln in run.stdout.splitlines():
        tok = ln.split()
        if tok[0] == "variant":
            variant = (int(tok[1]), int(tok[2]))
        elif tok[0] == "flags":
            table[int(tok[1])] = (int(tok[2]), int(tok[3]), [tuple(map(int, t.split(":"))) for t in tok[4:]])
        elif tok[0] == "ends":
            ends[int(tok[1])] = (int(tok[2]), int(tok[3]))
        else:
            role, onset, nfr, b, e = map(int, tok[1:])
            ranges[role, None if onset < 0 else onset, nfr] = (b, e)
    return variant, table, ends, ranges


def test_ns6_redeal_plan_table_is_the_kernels(sweep):
    variant, table, ends, _ = sweep
    assert variant == (REDEAL, REDEAL)
    for r, role in enumerate(ROLES):
        ahead, settle, flags = table[r]
        assert sorted(flags) == sorted(FLAGS[role]), f"{role}: {flags}"
        assert ahead == (1 if role == "FA" else 0) and settle == (1 if role == "S" else 0), role
        assert ends[r] == (LEAD[role], TAIL[role]), f"{role}: lead and tail {ends[r]}"


def test_ns6_redeal_steady_range_is_exactly_the_beats_with_every_flag_true(sweep):
    _, _, _, ranges = sweep
    assert len(ranges) == 6 * (MAX_ONSET + 2) * (MAX_NFR + 1)
    trips = {role: set() for role in ROLES}
    for (r, onset, nfr), (b, e) in ranges.items():
        role, niter = ROLES[r], nfr + DEPTH
        what = f"{role}, onset {onset}, nfr {nfr}: [{b}, {e})"
        e = min(e, niter)                       # as the kernel's loop takes it
        steady = list(range(b, e))              # empty when e <= b
        true_beats = [i for i in range(niter) if _all_true(role, i, onset, nfr)]
        if true_beats:
            assert true_beats == list(range(true_beats[0], true_beats[-1] + 1)), what
        want = true_beats[1:] if role == "S" else true_beats      # S: the first such beat sets firstOut, in the general copy
        assert steady == want, f"{what}, every flag is true on {true_beats[:1]} .. {true_beats[-1:]}"
        if steady:
            assert 0 <= b and e <= niter, what
            if role == "FA":
                assert e <= nfr - 1, f"{what}: the prefetch of frame i + 1 would leave the utterance"
            if role == "S":
                assert b - 1 == onset + 13 and _all_true(role, b - 1, onset, nfr), what
            assert sorted(list(range(0, b)) + steady + list(range(e, niter))) == list(range(niter)), what
        if onset is None:
            assert not steady, what
        else:
            trips[role].add(max(e - b, 0))
    for role in ROLES:
        assert set(range(0, 34)) <= trips[role], f"{role}: trip counts {sorted(trips[role])[:40]}"


def test_ns6_redeal_general_copy_covers_the_moved_work(sweep):
    """What the steady copy does not cover the general one must: FA's filter runs on ticks 3 and 4, before its steady range begins, and
    on the drain beats nfr .. nfr + 2, after it; N1's logarithm runs from the onset's beat + 2 and ends two beats past the last frame."""
    _, _, _, ranges = sweep
    fa, n1 = ROLES.index("FA"), ROLES.index("N1")
    for onset in (0, 5, 16):
        for nfr in (onset + 1, onset + 3, onset + 20, MAX_NFR):
            b, e = ranges[fa, onset, nfr]
            filt = [i for i in range(nfr + DEPTH) if i - 3 < nfr and i - 3 - 2 >= onset]          # flag (3, 3)
            assert filt == list(range(onset + 5, nfr + 3)), (onset, nfr)
            assert all(i in filt for i in range(b, min(e, nfr + DEPTH))), (onset, nfr)
            assert (not filt) or filt[-1] == nfr + 2 >= e, (onset, nfr)
            b, e = ranges[n1, onset, nfr]
            logs = [i for i in range(nfr + DEPTH) if i - 2 < nfr and i - 2 >= onset]               # flag (2, 1)
            assert logs == list(range(onset + 2, nfr + 2)) and e == nfr + 2, (onset, nfr)
