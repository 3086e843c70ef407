"""CPU test: the inputs of the GPU parity tests, together with the edge signals of tests/ns_edge_cases.py, take every
branch of the frame loop's arithmetic in oracle/ns_oracle.c and oracle/ns16k_oracle.c in both directions
(tools/oracle_coverage.py: gcc -O0 --coverage with the parity flags, gcov -b -c).  A GPU test that compares a kernel with
the restatement sees only the branches its inputs take; the inputs of the older GPU tests alone leave the clamps, the
floors, the first-ten-frames rules and the latch untaken, which is asserted too, as the record of why the edge set exists.

Needs gcc and gcov: a missing tool is a failure, not a skip."""
import functools

import pytest

# the arithmetic of the frame loop: every branch of these is taken in both directions, but for UNREACHABLE
FULL_8K = ("ns_vad", "ns_filter_calc", "ns_gain_fact", "speech_q_var", "speech_q_spec", "speech_q_mel", "postproc", "compceps")
FULL_16K = ("vad16", "filter_calc16", "gain_fact16", "speech_q_var16", "speech_q_spec16", "speech_q_mel16")
# ... and these may leave reachable branches unreached: at most four per file, each naming the inputs that were tried
LOOSE_8K = ("waveproc", "vad_decide", "vad_proc")
# (no LOOSE_16K: oracle/ns16k_oracle.c has no counterparts of waveproc / vad_decide / vad_proc -- the variant ends at NoiseSup)

# branches no input of the entry points can take: (file, function, source text, gcov branch index) -> reason
UNREACHABLE = {
    ("ns_oracle.c", "ns_vad", "if (nb < 2147483647) nb++;", 1):
        "the frame counter saturating needs 2^31 - 1 frames (5.4 years of audio) in one utterance",
    ("ns16k_oracle.c", "vad16", "if (nb < 2147483647) nb++;", 1):
        "the frame counter saturating needs 2^31 - 1 frames in one stream",
    ("ns_oracle.c", "vad_decide", "feat15[14] = (v->vCount || v->hCount || trigger >= 3) ? 1.0f : 0.0f;", 4):
        "`trigger >= 3` evaluated true after vCount and hCount were both 0: three lines above, trigger >= 3 sets vCount = 5",
}

# reachable branches of LOOSE_8K that no input of either set reaches: (file, function, source text, branch) -> inputs tried.
# Empty: square4_burst reaches waveproc's four `&& found` exits, low_tone_in_noise and square4_burst the single-measure
# cases of vad_proc.
UNREACHED = {}


@functools.lru_cache(maxsize=None)
def _measured():
    from tools import oracle_coverage as C
    try:
        return C.measure(("gpu-tests", "both"))
    except RuntimeError as e:            # gcc / gcov missing
        pytest.fail(str(e))


def _key(b):
    return (b.file, b.function, b.text, b.index)


def _untaken(per_file, fname, functions):
    from tools import oracle_coverage as C
    found = {b.function for b in per_file[fname]}
    assert set(functions) <= found, f"{fname}: gcov reports no branches for {sorted(set(functions) - found)} (renamed?)"
    return [b for b in C.untaken(per_file[fname], set(functions))]


def test_both_sets_take_every_branch_of_the_frame_loop():
    from tools import oracle_coverage as C
    both = _measured()["both"]
    for fname in ("ns_oracle.c", "ns16k_oracle.c"):
        t, n = C.share(both[fname])
        print(f"{fname}: {t} of {n} branches taken by the GPU tests' inputs and the edge set")
    for fname, functions in (("ns_oracle.c", FULL_8K), ("ns16k_oracle.c", FULL_16K)):
        left = [b for b in _untaken(both, fname, functions) if _key(b) not in UNREACHABLE]
        assert not left, f"{fname}: branches of the frame loop never taken: " + "; ".join(f"{b.function} :{b.line} branch {b.index} `{b.text}`" for b in left)
    loose = [b for b in _untaken(both, "ns_oracle.c", LOOSE_8K) if _key(b) not in UNREACHABLE]
    assert len(UNREACHED) <= 4 and all(UNREACHED.values())
    extra = [b for b in loose if _key(b) not in UNREACHED]
    assert not extra, "ns_oracle.c: unlisted branches never taken: " + "; ".join(f"{b.function} :{b.line} branch {b.index} `{b.text}`" for b in extra)
    # the lists hold nothing that is in fact taken (a stale entry would hide a later loss)
    untaken_keys = {_key(b) for f in both for b in C.untaken(both[f])}
    stale = [k for k in list(UNREACHABLE) + list(UNREACHED) if k not in untaken_keys]
    assert not stale, f"listed as never taken, but taken (or the source line changed): {stale}"


def test_the_older_gpu_inputs_alone_do_not():
    from tools import oracle_coverage as C
    old = _measured()["gpu-tests"]
    for fname in ("ns_oracle.c", "ns16k_oracle.c"):
        t, n = C.share(old[fname])
        print(f"{fname}: {t} of {n} branches taken by the GPU tests' inputs alone")
    left8 = [b for b in _untaken(old, "ns_oracle.c", FULL_8K) if _key(b) not in UNREACHABLE]
    left16 = [b for b in _untaken(old, "ns16k_oracle.c", FULL_16K) if _key(b) not in UNREACHABLE]
    for b in left8 + left16:
        print(f"  {b.file} {b.function} :{b.line} branch {b.index}   {b.text}")
    assert left8 and left16, "the older inputs now take every branch: the record in this file's docstring is out of date"


def test_edge_set_stays_small():
    from tests import ns_edge_cases as E
    s = E.signals_8k()
    total = sum(len(x) for x in s.values())
    print(f"{len(s)} signals, {total} samples at 8 kHz")
    assert total < 400000
    assert all(x.dtype.name == "int16" for x in s.values())
    assert all(x.dtype.name == "float32" and len(x) % 160 == 0 for x in E.streams_16k().values())
    assert all(f.__doc__ for f in E._SIGNALS_8K)
