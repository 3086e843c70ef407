"""CPU test of csrc/chunk_plan.h, the cut that the entry points for lists of utterances in host memory share (scores, STOI, the
DNN estimator, the training-set builder, the Hu-Wang chain at 16 kHz): tests/chunk_plan_driver.cpp, compiled with the address
and undefined-behaviour sanitizers as a stand-alone program, prints the cuts, every chunk's totals and their maxima; every
number must equal an independent restatement of the rule, which is the reference here, not the header.

The rule: utterances in list order; from a chunk's first utterance on, the chunk takes the next one as long as the footprint of
the chunk with it stays within the budget, and it always takes its first.  The footprint is a function of the chunk's totals
(the sums of its utterances' quantities) and of its number of utterances; in the additive form it is the sum of the
utterances' bytes.  The restatement finds each chunk's end by trying the ends one after the other with sums of its own, where
the header carries one running total through one loop."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
HUGE = 2 ** 60


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/chunk_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("chunk_plan") / "chunk_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "chunk_plan_driver.cpp"), "-o", exe])
    return exe


def _run(driver, lines):
    run = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    return run.stdout


def _plans(text):
    plans, cur = [], {}
    for ln in text.splitlines():
        tok = ln.split()
        if tok[0] == "end":
            plans.append(cur)
            cur = {}
        else:
            cur[tok[0]] = [int(v) for v in tok[1:]]
    return plans


def _restate(items, budget, footprint):
    """items: per utterance its tuple of quantities -> cuts"""
    n, cuts = len(items), [0]
    while cuts[-1] < n:
        first = end = cuts[-1]
        end += 1                                                              # a chunk always takes its first utterance
        while end < n and footprint([sum(q) for q in zip(*items[first:end + 1])], end + 1 - first) <= budget:
            end += 1
        cuts.append(end)
    return cuts if n else [0, 0]


def _check(what, got, items, budget, footprint):
    n, width = len(items), len(items[0]) if items else len(got["max"])
    cuts = got["cuts"]
    assert cuts == _restate(items, budget, footprint), f"{what}: cuts {cuts}"
    # properties, stated on the driver's output alone
    assert cuts[0] == 0 and cuts[-1] == n and got["chunks"] == [len(cuts) - 1], f"{what}: cuts {cuts}"
    if n == 0:
        assert cuts == [0, 0] and got["max"] == [0] * width and got["max_n"] == [0] and got["sum"] == [0] * width
        return
    assert all(a < b for a, b in zip(cuts, cuts[1:])), f"{what}: cuts {cuts} do not increase strictly"
    sums = [[sum(q[i] for q in items[a:b]) for i in range(width)] for a, b in zip(cuts, cuts[1:])]
    assert got["sum"] == [v for s in sums for v in s], f"{what}: the chunks' totals"
    assert got["max"] == [max(s[i] for s in sums) for i in range(width)], f"{what}: max is not the elementwise maximum"
    assert got["max_n"] == [max(b - a for a, b in zip(cuts, cuts[1:]))], f"{what}: max_n"
    for (a, b), s in zip(zip(cuts, cuts[1:]), sums):
        assert b - a == 1 or footprint(s, b - a) <= budget, f"{what}: chunk [{a}, {b}) exceeds the budget"
        if b < n:
            more = [x + y for x, y in zip(s, items[b])]
            assert footprint(more, b - a + 1) > budget, f"{what}: chunk [{a}, {b}) could have taken utterance {b}"


def _additive(c, n_in_chunk):
    return c[-1]


def _add_line(budget, pairs):
    return f"add {budget} {len(pairs)} " + " ".join(f"{a} {b}" for a, b in pairs)


def test_every_short_list(driver):
    """Every list of up to 6 utterances with 0, 1, 5 or 9 bytes each, at budgets below, at and above what one and two
    utterances take.  The second quantity, which only the maxima see, varies with the position and the bytes."""
    cases = []
    for n in range(7):
        for bytes_ in itertools.product((0, 1, 5, 9), repeat=n):
            pairs = [((5 * u + b) % 7, b) for u, b in enumerate(bytes_)]
            cases += [(budget, pairs) for budget in (0, 1, 9, 10, 14, HUGE)]
    plans = _plans(_run(driver, [_add_line(budget, pairs) for budget, pairs in cases]))
    assert len(plans) == len(cases)
    for (budget, pairs), got in zip(cases, plans):
        what = f"bytes {[b for _, b in pairs]}, budget {budget}"
        _check(what, got, pairs, budget, _additive)
        if budget == HUGE:
            assert got["chunks"] == [1], f"{what}: a budget that holds everything gives one chunk"
        if budget == 0 and all(b > 0 for _, b in pairs):
            # every entry point's utterance has a constant term, so none weighs nothing; utterances of 0 bytes do fit
            # a budget of 0 together, and the maximal-chunk property above then demands that they share a chunk
            assert got["cuts"] == list(range(len(pairs) + 1)) or not pairs, f"{what}: budget 0 gives one utterance per chunk"


def test_random_lists(driver):
    rng = np.random.default_rng(20240607)
    cases = []
    for i in range(300):
        n = int(rng.integers(0, 201))
        top = int(rng.choice([2, 1000, 10 ** 9]))
        pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 50, n), rng.integers(0, top, n))]
        total = sum(b for _, b in pairs)
        budget = [0, 1, top - 1, top, 3 * top, total // 7, total // 2, total - 1, total, HUGE][i % 10]
        cases.append((budget, pairs))
    plans = _plans(_run(driver, [_add_line(budget, pairs) for budget, pairs in cases]))
    assert len(plans) == len(cases)
    counts = set()
    for i, ((budget, pairs), got) in enumerate(zip(cases, plans)):
        _check(f"random list {i} of {len(pairs)}, budget {budget}", got, pairs, budget, _additive)
        counts.add(got["chunks"][0])
    assert 1 in counts and max(counts) > 100, "the lists were meant to give one chunk, many chunks and counts between"


def test_footprint_of_the_totals(driver):
    """A footprint with a term per chunk, A * samples + B * n^2, as the Hu-Wang list's scratch has: not a sum over utterances."""
    rng = np.random.default_rng(64)
    cases = [(0, 1, 2, [3, 4]), (13, 1, 1, [1] * 9), (HUGE, 3, 50, [5, 0, 7]), (40, 0, 2, [9] * 11), (5, 1, 0, [])]
    for i in range(150):
        n = int(rng.integers(0, 121))
        A, B = int(rng.choice([0, 1, 3])), int(rng.choice([0, 2, 50]))
        s = [int(v) for v in rng.integers(0, 400, n)]
        budget = [0, 50, 1000, 20000, A * sum(s) + B * n * n, HUGE][i % 6]
        cases.append((budget, A, B, s))
    plans = _plans(_run(driver, [f"quad {budget} {A} {B} {len(s)} " + " ".join(map(str, s)) for budget, A, B, s in cases]))
    assert len(plans) == len(cases)
    for i, ((budget, A, B, s), got) in enumerate(zip(cases, plans)):
        _check(f"totals case {i} (A {A}, B {B}, budget {budget})", got, [(v,) for v in s], budget,
               lambda c, k, A=A, B=B: A * c[0] + B * k * k)
    # B * n^2 alone: chunks of floor(sqrt(40 / 2)) = 4 utterances whatever they hold
    assert plans[3]["cuts"] == [0, 4, 8, 11] and plans[3]["max"] == [36] and plans[3]["max_n"] == [4]


def test_budget_of(driver):
    """An override is MiB, whatever it says ("-1" gives atoll's -1 MiB: every utterance its own chunk); without one 60 % of the
    free and the held bytes, rounded as (free + held) / 10 * 6 rounds."""
    pairs = [(0, 0), (9, 0), (9, 1), (1000, 0), (10 ** 11, 5 * 10 ** 9), (288 * 2 ** 30, 0)]
    cases = [(text, free, held) for text in ("0", "3", "-1", None) for free, held in pairs]
    out = _run(driver, [f"budget {text or '-'} {free} {held}" for text, free, held in cases]).split()
    got = [int(v) for v in out[1::2]]
    assert out[0::2] == ["budget"] * len(cases)
    assert got == [int(text) * 2 ** 20 if text else (free + held) // 10 * 6 for text, free, held in cases]


def test_pack_padded(driver):
    """L elements, zeros up to the next multiple of 8, and not one element further: the 8 sentinels behind stay."""
    lengths = (0, 1, 7, 8, 9)
    lines = _run(driver, [f"pack {L}" for L in lengths]).splitlines()
    assert len(lines) == 2 * len(lengths)
    for i, L in enumerate(lengths):
        padded = (L + 7) // 8 * 8
        for name, ln in zip(("pack16", "pack32"), lines[2 * i:2 * i + 2]):
            tok = ln.split()
            assert tok[0] == name and int(tok[1]) == padded, f"{name}, L = {L}: returned {tok[1]}"
            assert [int(v) for v in tok[2:]] == list(range(1, L + 1)) + [0] * (padded - L) + [0x7e7e] * 8, f"{name}, L = {L}"
