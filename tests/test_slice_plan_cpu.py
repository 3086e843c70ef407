"""CPU test of csrc/slice_plan.h, the cut along the time axis that sea_denoise_utterances, sea_wb_denoise_utterances and
sea_packed_plan share: tests/slice_plan_driver.cpp, compiled with the address and undefined-behaviour sanitizers as a
stand-alone program, prints the plan and every slice's offsets | lengths rows; every number must equal an independent
restatement of the rule (a linear scan for each boundary where the header bisects).

The rule: utterances sorted longest first (stable), nfr = length // hop; want = min(want, 64, max(1, max_fr // 8)); B[k] is
the smallest f > B[k-1] with sum_j min(nfr[j], f) >= total_fr * k // want, boundaries stop at the first such f >= max_fr,
and the last one is max_fr; slice k holds frames [B[k], B[k+1]) of the first nact[k] sorted utterances, those with
nfr > B[k].

The driver's second command runs RowOrder, the in-order placement of the rows the slices of a pipeline emit: whatever order the
slices arrive in, slice k is cut once it and every slice before it have arrived, its rows start behind the earlier slices'."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
WANTS = (1, 2, 7, 8, 10, 40)


def _lists(hop):
    """name -> (lengths in samples, slice counts asked for)"""
    r11, r23 = np.random.default_rng(11), np.random.default_rng(23)
    return {
        # the lists of test_gpu_parity.py's pipeline tests
        "seed 11": ([int(v) for v in r11.integers(0, 40000, 90)] + [0, 79, 80, 81, 24000, 24000, 24037], WANTS),
        "seed 23": ([int(v) for v in r23.integers(0, 48000, 60)] + [0, 79, 80, 161, 32000, 32000, 31999], WANTS),
        "nothing reaches a frame": ([0, hop - 1, 1, hop // 2], (1, 8)),
        "seven frames": ([7 * hop + 3], (1, 8)),                              # max_fr // 8 == 0: one slice
        "12 000 frames, 100 asked for": ([12000 * hop], (100,)),              # the cap of 64
        "50 equal": ([333 * hop + 5] * 50, WANTS),                            # every slice has the full prefix
        "one long, forty of one frame": ([800 * hop] + [hop] * 40, WANTS),    # shares reached at once: boundaries 1, 2, 3, ...
        "empty list": ([], (8,)),
    }


def _restate(lengths, hop, want):
    n = len(lengths)
    idx = sorted(range(n), key=lambda u: -lengths[u])                         # sorted() is stable
    inv = [0] * n
    for j, u in enumerate(idx):
        inv[u] = j
    nfr = [lengths[u] // hop for u in idx]
    total_fr, max_fr = sum(nfr), (nfr[0] if n else 0)
    plan = dict(idx=idx, inv=inv, nfr=nfr, total_fr=[total_fr], max_fr=[max_fr])
    if total_fr == 0:
        plan.update(K=[0], B=[0], nact=[], foff=[0], mbase=[0], rows={})
        return plan
    want = min(want, 64, max(1, max_fr // 8))
    a = np.array(nfr, np.int64)
    B = [0]
    for k in range(1, want):
        share = total_fr * k // want
        f = B[-1] + 1
        while int(np.minimum(a, f).sum()) < share:
            f += 1
        if f >= max_fr:
            break
        B.append(f)
    B.append(max_fr)
    K = len(B) - 1
    nact = [sum(1 for x in nfr if x > B[k]) for k in range(K)]
    piece = [[hop * (min(nfr[j], B[k + 1]) - B[k]) for j in range(nact[k])] for k in range(K)]
    foff, mbase = [0], [0]
    for k in range(K):
        foff.append(foff[-1] + sum(piece[k]) // hop)
        mbase.append(mbase[-1] + 2 * nact[k])
    rows = {}
    for k in range(K):
        for conv, start in (("abs", hop * foff[k]), ("rel", 0)):
            offs = [start + sum(piece[k][:j]) for j in range(nact[k])]
            rows[k, conv] = (offs, piece[k], [2 * sum(piece[k][:j]) for j in range(nact[k] + 1)])
    plan.update(K=[K], B=B, nact=nact, foff=foff, mbase=mbase, rows=rows)
    return plan


def _parse(text):
    plans, cur = [], None
    for ln in text.splitlines():
        tok = ln.split()
        if tok[0] == "case":
            cur = dict(rows={})
        elif tok[0] == "end":
            plans.append(cur)
        elif tok[0] == "rows":
            parts = " ".join(tok[3:]).split("|")
            cur["rows"][int(tok[1]), tok[2]] = tuple([int(v) for v in part.split()] for part in parts)
        else:
            cur[tok[0]] = [int(v) for v in tok[1:]]
    return plans


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/slice_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("slice_plan") / "slice_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "slice_plan_driver.cpp"), "-o", exe])
    return exe


def test_slice_plan_equals_the_rule(driver):
    cases = [(hop, name, lengths, want) for hop in (80, 160) for name, (lengths, wants) in _lists(hop).items() for want in wants]
    stdin = "".join(f"{hop} {want} {len(lengths)} {' '.join(map(str, lengths))}\n" for hop, _, lengths, want in cases)
    run = subprocess.run([driver], input=stdin, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    plans = _parse(run.stdout)
    assert len(plans) == len(cases)
    seen_K = set()
    for (hop, name, lengths, want), got in zip(cases, plans):
        what = f"{name}, hop {hop}, {want} asked for"
        ref = _restate(lengths, hop, want)
        for key in ("K", "total_fr", "max_fr", "idx", "inv", "nfr", "B", "nact", "foff", "mbase"):
            assert got[key] == ref[key], f"{what}: {key} differs"
        assert got["rows"] == ref["rows"], f"{what}: offsets | lengths rows differ"

        # properties that hold for any list, stated on the driver's output alone
        K, B, nact, nfr, idx, inv = got["K"][0], got["B"], got["nact"], got["nfr"], got["idx"], got["inv"]
        seen_K.add(K)
        assert all(inv[idx[j]] == j for j in range(len(lengths))), f"{what}: inv is not idx's inverse"
        if K == 0:
            assert sum(nfr) == 0
            continue
        assert B[0] == 0 and B[-1] == got["max_fr"][0] and all(b0 < b1 for b0, b1 in zip(B, B[1:])), f"{what}: B = {B}"
        assert all(n0 >= n1 for n0, n1 in zip(nact, nact[1:])) and nact[0] == sum(1 for x in nfr if x > 0), f"{what}: nact = {nact}"
        end = [0] * len(lengths)                                  # where the pieces of sorted position j have got to, in samples
        for k in range(K):
            offs, lens, _ = got["rows"][k, "abs"]
            rel = got["rows"][k, "rel"][0]
            assert rel[0] == 0 and offs[0] == hop * got["foff"][k] and [o - offs[0] for o in offs] == rel
            assert all(o + L == o1 for o, L, o1 in zip(offs, lens, offs[1:])) and offs[-1] + lens[-1] == hop * got["foff"][k + 1], \
                f"{what}: slice {k} is not packed back to back"
            for j in range(len(lengths)):
                if j < nact[k]:
                    assert end[j] == hop * B[k] and lens[j] > 0, f"{what}: slice {k} does not continue position {j}"
                    end[j] += lens[j]
                else:
                    assert nfr[j] <= B[k]
        assert end == [hop * x for x in nfr], f"{what}: the pieces do not tile the whole frames"
    assert {0, 1, 8, 10, 40, 64} <= seen_K


def test_slice_plan_named_cases(driver):
    """The caps and the degenerate lists, as numbers."""
    hop = 160
    lines = [
        f"{hop} 8 4 0 {hop - 1} 1 17",                                 # no whole frame
        f"{hop} 8 1 {7 * hop}",                                        # max_fr // 8 == 0
        f"{hop} 100 1 {12000 * hop}",                                  # 64 at the most
        f"{hop} 10 50 " + " ".join([str(333 * hop)] * 50),             # equal lengths
    ]
    run = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    none, seven, capped, equal = _parse(run.stdout)
    assert none["K"] == [0] and none["total_fr"] == [0]
    assert seven["K"] == [1] and seven["B"] == [0, 7]
    assert capped["K"] == [64] and len(capped["B"]) == 65
    assert equal["K"] == [10] and equal["nact"] == [50] * 10


def _order_lists(hop):
    """name -> (lengths in samples, slice count asked for, K the plan must come to)"""
    r5 = np.random.default_rng(5)
    return {
        "one slice": ([50 * hop, 20 * hop + 3, 0, 9 * hop], 1, 1),
        "two slices": ([50 * hop, 20 * hop + 3, 0, 9 * hop, hop - 1, 50 * hop], 2, 2),
        "five slices": ([int(v) for v in r5.integers(0, 400 * hop, 30)] + [0, hop, 400 * hop], 5, 5),
        "64 slices": ([1000 * hop, 900 * hop + 1, 600 * hop, 40 * hop, 0, 3 * hop], 100, 64),
    }


def _arrival_orders(K, rng):
    ident = list(range(K))
    pairs = [k ^ 1 if (k ^ 1) < K else k for k in ident]                      # k + 1 before k, for every even k
    return [ident, ident[::-1], pairs] + [[int(v) for v in rng.permutation(K)] for _ in range(3)]


def test_row_order_cuts_in_slice_order_whatever_arrives_first(driver):
    rng = np.random.default_rng(31)
    cases = []
    for hop in (80, 160):
        for name, (lengths, want, K) in _order_lists(hop).items():
            plan = _restate(lengths, hop, want)
            assert plan["K"] == [K], f"{name}: the list was meant to give {K} slices"
            nact, B, nfr = plan["nact"], plan["B"], plan["nfr"]
            for arrival in _arrival_orders(K, rng):
                # rows emitted per slice and sorted position: anything from none to the piece's frames + the 6 rows of a flush
                cnt = np.zeros((K, len(lengths)), np.int64)
                for k in range(K):
                    frames = np.array([min(nfr[j], B[k + 1]) - B[k] for j in range(nact[k])])
                    c = rng.integers(0, frames + 7)
                    c[rng.random(nact[k]) < 0.2] = 0
                    top = rng.random(nact[k]) < 0.2
                    c[top] = frames[top] + 6
                    cnt[k, :nact[k]] = c
                cases.append((f"{name}, hop {hop}, arrival {arrival[:8]}", lengths, hop, want, nact, arrival, cnt))
    stdin = "".join(f"{hop} {want} {len(lengths)} {' '.join(map(str, lengths))} {' '.join(map(str, arrival))} "
                    f"{' '.join(str(int(v)) for k in range(len(nact)) for v in cnt[k, :nact[k]])}\n"
                    for _, lengths, hop, want, nact, arrival, cnt in cases)
    run = subprocess.run([driver, "order"], input=stdin, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    blocks = [b.split("\n") for b in run.stdout.split("case\n")[1:]]
    assert len(blocks) == len(cases)
    for (what, lengths, hop, want, nact, arrival, cnt), lines in zip(cases, blocks):
        K = len(nact)
        want_start = np.cumsum(cnt, axis=0) - cnt                             # the sum of cnt[k'][j] over k' < k
        want_pos = cnt.sum(axis=0)                                            # ... over all k
        arrived, cut, start, pos = [], [], {}, None
        for tok in (ln.split() for ln in lines if ln):
            if tok[0] == "arrive":
                arrived.append(int(tok[1]))
            elif tok[0] == "cut":
                k = int(tok[1])
                assert set(range(k + 1)) <= set(arrived), f"{what}: slice {k} was cut with only {arrived} on the host"
                assert not set(range(k + 1)) <= set(arrived[:-1]), f"{what}: slice {k} could have been cut an arrival earlier"
                cut.append(k)
            elif tok[0] == "start":
                start[int(tok[1])] = [int(v) for v in tok[2:]]
            elif tok[0] == "pos":
                pos = [int(v) for v in tok[1:]]
        assert arrived == arrival
        assert cut == list(range(K)), f"{what}: cut in the order {cut}"
        assert list(start) == cut
        for k in range(K):
            assert start[k] == [int(v) for v in want_start[k, :nact[k]]], f"{what}: start rows of slice {k}"
        assert pos == [int(v) for v in want_pos], f"{what}: totals"
