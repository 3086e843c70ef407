#!/usr/bin/env python3
"""tools/wb_oracle_coverage.py -- which branch outcomes of the REFERENCE's own wideband (16 kHz) code a set of test inputs takes
(CPU only).

The wideband GPU tests compare the kernels with the reference's code run live (tests/wb_reference.py, tests/wb_afe_reference.py
on oracle/_ref/libetsi_ref.so); an outcome of a branch that their inputs never take is a rule the kernels restate and no test
sees.  `make -C oracle refcov` builds the same library at -O0 --coverage into oracle/_ref/cov/ where the reference's sources
are; this tool points the two trace modules' REF_LIB at it in a child process (the counters are written when the process that
loaded the library ends), runs a named input set through both traces and reads `gcov -b -c --json-format`:

    python tools/wb_oracle_coverage.py --set wb-tests    what the wideband GPU tests fed before the edge set existed
    python tools/wb_oracle_coverage.py --set edge        the edge signals of tests/ns_edge_cases.signals_wb()
    python tools/wb_oracle_coverage.py --set both
    ... --only NAME[,NAME]                               (edge) only these signals: what one signal is there for
    ... --first FILE:LINE:INDEX[,...]                    (edge, with --only NAME) the frame of that signal at which each outcome
                                                         is first taken (one child per prefix: a bisection)

It prints, per file, the share of outcomes taken and, per data-path function, the outcomes never taken.  A branch is named by
file, function, line and gcov's branch index -- never by its text, which is the reference's.  The counters go to a temporary
directory (GCOV_PREFIX), so oracle/_ref/cov/ is only read.  tests/test_wb_edge_coverage_cpu.py asserts on measure()."""
import argparse
import collections
import glob
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COV_DIR = os.path.join(ROOT, "oracle", "_ref", "cov")
COV_LIB = os.path.join(COV_DIR, "libetsi_ref_cov.so")
# the reference's files on the wideband data path -> the compilation unit whose counters hold them (NoiseSup.c and CompCeps.c
# are compiled through the two drivers, as in `make ref`)
UNITS = collections.OrderedDict([("16kHzProcessing.c", "16kHzProcessing"), ("NoiseSup.c", "ref_driver"), ("CompCeps.c", "ref_driver_cc"),
                                 ("VAD.c", "VAD"), ("WaveProc.c", "WaveProc"), ("PostProc.c", "PostProc")])
FILES = tuple(UNITS)
SETS = ("wb-tests", "edge", "both")
# not the data path: allocation, initialisation, release (their branches are allocation failures and configuration)
_NOT_DATA = re.compile(r"(Alloc|Init|Delete|Free|Release)", re.I)

Branch = collections.namedtuple("Branch", "file function line index taken")


def is_data_path(function):
    return function is not None and not _NOT_DATA.search(function)


class CoverageRun:
    """The instrumented library with its counters in a temporary directory.  run() adds a set's executions to the counters
    (they accumulate over runs, as gcov's do); reset() zeroes them; branches() reads them."""

    def __init__(self):
        for tool in ("gcc", "gcov"):
            if shutil.which(tool) is None:
                raise RuntimeError(f"{tool} not found: the coverage measurement needs gcc and gcov")
        if not os.path.exists(COV_LIB):
            raise FileNotFoundError(f"{COV_LIB} is missing: build it with `make -C oracle refcov` where the reference's sources are")
        self.dir = tempfile.mkdtemp(prefix="wb_oracle_cov_")
        for unit in set(UNITS.values()):
            shutil.copy(os.path.join(COV_DIR, unit + ".gcno"), self.dir)

    def run(self, name, only=None, frames=None):
        """a child process per run; GCOV_PREFIX_STRIP larger than any path's depth leaves the bare file name under GCOV_PREFIX"""
        cmd = [sys.executable, os.path.abspath(__file__), "--child", COV_LIB, "--set", name]
        if only:
            cmd += ["--only", ",".join(only)]
        if frames is not None:
            cmd += ["--frames", str(frames)]
        env = dict(os.environ, GCOV_PREFIX=self.dir, GCOV_PREFIX_STRIP="99")
        subprocess.check_call(cmd, cwd=ROOT, env=env)

    def reset(self):
        for f in glob.glob(os.path.join(self.dir, "*.gcda")):
            os.remove(f)

    def branches(self):
        """{file: [Branch, ...]} from `gcov -b -c --json-format` (conditional branches only; a line that never ran counts as
        untaken).  The JSON form names lines, functions and branches from the notes file alone, so it reads the same where
        the reference's sources are absent (the text form lists no branch of a file it cannot open)."""
        res = {}
        for f, unit in UNITS.items():
            subprocess.check_call(["gcov", "-b", "-c", "--json-format", unit + ".gcda"], cwd=self.dir, stdout=subprocess.DEVNULL,
                                  stderr=subprocess.DEVNULL)
            with gzip.open(os.path.join(self.dir, unit + ".gcov.json.gz"), "rt") as fh:
                doc = json.load(fh)
            res[f] = [Branch(f, line.get("function_name"), int(line["line_number"]), i, int(br["count"]))
                      for entry in doc["files"] if os.path.basename(entry["file"]) == f
                      for line in entry["lines"] for i, br in enumerate(line["branches"])]
            if not res[f]:
                raise RuntimeError(f"gcov reports no branch of {f} in {unit}.gcno")
        return res

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def untaken(branches, data_path_only=True):
    """the Branch entries never taken, by default of the data-path functions only"""
    return [b for b in branches if b.taken == 0 and (not data_path_only or is_data_path(b.function))]


def share(branches):
    return (sum(b.taken > 0 for b in branches), len(branches))


def measure(sets=SETS):
    """{set name: {file: [Branch]}} for the given sets; `both` is wb-tests followed by edge"""
    res = {}
    with CoverageRun() as cr:
        if "wb-tests" in sets or "both" in sets:
            cr.run("wb-tests")
            if "wb-tests" in sets:
                res["wb-tests"] = cr.branches()
        if "both" in sets:
            cr.run("edge")
            res["both"] = cr.branches()
        if "edge" in sets:
            cr.reset()
            cr.run("edge")
            res["edge"] = cr.branches()
    return res


def takes(cr, name, frames):
    """the (file, function, line, index) of every outcome the first `frames` frames of edge signal `name` take, on a reset run"""
    cr.reset()
    cr.run("edge", [name], frames)
    return {(b.file, b.function, b.line, b.index) for br in cr.branches().values() for b in br if b.taken}


def first_frames(name, where):
    """{(file, line, index): the frame f of edge signal `name` at which the reference first takes that outcome (the prefix of
    f + 1 frames takes it, the prefix of f frames does not), or None if the whole signal does not}.  Bisection over prefixes,
    one child per prefix; an outcome taken by a prefix is taken by every longer one because the reference's state at a frame
    depends on earlier frames only (an outcome of the flush is the exception: it belongs to the utterance's end)."""
    from tests import ns_edge_cases as E
    nfr = len(E.signals_wb()[name]) // 160
    res = {}
    with CoverageRun() as cr:
        cache = {}

        def taken(n, w):
            if n not in cache:
                cache[n] = {(f, line, idx) for f, _, line, idx in takes(cr, name, n)}
            return w in cache[n]
        for w in where:
            if not taken(nfr, w):
                res[w] = None
                continue
            lo, hi = 0, nfr             # invariant: the prefix of lo frames does not take it, the prefix of hi frames does
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if taken(mid, w):
                    hi = mid
                else:
                    lo = mid
            res[w] = hi - 1
    return res


# ---- the input sets (run in the child process, on the instrumented build) -----------------------------------------
def wb_tests_inputs():
    """what the wideband GPU tests fed before the edge set: tests/test_gpu_wb.py's live batch, both fixtures' utterances,
    tests/test_gpu_wb_afe.py's edge batch and the four signals signals_wb() carried over from the 8 kHz recipes"""
    import numpy as np
    from tests import ns_edge_cases as E
    from tests import test_gpu_wb as WB
    from tests import test_gpu_wb_afe as WA
    utts = list(WB._live_batch()[0])
    for gold in (WB.GOLD, WA.GOLD):
        with np.load(gold) as z:
            utts += [z[k] for k in sorted(z.files) if re.fullmatch(r"x\d+", k)]
    utts += list(WA._edge_batch()[0])
    sig = E.signals_wb()
    utts += [sig[k] for k in E.WB_CARRIED]
    return utts


def edge_inputs(only=None):
    from tests import ns_edge_cases as E
    sig = E.signals_wb()
    names = [k for k in sig if k not in E.WB_CARRIED]
    if only:
        unknown = [k for k in only if k not in sig]
        if unknown:
            raise SystemExit(f"no such wideband signal: {unknown}; there are {list(sig)}")
        names = list(only)
    return [sig[k] for k in names]


def _child(lib, name, only, frames):
    from tests import wb_afe_reference as A
    from tests import wb_reference as W
    W.REF_LIB = lib
    utts = []
    if name in ("wb-tests", "both"):
        utts += wb_tests_inputs()
    if name in ("edge", "both"):
        utts += edge_inputs(only)
    for x in utts:
        if frames is not None:
            x = x[:160 * frames]
        W.trace(x)
        A.trace(x)


def report(per_file, out=sys.stdout):
    for f in FILES:
        br = per_file[f]
        t, n = share(br)
        out.write(f"{f}: {t} of {n} outcomes taken ({100.0 * t / max(n, 1):.1f} %)\n")
        by_fn = collections.OrderedDict()
        for b in untaken(br):
            by_fn.setdefault(b.function, []).append(b)
        for fn, lst in by_fn.items():
            out.write(f"  {fn}: " + ", ".join(f":{b.line} branch {b.index}" for b in lst) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", choices=SETS, default="both")
    ap.add_argument("--only", default=None, help="(edge) comma-separated signal names")
    ap.add_argument("--first", default=None, help="(edge, one --only NAME) comma-separated FILE:LINE:INDEX")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--frames", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    only = a.only.split(",") if a.only else None
    if a.child:
        _child(a.child, a.set, only, a.frames)
        return
    if a.first:
        if not only or len(only) != 1:
            ap.error("--first needs --only with one signal name")
        where = [(w.split(":")[0], int(w.split(":")[1]), int(w.split(":")[2])) for w in a.first.split(",")]
        for (f, line, idx), n in first_frames(only[0], where).items():
            print(f"{only[0]}: {f}:{line} branch {idx} " + ("is never taken" if n is None else f"is first taken at frame {n}"))
        return
    with CoverageRun() as cr:
        cr.run(a.set, only)
        report(cr.branches())


if __name__ == "__main__":
    main()
