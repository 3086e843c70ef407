#!/usr/bin/env python3
"""tools/oracle_coverage.py -- which branches of the CPU restatements a set of test inputs takes (CPU only).

Every GPU parity test compares a kernel with oracle/ns_oracle.c / ns16k_oracle.c on some inputs; a branch of the
restatement that those inputs never take is arithmetic that the kernels carry too and that no test sees.  This tool
compiles the three restatements with oracle/Makefile's parity flags at -O0 --coverage into a TEMPORARY directory (one
compile per file, so that the notes files are named after the sources), loads that build through oracle.oracle's
classes in a child process, runs a named input set and reads `gcov -b -c`:

    python tools/oracle_coverage.py --set gpu-tests     what the GPU tests of the NoiseSup path feed (their own helpers)
    python tools/oracle_coverage.py --set edge          tests/ns_edge_cases.py
    python tools/oracle_coverage.py --set both
    ... --only NAME[,NAME]                              (edge) only these signals: what one signal is there for

It prints, per file, the share of branches taken and, per function, the branches never taken with line and source text.
tests/test_edge_coverage_cpu.py asserts on measure()."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ORACLE_DIR = os.path.join(ROOT, "oracle")
FILES = ("ns_oracle.c", "ns16k_oracle.c", "resynth_oracle.c")
SETS = ("gpu-tests", "edge", "both")

Branch = collections.namedtuple("Branch", "file function line index taken text")


def parity_flags():
    """the PARITY line of oracle/Makefile with its optimisation level replaced"""
    with open(os.path.join(ORACLE_DIR, "Makefile")) as fh:
        m = re.search(r"^PARITY\s*:=\s*(.*)$", fh.read(), re.M)
    if not m:
        raise RuntimeError("oracle/Makefile: no PARITY line")
    return [f for f in m.group(1).split() if not f.startswith("-O")] + ["-O0", "--coverage"]


class CoverageBuild:
    """One instrumented build in a temporary directory.  run() adds a set's executions to the counters (they accumulate
    over runs, as gcov's do); reset() zeroes them; branches() reads them."""

    def __init__(self):
        for tool in ("gcc", "gcov"):
            if shutil.which(tool) is None:
                raise RuntimeError(f"{tool} not found: the coverage measurement needs gcc and gcov")
        self.dir = tempfile.mkdtemp(prefix="oracle_cov_")
        flags = parity_flags()
        objs = []
        for f in FILES:
            obj = os.path.splitext(f)[0] + ".o"
            subprocess.check_call(["gcc"] + flags + ["-w", "-I", ORACLE_DIR, "-c", os.path.join(ORACLE_DIR, f), "-o", obj], cwd=self.dir)
            objs.append(obj)
        self.lib = os.path.join(self.dir, "libsea_oracle_cov.so")
        subprocess.check_call(["gcc", "--coverage", "-shared", "-o", self.lib] + objs + ["-lm"], cwd=self.dir)

    def run(self, name, only=None):
        """the counters are written when the process that loaded the library ends: a child process per run"""
        cmd = [sys.executable, os.path.abspath(__file__), "--child", self.lib, "--set", name]
        if only:
            cmd += ["--only", ",".join(only)]
        subprocess.check_call(cmd, cwd=ROOT)

    def reset(self):
        for f in os.listdir(self.dir):
            if f.endswith(".gcda"):
                os.remove(os.path.join(self.dir, f))

    def branches(self):
        """{file: [Branch, ...]} from `gcov -b -c` (conditional branches only; a line that never ran counts as untaken)"""
        res = {}
        for f in FILES:
            subprocess.check_call(["gcov", "-b", "-c", "-o", self.dir, os.path.join(ORACLE_DIR, f)], cwd=self.dir,
                                  stdout=subprocess.DEVNULL)
            res[f] = _parse_gcov(os.path.join(self.dir, f + ".gcov"), f)
        return res

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_FUNC = re.compile(r"^function (\S+) called")
_LINE = re.compile(r"^\s*(\S+):\s*(\d+):(.*)$")
_BR = re.compile(r"^branch\s+(\d+) (?:taken (\d+)|never executed)")


def _parse_gcov(path, fname):
    out, func, line, text = [], None, 0, ""
    with open(path, errors="replace") as fh:
        for row in fh:
            m = _FUNC.match(row)
            if m:
                func = m.group(1)
                continue
            m = _BR.match(row)
            if m:
                out.append(Branch(fname, func, line, int(m.group(1)), int(m.group(2) or 0), text))
                continue
            m = _LINE.match(row)
            if m:
                line, text = int(m.group(2)), m.group(3).strip()
    return out


def untaken(branches, functions=None):
    """the Branch entries never taken, optionally of the named functions only"""
    return [b for b in branches if b.taken == 0 and (functions is None or b.function in functions)]


def share(branches):
    n = len(branches)
    return (sum(b.taken > 0 for b in branches), n)


def measure(sets=SETS):
    """{set name: {file: [Branch]}} for the given sets, one build; `both` is gpu-tests followed by edge"""
    res = {}
    with CoverageBuild() as cb:
        if "gpu-tests" in sets or "both" in sets:
            cb.run("gpu-tests")
            if "gpu-tests" in sets:
                res["gpu-tests"] = cb.branches()
        if "both" in sets:
            cb.run("edge")
            res["both"] = cb.branches()
        if "edge" in sets:
            cb.reset()
            cb.run("edge")
            res["edge"] = cb.branches()
    return res


# ---- the input sets (run in the child process, on the instrumented build) -----------------------------------------
def _run_8k(ora, utts):
    for x in utts:
        ora.ns_trace(x, want_state=False)
        ora.afe_trace(x)


def run_gpu_tests_inputs(ora):
    """what the GPU parity tests of the 8 kHz NoiseSup path, its feature chain and the 16 k-native variant feed, from the
    test modules' own helpers"""
    import numpy as np
    from oracle import oracle as O
    from speech_enhancement_amd import corpus
    from tests import test_gpu_ns16k as N
    from tests import test_gpu_parity as P
    utts = P._mixed_corpus() + [O.kat_ns_signal()] + P._short_utterances()[::37]
    utts += [np.zeros(480, np.int16), corpus.synth_utterance(31, 32000)]     # test_afe_feature_chain_vs_oracle's two more
    _run_8k(ora, utts)
    for nfr in (140, 90):
        for s in N._streams(nfr):
            ora.ns16k_new().push(s)
    g = np.load(os.path.join(N.GOLD, "ns16k_golden.npz"))
    for name in ("plain", "gated"):
        ora.ns16k_new().push(g[f"{name}/in"])


def run_edge_inputs(ora, only=None):
    from tests import ns_edge_cases as E
    s8, s16 = E.signals_8k(), E.streams_16k()
    if only:
        s8 = {k: v for k, v in s8.items() if k in only}
        s16 = {k: v for k, v in s16.items() if k in only}
    _run_8k(ora, s8.values())
    for x in s16.values():
        ora.ns16k_new().push(x)


def _child(lib, name, only):
    from oracle import oracle as O
    ora = O.Oracle(path=lib)
    x, m = O.kat_resynth_case(3200)                 # the third file is measured too (nothing is asserted about it)
    ora.resynth64(x, m)
    if name in ("gpu-tests", "both"):
        run_gpu_tests_inputs(ora)
    if name in ("edge", "both"):
        run_edge_inputs(ora, only)


def report(per_file, out=sys.stdout):
    for f in FILES:
        br = per_file[f]
        t, n = share(br)
        out.write(f"{f}: {t} of {n} branches taken ({100.0 * t / max(n, 1):.1f} %)\n")
        by_fn = collections.OrderedDict()
        for b in untaken(br):
            by_fn.setdefault(b.function, []).append(b)
        for fn, lst in by_fn.items():
            out.write(f"  {fn}:\n")
            for b in lst:
                out.write(f"    :{b.line} branch {b.index}   {b.text}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", choices=SETS, default="both")
    ap.add_argument("--only", default=None, help="(edge) comma-separated signal names")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    only = a.only.split(",") if a.only else None
    if a.child:
        _child(a.child, a.set, only)
        return
    with CoverageBuild() as cb:
        cb.run(a.set, only)
        report(cb.branches())


if __name__ == "__main__":
    main()
