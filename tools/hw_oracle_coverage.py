#!/usr/bin/env python3
"""tools/hw_oracle_coverage.py -- which branch outcomes of the REFERENCE's own Hu-Wang estimator (HuWang.cpp) a set of test
inputs takes, at both banks: 25 channels at 8 kHz (hw25) and 64 channels at 16 kHz (hw64).  CPU only.

The Hu-Wang kernels are compared bit for bit with arrays that the reference's HuWang.cpp produced (tests/golden/hw25_*,
hw64_*) or with the numpy models pinned to them; an outcome of a branch that no input takes is a rule the kernels restate and
no test sees.  `make -C oracle hwcov` (this file with --build, where the reference's sources are) compiles HuWang.cpp
UNMODIFIED once per bank at -O0 --coverage -ffp-contract=off into a shared library under oracle/_ref/hwcov/<bank>/ and links
the four drivers that the tools/gen_hw*_golden.py hold (front half, pitch, AM, resynthesis: imported, not restated) against
it, so that all four add to one set of counters.  At run time only oracle/_ref/hwcov is needed:

    python tools/hw_oracle_coverage.py --set hw-tests    every input of the eight gen_hw* tools and of the Hu-Wang GPU tests
    python tools/hw_oracle_coverage.py --set edge        the edge inputs (tests/hw25_model.edge_inputs and its siblings)
    python tools/hw_oracle_coverage.py --set both
    ... --bank hw25|hw64                                 one bank only
    ... --only NAME[,NAME]                               (edge) only these inputs: what one input is there for

It prints, per bank and per range of HuWang.cpp, the share of outcomes taken and, per function, the outcomes never taken.  An
outcome is named by bank, function, line and gcov's branch index -- never by its text, which is the reference's.  Outcomes
that gcov marks as exception edges, and those on lines that allocate or release (recorded by line number at build time),
are left out.  The counters go to a temporary directory (GCOV_PREFIX), so oracle/_ref/hwcov/ is only read.
tests/test_hw_edge_coverage_cpu.py asserts on measure()."""
import argparse
import collections
import contextlib
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

COV_DIR = os.path.join(ROOT, "oracle", "_ref", "hwcov")
BANKS = ("hw25", "hw64")
SETS = ("hw-tests", "edge", "both")
DRIVERS = ("front", "pitch", "am", "resynth")
# the ranges of HuWang.cpp the eight tools divide it into: front half, initial grouping and pitch, AM and final grouping,
# resynthesis, the window tools
RANGES = ((1, 465), (466, 1142), (1146, 1494), (1498, 1549), (1553, 1677))
COVFLAGS = ["-O0", "--coverage", "-ffp-contract=off", "-fPIC", "-w"]

Branch = collections.namedtuple("Branch", "bank function line index taken")


def range_of(line):
    for lo, hi in RANGES:
        if lo <= line <= hi:
            return (lo, hi)
    return None


# ---- the tools' modules, per bank ------------------------------------------------------------------------------------
def _tools(bank):
    """the four gen_hw* modules of a bank whose drivers and readers are used: front, pitch, am, resynth"""
    if bank == "hw25":
        from tools import gen_hw25_am_golden as GA
        from tools import gen_hw25_golden as GF
        from tools import gen_hw25_pitch_golden as GP
        from tools import gen_hw25_resynth_golden as GR
        return GF, GP, GA, GR
    from tools import gen_hw64_am_golden as GA
    from tools import gen_hw64_golden as GF
    from tools import gen_hw64_pitch_golden as GP
    from tools import gen_hw64_resynth_golden as GR
    return GF, GP.G, GA.G, GR.G


def _models(bank):
    if bank == "hw25":
        from tests import hw25_am_model as AM
        from tests import hw25_model as M
        from tests import hw25_pitch_model as PM
        from tests import hw25_resynth_model as RM
    else:
        from tests import hw64_am_model as AM
        from tests import hw64_model as M
        from tests import hw64_pitch_model as PM
        from tests import hw64_resynth_model as RM
    return M, PM, AM, RM


# ---- the build (only where the reference's sources are) ---------------------------------------------------------------
def build(ref_root):
    """oracle/_ref/hwcov/<bank>/: libhuwang.so (instrumented), HuWang.gcno, lines.json and the four drivers"""
    from tools import gen_hw25_pitch_golden as GP25
    from tools import gen_hw64_golden as GF64
    src = os.path.join(ref_root, GP25.REL, "HuWang.cpp")
    inc64 = os.path.join(ref_root, GF64.INC)
    if not os.path.exists(src) or not os.path.exists(os.path.join(inc64, "HuWang.h")):
        print(f"hwcov: {src} or {inc64}/HuWang.h absent -- keeping prebuilt oracle/_ref/hwcov (if any)")
        return
    with open(src, errors="replace") as fh:
        alloc = [n for n, text in enumerate(fh, 1) if re.search(r"\b(new|delete)\b", text.split("//")[0])]
    for bank in BANKS:
        GF, GP, GA, GR = _tools(bank)
        out = os.path.join(COV_DIR, bank)
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        with tempfile.TemporaryDirectory(prefix="hwcov_") as work:   # outside the repository
            if bank == "hw25":   # compiled where it lies, with the tools' two-line header for `struct mask`
                inc = os.path.join(work, "inc")
                os.makedirs(inc)
                with open(os.path.join(inc, "..\\aurora_etsi\\NoiseSupExports.h"), "w") as fh:
                    fh.write(GP.HEADER)
                unit, incs = src, ["-I", inc, "-I", os.path.join(ref_root, GP.REL)]
            else:                # copied unmodified, so that its #include does not find the 8 kHz header beside the original
                shutil.copy(src, os.path.join(work, "HuWang.cpp"))
                unit, incs = "HuWang.cpp", ["-I", inc64]
            subprocess.check_call(["g++", *COVFLAGS, *incs, "-c", unit, "-o", "HuWang.o"], cwd=work)
            subprocess.check_call(["g++", "--coverage", "-shared", "HuWang.o", "-o", "libhuwang.so"], cwd=work)
            for name, mod in zip(DRIVERS, (GF, GP, GA, GR)):
                with open(os.path.join(work, name + ".cpp"), "w") as fh:
                    fh.write(mod.DRIVER)
                subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-w", *incs, "-c", name + ".cpp", "-o", name + ".o"],
                                      cwd=work)
                subprocess.check_call(["g++", "-rdynamic", name + ".o", "-L", work, "-lhuwang", "-ldl", "-Wl,-rpath,$ORIGIN", "-o", name],
                                      cwd=work)
                shutil.copy(os.path.join(work, name), out)
            shutil.copy(os.path.join(work, "libhuwang.so"), out)
            shutil.copy(os.path.join(work, "HuWang.gcno"), out)
        with open(os.path.join(out, "lines.json"), "w") as fh:
            json.dump({"alloc": alloc}, fh)
        print(f"hwcov: built {out}")


# ---- a measurement ----------------------------------------------------------------------------------------------------
class CoverageRun:
    """The instrumented builds with their counters in a temporary directory, one sub-directory per bank.  run() adds a set's
    executions to the counters (they accumulate over runs, as gcov's do); reset() zeroes them; branches() reads them."""

    def __init__(self, banks=BANKS):
        for tool in ("g++", "gcov"):
            if shutil.which(tool) is None:
                raise RuntimeError(f"{tool} not found: the coverage measurement needs g++ and gcov")
        self.banks = tuple(banks)
        for bank in self.banks:
            for f in ("libhuwang.so", "HuWang.gcno", "lines.json") + DRIVERS:
                if not os.path.exists(os.path.join(COV_DIR, bank, f)):
                    raise FileNotFoundError(f"{os.path.join(COV_DIR, bank, f)} is missing: build it with `make -C oracle hwcov` "
                                            "where the reference's sources are")
        self.dir = tempfile.mkdtemp(prefix="hw_oracle_cov_")
        for bank in self.banks:
            os.makedirs(os.path.join(self.dir, bank))
            shutil.copy(os.path.join(COV_DIR, bank, "HuWang.gcno"), os.path.join(self.dir, bank))

    @contextlib.contextmanager
    def _counting(self, bank):
        """GCOV_PREFIX_STRIP larger than any path's depth leaves the bare file name under GCOV_PREFIX"""
        old = {k: os.environ.get(k) for k in ("GCOV_PREFIX", "GCOV_PREFIX_STRIP")}
        os.environ.update(GCOV_PREFIX=os.path.join(self.dir, bank), GCOV_PREFIX_STRIP="99")
        try:
            yield
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    def run(self, name, only=None):
        for bank in self.banks:
            exes = {d: os.path.join(COV_DIR, bank, d) for d in DRIVERS}
            tmp = os.path.join(self.dir, bank, "io")
            os.makedirs(tmp, exist_ok=True)
            with self._counting(bank):
                if name in ("hw-tests", "both"):
                    feed(bank, exes, tmp, hw_tests_inputs(bank))
                if name in ("edge", "both"):
                    feed(bank, exes, tmp, edge_inputs(bank, only))

    def reset(self):
        for f in glob.glob(os.path.join(self.dir, "*", "*.gcda")):
            os.remove(f)

    def branches(self):
        """{bank: [Branch, ...]} from `gcov -b -c --json-format` (a line that never ran counts as untaken).  The JSON form
        names lines, functions and branches from the notes file alone, so it reads the same where the reference is absent."""
        res = {}
        for bank in self.banks:
            cwd = os.path.join(self.dir, bank)
            if not os.path.exists(os.path.join(cwd, "HuWang.gcda")):
                raise RuntimeError(f"{bank}: no counters were written")
            subprocess.check_call(["gcov", "-b", "-c", "--json-format", "HuWang.gcda"], cwd=cwd, stdout=subprocess.DEVNULL,
                                  stderr=subprocess.DEVNULL)
            with gzip.open(os.path.join(cwd, "HuWang.gcov.json.gz"), "rt") as fh:
                doc = json.load(fh)
            with open(os.path.join(COV_DIR, bank, "lines.json")) as fh:
                alloc = set(json.load(fh)["alloc"])
            out = []
            for entry in doc["files"]:
                if os.path.basename(entry["file"]) != "HuWang.cpp":
                    continue
                names = {f["name"]: f.get("demangled_name", f["name"]).split("(")[0] for f in entry["functions"]}
                for line in entry["lines"]:
                    n = int(line["line_number"])
                    if n in alloc:
                        continue
                    kept = [br for br in line["branches"] if not br.get("throw")]
                    out += [Branch(bank, names.get(line.get("function_name"), line.get("function_name")), n, i, int(br["count"]))
                            for i, br in enumerate(kept)]
            if not out:
                raise RuntimeError(f"gcov reports no branch of HuWang.cpp at {bank}")
            res[bank] = out
        return res

    def lines(self):
        """{bank: {line of HuWang.cpp: times executed}} for the executable lines, from the same counters"""
        res = {}
        for bank in self.banks:
            cwd = os.path.join(self.dir, bank)
            subprocess.check_call(["gcov", "--json-format", "HuWang.gcda"], cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            with gzip.open(os.path.join(cwd, "HuWang.gcov.json.gz"), "rt") as fh:
                doc = json.load(fh)
            res[bank] = {int(line["line_number"]): int(line["count"]) for entry in doc["files"]
                         if os.path.basename(entry["file"]) == "HuWang.cpp" for line in entry["lines"]}
        return res

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def untaken(branches):
    return [b for b in branches if b.taken == 0]


def share(branches):
    return (sum(b.taken > 0 for b in branches), len(branches))


def measure(sets=SETS, banks=BANKS):
    """{set name: {bank: [Branch]}} for the given sets; `both` is hw-tests followed by edge"""
    res = {}
    with CoverageRun(banks) as cr:
        if "hw-tests" in sets or "both" in sets:
            cr.run("hw-tests")
            if "hw-tests" in sets:
                res["hw-tests"] = cr.branches()
        if "both" in sets:
            cr.run("edge")
            res["both"] = cr.branches()
        if "edge" in sets:
            cr.reset()
            cr.run("edge")
            res["edge"] = cr.branches()
    return res


def front_lines_missed(bank, audio, first, last):
    """(executable lines, those never executed) of HuWang.cpp:first-last when the front driver alone runs the given signals on
    the instrumented build: the line assertion of tools/gen_hw25_golden.py and gen_hw64_golden.py"""
    with CoverageRun((bank,)) as cr:
        tmp = os.path.join(cr.dir, bank, "io")
        os.makedirs(tmp)
        with cr._counting(bank):
            for x in audio:
                _tools(bank)[0].run(os.path.join(COV_DIR, bank, "front"), tmp, x)
        counts = {n: c for n, c in cr.lines()[bank].items() if first <= n <= last}
    return len(counts), sorted(n for n, c in counts.items() if c == 0)


# ---- the input sets ---------------------------------------------------------------------------------------------------
# an input set is a dict: audio {name: x}: one call of createIBM each (the AM driver), which runs the front half, initGroup,
# pitchDtm, computeAM and finalSeg, so the front and the pitch driver would add nothing on the same samples (the front driver
# runs once, on the first input); pitch_hand {name: (acf, pratio, mark, cross)}: through the pitch driver, step by step and
# through pitchDtm itself; final {name: dict}: straight into finalSeg; resynth {name: (x, mask)}; constants: the AM driver's
# constants run
def hw_tests_inputs(bank):
    """every input of the bank's four gen_hw* tools and of its GPU tests (tests/test_gpu_<bank>*.py) that the reference can be
    given: the tools' audio and hand-made arrays, the front-half batch of seven, the short model-judged inputs of the pitch
    and AM modules' audio batches (extra_inputs()) and, at 25 bands, the signal of tests/test_gpu_hw25_single.py at its
    lengths.  Left out, because the reference cannot take them: arrays made up for one stage that has no entry of its own in
    the reference (the zero streams handed to the correlogram, gOut and pitch handed to the AM stage); more than 400
    segments in finalSeg and utterances past MAX_SIG_LENGTH (they overrun its arrays); samples that are not finite; the
    resynthesis modules' slices of p with random masks whose last rows are set (the reference writes past its weight array
    on them: the model judges them; their samples are p's, which is fed whole).  Inputs shorter than a frame take no outcome
    past the length test and are dropped; the 65 537-utterance batch is eight zeros and the fixture's (d)."""
    import importlib
    import numpy as np
    GF = _tools(bank)[0]
    M, PM, AM, RM = _models(bank)
    hop = PM.HOP if hasattr(PM, "HOP") else 80
    audio = {f"front_{k}": x for k, x in GF.inputs().items()}
    pa = PM.audio_inputs()
    audio.update({f"pitch_{k}": x for k, x in pa.items()})
    audio.update({f"am_{k}": x for k, x in AM.audio_inputs().items()})
    audio.update({f"resynth_{k}": RM.hand_input(k) for k in RM.HAND_INPUTS})
    T = importlib.import_module(f"tests.test_gpu_{bank}")
    audio.update({f"gpu_front_{u}": x for u, x in enumerate(T.seven_inputs()[0])})
    for stage in ("pitch", "am"):
        T = importlib.import_module(f"tests.test_gpu_{bank}_{stage}")
        audio.update({f"gpu_{stage}_{u}": x for u, x in enumerate(T.extra_inputs())})
    if bank == "hw25":
        from tests import test_gpu_hw25_single as S
        audio.update({f"gpu_single_{L}": S._signal()[:L] for L in S.LENGTHS})
    audio = {k: np.ascontiguousarray(x, dtype=np.float32) for k, x in audio.items() if len(x) >= hop}
    cross0 = (lambda a: a) if bank == "hw25" else (lambda a: tuple(a) + (np.zeros_like(a[1]),))
    hand = {k: cross0(PM.hand_inputs(k)) for k in PM.HAND_CASES}
    for extra in ("no_streak_case", "many_segments_case"):
        if hasattr(PM, extra):
            c = getattr(PM, extra)()
            if isinstance(c, (tuple, list)) and len(c) >= 3:
                c = tuple(c[:4]) if bank == "hw25" and len(c) >= 4 else tuple(c[:3]) + (np.zeros_like(c[1]),)
                hand[extra] = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in c)
    # AM.many_final_segments_case() is left out: more than 400 segments in finalSeg overrun the reference's own array
    final = {k: make() for k, make in AM.HAND_CASES.items()}
    return dict(audio=audio, pitch_hand=hand, final=final, resynth=RM.reference_cases(AM.load_golden()), constants=True)


def edge_inputs(bank, only=None):
    """the edge set: audio from tests/<bank>_model.edge_inputs(), hand-made arrays from the _pitch and _am siblings"""
    M, PM, AM, RM = _models(bank)
    import numpy as np
    audio = dict(M.edge_inputs())
    hand = {k: tuple(PM.hand_inputs(k)) for k in PM.EDGE_HAND_CASES}
    if bank == "hw64":
        hand = {k: tuple(a) + (np.zeros_like(a[1]),) for k, a in hand.items()}
    final = {k: make() for k, make in AM.EDGE_HAND_CASES.items()}
    if only:
        known = set(audio) | set(hand) | set(final)
        unknown = [k for k in only if k not in known]
        if unknown:
            raise SystemExit(f"no such {bank} edge input: {unknown}; there are {sorted(known)}")
        audio, hand, final = ({k: v for k, v in d.items() if k in only} for d in (audio, hand, final))
    return dict(audio=audio, pitch_hand=hand, final=final, resynth={}, constants=False)


def feed(bank, exes, tmp, inputs):
    """run an input set through the bank's four drivers.  The reference refuses some inputs (no segment, more than 400, a
    Develope that would read an unset mark): the part of the chain before the refusal has run and is counted.  The runs are
    independent processes whose counters libgcov merges under a file lock, so they go through a small thread pool, each with
    files of its own; the same samples are run once."""
    import concurrent.futures
    import hashlib
    import threading
    GF, GP, GA, GR = _tools(bank)

    def audio(x):
        def job(d):
            try:
                GA.run_audio(exes["am"], d, x)
            except SystemExit:      # the driver's refusal 3: no segment, or more than 400
                pass
        return job

    def hand(arrays):
        def job(d):
            if not isinstance(GP.run(exes["pitch"], d, arrays=arrays), int):
                GP.run(exes["pitch"], d, arrays=arrays, whole=True)
        return job

    seen, distinct = set(), []
    for x in inputs["audio"].values():
        key = hashlib.sha256(x.tobytes()).digest()
        if key not in seen:
            seen.add(key)
            distinct.append(x)
    jobs = [audio(x) for x in sorted(distinct, key=len, reverse=True)]
    if inputs.get("constants"):
        jobs.append(lambda d: GA.run_constants(exes["am"], d))
    if distinct:
        jobs.append(lambda d: GF.run(exes["front"], d, distinct[0]))
    jobs += [hand(arrays) for arrays in inputs["pitch_hand"].values()]
    jobs += [(lambda d, c=c: GA.run_hand(exes["am"], d, c)) for c in inputs["final"].values()]
    jobs += [(lambda d, k=k, x=x, m=m: GR.run(exes["resynth"], d, x, m, k[0])) for k, (x, m) in inputs["resynth"].items()]

    def run(job):
        d = os.path.join(tmp, threading.current_thread().name)
        os.makedirs(d, exist_ok=True)
        job(d)

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        for f in [pool.submit(run, job) for job in jobs]:
            f.result()


# ---- the report -------------------------------------------------------------------------------------------------------
def report(per_bank, out=sys.stdout):
    for bank, br in per_bank.items():
        for lo, hi in RANGES:
            part = [b for b in br if (lo, hi) == range_of(b.line)]
            t, n = share(part)
            out.write(f"{bank} HuWang.cpp:{lo}-{hi}: {t} of {n} outcomes taken, {n - t} untaken\n")
            by_fn = collections.OrderedDict()
            for b in part:
                by_fn.setdefault(b.function, []).append(b)
            for fn, lst in by_fn.items():
                miss = untaken(lst)
                out.write(f"  {fn}: {len(lst) - len(miss)} of {len(lst)}" +
                          ("; untaken " + ", ".join(f":{b.line} branch {b.index}" for b in miss) if miss else "") + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--set", choices=SETS, default="both")
    ap.add_argument("--bank", choices=BANKS, default=None)
    ap.add_argument("--only", default=None, help="(edge) comma-separated input names")
    ap.add_argument("--build", metavar="REFERENCE_TREE", default=None, help="build oracle/_ref/hwcov from the reference's sources")
    a = ap.parse_args()
    if a.build:
        build(a.build)
        return
    with CoverageRun((a.bank,) if a.bank else BANKS) as cr:
        cr.run(a.set, a.only.split(",") if a.only else None)
        report(cr.branches())


if __name__ == "__main__":
    main()
