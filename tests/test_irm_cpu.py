"""CPU tests of the IRM target (csrc/irm_kernel.hip, csrc/irm_rdft128.inc, oracle/resynth_oracle.c: ora_irm_target), no GPU.

What is shown here, so that tests/test_gpu_irm.py can hold the device to tests/irm_model.py within irm_cases.IRM_TOL:
  * the generated codelet is what tools/gen_rdft_codelet.py writes, and computes the 128-point DFT of 80 reals to a DERIVED bound
    (tests/irm_kernel_driver.cpp includes it as the kernel does; address and undefined-behaviour sanitizers on);
  * IRM_TOL is 4 .. 16 times the larger of the two errors a correct implementation makes against the float64 model: the
    restatement's (E_oracle) and a float32 restatement of the kernel's own arithmetic (E_kernel, the worse of two contraction forms);
  * every misreading of irm_model.MUTANTS moves the model by >= 4 IRM_TOL on a case of tests/irm_cases.py;
  * >= 90 % of every non-silent case lies in [0.05, 0.95], where the ratio is sensitive;
  * the inputs of test_irm_target_vs_oracle under the tolerance of before, 1e-4: what they could not see.

MEASURED (printed by the tests; -s shows them):
  codelet     unit impulses: worst |g - exp(-2 pi i n k / 128)| = 1.62e-7 (bound 6.74e-7);
              random int16-valued inputs: worst bin 2.51e-7 ||x|| (bound 5.01e-6 ||x||), all bins 8.61e-8 ||X|| (bound 1.30e-6 ||X||)
  E_oracle    4.22e-7     E_kernel plain 1.42e-7, contracted 1.42e-7     IRM_TOL 3.5e-6 = 8.3 x the larger
  mutants     window /320 5.2e-4; Hanning for Hamming 1.0e-2; rectangular 0.126; one sample late 4.3e-3; bin 63 left out 0.24;
              bin 64 included 6.5e-2; one bin 0.2 % 2.3e-4; component 3 left out 1.8e-2; slot 15 reads the next tile 0.14;
              noise sum of tile 1 from the pure stream 0.29; tile tail into the last row 5.7e-2   (each on the first case that sees it)
  present inputs (test_irm_target_vs_oracle's, Hamming), per utterance:
              one bin 0.2 %: 7.1e-5, 3.9e-5, 5.8e-5, 7.7e-5; bin 63 1 %: 2.0e-4, 1.1e-4, 7.2e-5, 2.7e-4;
              component 1 x 1.0005: 6.6e-5, 2.3e-5, 4.7e-5, 5.4e-5 -- under the 1e-4 of before, 7 to 20 times IRM_TOL
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import irm_cases as C
from tests import irm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
U = 2.0 ** -24                      # float32 unit roundoff (half an ulp of a value in [1, 2))
N_RANDOM = 6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/irm_kernel_driver.cpp"
    exe = str(tmp_path_factory.mktemp("irm_driver") / "irm_kernel_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "irm_kernel_driver.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and not run.stderr, f"driver (sanitizers on) exited with {run.returncode}:\n{run.stderr[-2000:]}"
    return run.stdout


@pytest.fixture(scope="module")
def case_list(oracle):
    return C.cases(oracle)


@pytest.fixture(scope="module")
def models(case_list):
    return [M.irm(p, n, kind) for _, p, n, kind, _ in case_list]


# ---- the codelet ---------------------------------------------------------------------------------------------------------------
def test_codelet_is_the_128_point_dft_of_80_reals(driver):
    """BOUNDS.  A value reaches an output through the radix-2 stages of sizes 2 .. 128; sizes 2 and 4 have exact twiddles (1, -i), so
    at most FIVE stages multiply it by a literal.  Such a stage's complex error, relative to the value it acts on, is at most
      sqrt(2) u / 2   the literal (each component rounded to float: half an ulp of a figure <= 1)
    + sqrt(2) u       the product (per component one product rounded, then the fused multiply-add rounded)
    + u               the butterfly's addition
    = (1.5 sqrt(2) + 1) u = 3.13 u,  u = 2^-24.
    Unit impulse: every value on its way has modulus 1 and the additions add an exact 0, so |g[k] - exp(-2 pi i n k / 128)| <=
    5 x 1.5 sqrt(2) u = 10.7 u to first order; the bound asserted is 8 sqrt(2) u (6.7e-7), which leaves the second-order terms room.
    General input: the stages are orthogonal up to their factor sqrt(2), so the errors add in the 2-norm over all 128 bins:
    ||G' - G|| <= 7 x 3.13 u ||G|| (seven stages, as if each had a literal), ||G|| = sqrt(128) ||x||.  Bins 65 .. 127 mirror bins
    63 .. 1, so the 64 bins the codelet gives must satisfy sqrt(|d0|^2 + 2 sum_{k=1..63} |d_k|^2) <= 22 u sqrt(128) ||x||: that
    is rigorous to first order.  A single bin: were the error spread evenly its modulus would be <= 22 u ||x||; the roundings of
    different butterflies do not conspire on one bin of 128, but a bin may well sit a few times above the mean, so the bound is
    c log2(128) u ||x|| with c = 4 x 3.13, rounded to 12: four times the even share of the worst-case total."""
    out = _run(driver, "codelet", 7, N_RANDOM).splitlines()
    assert len(out) == 2 * (80 + N_RANDOM)
    k, n = np.arange(64)[:, None], np.arange(80)[None, :]
    basis = np.exp(-2j * np.pi * n * k / 128.0)                     # [64][80]
    worst_imp = worst_bin = worst_norm = 0.0
    for t in range(80 + N_RANDOM):
        assert out[2 * t].startswith("in ") and out[2 * t + 1].startswith("out ")
        x = np.array(out[2 * t].split()[1:], np.float64)
        g = np.array(out[2 * t + 1].split()[1:], np.float64)
        assert x.size == 80 and g.size == 128
        g = g[0::2] + 1j * g[1::2]
        want = basis @ x
        d = np.abs(g - want)
        if t < 80:
            assert x[t] == 1.0 and np.count_nonzero(x) == 1
            worst_imp = max(worst_imp, float(d.max()))
        else:
            assert np.all(x == np.rint(x)) and np.abs(x).max() <= 32768 and np.count_nonzero(x) > 70
            nx = float(np.linalg.norm(x))
            worst_bin = max(worst_bin, float(d.max()) / nx)
            worst_norm = max(worst_norm, float(np.sqrt(d[0] ** 2 + 2.0 * (d[1:] ** 2).sum())) / (np.sqrt(128.0) * nx))
    imp_bound, bin_bound, norm_bound = 8 * np.sqrt(2.0) * U, 12 * 7 * U, 7 * (1.5 * np.sqrt(2.0) + 1.0) * U
    print(f"codelet: unit impulses worst |delta| {worst_imp:.3g} (bound {imp_bound:.3g}); random inputs worst bin "
          f"{worst_bin:.3g} ||x|| (bound {bin_bound:.3g}), all bins {worst_norm:.3g} ||X|| (bound {norm_bound:.3g})")
    assert worst_imp <= imp_bound
    assert worst_bin <= bin_bound
    assert worst_norm <= norm_bound


def test_generator_reproduces_the_committed_codelet():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rdft_codelet.py"), "128", "80", "64", "g"],
                         capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    with open(os.path.join(CSRC, "irm_rdft128.inc"), "rb") as f:
        committed = f.read()
    assert run.stdout == committed, "csrc/irm_rdft128.inc is not what tools/gen_rdft_codelet.py 128 80 64 g writes"
    assert committed.count(b"\n") == 1 + 1189 + 128                 # the header, the instructions, the outputs


# ---- the case list ---------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_kernel_edges(case_list):
    names = [c[0] for c in case_list]
    assert len(set(names)) == len(names)
    for kind in (0, 1, 2):
        got = {(p.shape[1], k) for _, p, _, k, fam in case_list if fam == "tones"}
        assert {(C.length(F, t), kind) for F in C.FRAMES for t in C.TAILS} <= got
    Ls = {p.shape[1] for _, p, _, _, _ in case_list}
    assert {L % 8 == 0 for L in Ls} == {True, False} and 811 in Ls
    assert {M.n_frames(L) for L in Ls} >= {1, 15, 16, 17, 65}
    sq = dict((c[0], c) for c in case_list)["square waves w=1"]
    assert sq[1].min() == -32768 and sq[1].max() == 32767 and sq[2].min() == -32768 and sq[2].max() == 32767
    imp = dict((c[0], c) for c in case_list)["one sample per frame w=1"]
    for x in (imp[1], imp[2]):
        for f in range(M.n_frames(x.shape[1])):
            assert np.all(np.count_nonzero(x[:, 160 * f:160 * f + 320], axis=1) == 1)


def test_cases_sit_where_the_ratio_is_sensitive(case_list, models):
    """In every case but the silent ones >= 90 % of the compared values lie in [0.05, 0.95]; the cases built for an exact value
    give it exactly, in the model as on the device."""
    for (name, _, _, _, fam), r in zip(case_list, models):
        for sl, v in C.exact_values(name):
            assert np.all(np.isnan(r[:, sl])) if v is None else np.all(r[:, sl] == v), name
        if fam == C.SILENT:
            continue
        assert not np.isnan(r).any(), name
        share = float(np.mean((r >= 0.05) & (r <= 0.95)))
        print(f"{name}: {100 * share:.1f} % in [0.05, 0.95], range {r.min():.3f} .. {r.max():.3f}")
        assert share >= 0.9, name
    tones = dict((c[0], r) for c, r in zip(case_list, models))["tones F=17 tail=5 w=1"]
    assert 0.2 <= tones.min() and tones.max() <= 0.8


# ---- the errors of correct implementations, and the tolerance -----------------------------------------------------------------
def _max_delta(got, want, what):
    ok = ~np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), ~ok), f"{what}: shape or NaN positions"
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0


@pytest.fixture(scope="module")
def errors(driver, oracle, case_list, models, tmp_path_factory):
    e_oracle = max(_max_delta(oracle.irm_target(p, n, kind).astype(np.float64), m, name)
                   for (name, p, n, kind, _), m in zip(case_list, models))
    path = str(tmp_path_factory.mktemp("irm_frames") / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(case_list)).tobytes())
        for _, p, n, kind, _ in case_list:
            f.write(np.array([kind, p.shape[1]], np.int32).tobytes())
            f.write(np.ascontiguousarray(p).tobytes())
            f.write(np.ascontiguousarray(n).tobytes())
    e_form = []
    for form in (0, 1):
        lines = _run(driver, "frames", path, form).splitlines()
        pos, worst = 0, 0.0
        for i, ((name, _, _, _, _), m) in enumerate(zip(case_list, models)):
            head = lines[pos].split()
            assert head[0] == "case" and int(head[1]) == i and int(head[2]) == m.shape[0], name
            got = np.array([ln.split() for ln in lines[pos + 1:pos + 1 + m.shape[0]]], np.float64).reshape(m.shape[0], 64)
            got = got.astype(np.float32).astype(np.float64)      # nine digits name the float
            for sl, v in C.exact_values(name):      # the float form gives the exact values exactly too
                assert np.all(np.isnan(got[:, sl])) if v is None else np.all(got[:, sl] == v), name
            worst = max(worst, _max_delta(got, m, f"{name}, form {form}"))
            pos += 1 + m.shape[0]
        assert pos == len(lines)
        e_form.append(worst)
    return e_oracle, e_form


def test_tolerance_is_derived_from_the_measured_errors(errors):
    e_oracle, e_form = errors
    e_kernel = max(e_form)
    e = max(e_oracle, e_kernel)
    print(f"E_oracle {e_oracle:.3g}   E_kernel {e_kernel:.3g} (plain {e_form[0]:.3g}, contracted {e_form[1]:.3g})   "
          f"IRM_TOL {C.IRM_TOL:.3g} = {C.IRM_TOL / e:.2f} x the larger")
    assert 4 * e <= C.IRM_TOL <= 16 * e


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_seen_by_a_case(case_list, models):
    """Each misreading moves the model by >= 4 IRM_TOL on at least one case: the first case of the list that sees it is printed."""
    unseen = []
    for mutant, kw in M.MUTANTS.items():
        best = (0.0, None)
        for (name, p, n, kind, fam), m in zip(case_list, models):
            if fam == C.SILENT:
                continue
            r = M.irm(p, n, kind, **kw)
            ok = ~(np.isnan(m) | np.isnan(r))
            d = float(np.abs(r[ok] - m[ok]).max()) if ok.any() else 0.0
            if d > best[0] or best[1] is None:
                best = (d, name)
            if d >= 4 * C.IRM_TOL:
                break
        print(f"mutant '{mutant}': {best[0]:.3g} on '{best[1]}' (needs >= {4 * C.IRM_TOL:.3g})")
        if best[0] < 4 * C.IRM_TOL:
            unseen.append(mutant)
    assert not unseen, unseen
    # a tile's slot 15 in the MIDDLE of an utterance: steady tones cannot tell a frame from the next one, the ramped ones do
    name = "ramped tones F=65 tail=159 w=1"
    (_, p, n, kind, _), m = next((c, m) for c, m in zip(case_list, models) if c[0] == name)
    d = np.abs(M.irm(p, n, kind, slot15_reads_next_tile=True) - m)
    slot15 = np.arange(65) % 16 == 15
    print(f"mutant 'slot 15 reads the next tile' on '{name}', rows 15, 31, 47: {d[slot15][:3].max(axis=1)}")
    assert np.all(d[~slot15] == 0.0) and np.all(d[slot15][:3].max(axis=1) >= 4 * C.IRM_TOL)


def test_present_inputs_and_their_blind_spots(oracle):
    """The record of why tests/irm_cases.py exists: on the inputs of test_gpu_parity.py::test_irm_target_vs_oracle the small errors
    below stay under the 1e-4 those tests allowed -- a wrong fourth digit in the generated transform would have shipped."""
    from speech_enhancement_amd import corpus
    lens = [4800, 320, 320 + 160 * 3 + 11, 160 * 150 + 5]
    pairs = []
    for i, L in enumerate(lens):
        clean = corpus.synth_utterance(120 + i, L)
        noise = (corpus.synth_utterance(140 + i, L).astype(np.int32) // 3).astype(np.int16)
        pairs.append((oracle.subband64(clean), oracle.subband64(noise)))
    base = [M.irm(p, n, 1) for p, n in pairs]
    e = max(_max_delta(oracle.irm_target(p, n, 1).astype(np.float64), b, f"L={p.shape[1]}") for (p, n), b in zip(pairs, base))
    print(f"ora_irm_target vs the model on the present inputs: {e:.3g}")
    assert e <= C.IRM_TOL

    def deviations(kw):
        out = []
        for (p, n), b in zip(pairs, base):
            r = M.irm(p, n, 1, **kw)
            ok = ~(np.isnan(b) | np.isnan(r))
            out.append(float(np.abs(r[ok] - b[ok]).max()))
        return out
    for mutant, kw in list(M.SMALL_MUTANTS.items()) + [(k, v) for k, v in M.MUTANTS.items() if k not in M.SMALL_MUTANTS]:
        d = deviations(kw)
        print(f"present inputs, '{mutant}': " + ", ".join(f"{v:.2g}" for v in d) + f"   (old tolerance 1e-4, IRM_TOL {C.IRM_TOL:.2g})")
        if mutant in M.SMALL_MUTANTS:
            assert min(d) < 1e-4, mutant                     # at least one input lets it pass at 1e-4 ...
            assert max(d) >= 4 * C.IRM_TOL, mutant           # ... which IRM_TOL does not
    for mutant in ("one bin's power off by 0.2 %", "polyphase component 1 scaled by 1.0005"):
        assert max(deviations(M.SMALL_MUTANTS[mutant])) < 1e-4, mutant      # no input at all sees these at 1e-4
