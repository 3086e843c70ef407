#!/usr/bin/env python3
"""tools/gen_hw25_edge_golden.py -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hw25_edge_golden.npz: what THE REFERENCE ITSELF makes of the edge inputs (tests/hw25_model.EDGE_INPUTS,
tests/hw25_pitch_model.EDGE_HAND_CASES, tests/hw25_am_model.EDGE_HAND_CASES: the inputs that take the outcomes of HuWang.cpp
which no older input takes, tests/test_hw_edge_coverage_cpu.py) at every stage: data only, no reference source.  Runs only
where the reference tree exists:

    python tools/gen_hw25_edge_golden.py <reference tree>

It builds nothing of its own: the four drivers of tools/gen_hw25_golden.py, gen_hw25_pitch_golden.py, gen_hw25_am_golden.py
and gen_hw25_resynth_golden.py are built by those tools' build () and read by their readers.  tools/gen_hw64_edge_golden.py is
this file at the 64-band tools and models.

Per audio input k: x_k; the front half under front_NAME_k (cross_hc, cross_ev, pRatio, mark, pitch whole; hOut, hEv, acf_hc,
acf_ev as front_NAME_crc_k, the CRC32 of the float32 bytes, and front_NAME_s_k, the values at sample_at (size)).  Where
createIBM takes the input (edc has no segment: the reference's arrays end with the front half): the pitch fixture's arrays
(nseg, lrframe, the pitch and grp stages, pitch, grp, pratio), the AM fixture's (cross_ev, seng, ratio, amcrn, the stages of
finalSeg, grp_final, mask, and gout / ampatt / am as CRCs per channel plus samples) and out_k, resynthesis of createIBM's mask.
Per hand-made pitch case: the pitch fixture's arrays; per hand-made finalSeg case: the stages, grp_final, mask.

Asserted before anything is written: the instrumented build of oracle/_ref/hwcov gives the same bytes as the plain one;
pitchDtm itself equals its steps; the numpy models equal the reference on every array, up to sEng; no unit's ratio lies within
the AM fixture's ratio_tol (relative) of THETAE, and the model's ratio lies within it of the reference's; the file stays under
1 MiB.  ratio_tol is copied from the AM fixture so that the tests read it beside the arrays it bounds.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import hw_oracle_coverage as C  # noqa: E402

LARGE = ("hOut", "hEv", "acf_hc", "acf_ev")
SMALL = ("cross_hc", "cross_ev", "pRatio", "mark", "pitch")
SAMPLES = 256


def path_of(bank):
    return os.path.join(ROOT, "tests", "golden", f"{bank}_edge_golden.npz")


def sample_at(size):
    """the flat indices of the values kept beside a large array's CRC"""
    return np.linspace(0, size - 1, min(SAMPLES, size)).astype(np.int64)


def same(a, b):
    return all(np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in a)


def main(bank="hw25"):
    if len(sys.argv) != 2:
        raise SystemExit(f"usage: python tools/gen_{bank}_edge_golden.py <reference tree>")
    ref_root = sys.argv[1]
    GF, GP, GA, GR = C._tools(bank)
    M, PM, AM, RM = C._models(bank)
    if bank == "hw25":
        builds = (lambda t: GF.build(ref_root, t), lambda t: GP.build(ref_root, t, "plain", []),
                  lambda t: GA.build(ref_root, t, "plain", []), lambda t: GR.build(ref_root, t, "plain", []))
    else:
        from tools import gen_hw64_am_golden, gen_hw64_golden, gen_hw64_pitch_golden, gen_hw64_resynth_golden
        builds = (lambda t: gen_hw64_golden.build(ref_root, t), lambda t: gen_hw64_pitch_golden.build(ref_root, t, "plain", []),
                  lambda t: gen_hw64_am_golden.build(ref_root, t, "plain", []),
                  lambda t: gen_hw64_resynth_golden.build(ref_root, t, "plain", []))
    cov = {d: os.path.join(C.COV_DIR, bank, d) for d in C.DRIVERS}
    assert all(os.path.exists(p) for p in cov.values()), "build oracle/_ref/hwcov first (make -C oracle hwcov)"
    am_gold = AM.load_golden()
    tol = float(am_gold["ratio_tol"])
    data = {"ratio_tol": np.float64(tol)}
    t = M.tables()
    edge = C.edge_inputs(bank)
    with tempfile.TemporaryDirectory() as tmp:
        exe = {}
        for d, b in zip(C.DRIVERS, builds):
            os.makedirs(os.path.join(tmp, d))
            exe[d] = b(os.path.join(tmp, d))
        io = os.path.join(tmp, "io")
        os.makedirs(io)
        for k, x in edge["audio"].items():
            L, nfr = len(x), len(x) // PM.HOP
            data[f"x_{k}"] = x
            fr = GF.run(exe["front"], io, x)
            assert same(fr, GF.run(cov["front"], io, x)), f"{k}: the coverage build differs in the front half"
            model = M.frontend(x, t)
            for name in LARGE + SMALL:
                assert M.same_bits(model[name], fr[name]), f"{k}: the model's {name} differs from the reference's"
                if name in LARGE:
                    data[f"front_{name}_crc_{k}"] = np.uint32(PM.crc32(fr[name]))
                    data[f"front_{name}_s_{k}"] = fr[name].ravel()[sample_at(fr[name].size)]
                else:
                    data[f"front_{name}_{k}"] = fr[name]
            zero_rows = int(((fr["acf_hc"] == 0).all(axis=2)).sum())
            print(f"input {k}: L {L}, frames {nfr}, marks {int(fr['mark'].sum())}, units whose ACF is all zero {zero_rows}, "
                  f"NaN pRatio {int(np.isnan(fr['pRatio']).sum())}")
            r = GP.run(exe["pitch"], io, x=x)
            if isinstance(r, int):
                assert r == 3 and GP.run(cov["pitch"], io, x=x) == 3, f"{k}: refused with {r}"
                assert M.frontend(x, t)["mark"].sum() == 0 or PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"])["status"] == 0
                print(f"input {k}: no segment, createIBM is not called")
                continue
            GP.both(exe["pitch"], cov["pitch"], io, r, x=x)
            assert int(r.pop("acfcrc")) == PM.crc32(fr["acf_hc"])
            pm = (PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"]) if bank == "hw25" else
                  PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"]))
            assert pm["status"] == int(r["nseg"])
            for name in ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES:
                assert M.same_bits(np.asarray(pm[name]).astype(np.float32), np.asarray(r[name]).astype(np.float32)), f"{k}: the model's {name}"
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            a = GA.run_audio(exe["am"], io, x)
            assert same(a, GA.run_audio(cov["am"], io, x)), f"{k}: the coverage build differs in createIBM"
            for name in ("pitch", "grp", "pratio"):
                assert np.asarray(a[name]).tobytes() == np.asarray(r[name]).tobytes(), f"{k}: createIBM's {name} is not pitchDtm's"
            g = AM.gout(x, t)
            assert M.same_bits(g, a["gout"])
            m = AM.am_stage(g, a["pitch"])
            for name in ("ampatt", "am", "seng"):
                assert M.same_bits(m[name], a[name]), f"{k}: the model's {name} differs from the reference's"
            run = a["ratio"] != 0
            rel = np.abs(m["ratio"][run].astype(np.float64) - a["ratio"][run]) / a["ratio"][run]
            band = int((np.abs(a["ratio"][run].astype(np.float64) - AM.THETAE) <= tol * AM.THETAE).sum())
            assert rel.max() <= tol, f"{k}: the model's ratio differs by {rel.max():.3g}, more than the fixture's ratio_tol {tol:.3g}"
            assert band == 0, f"{k}: a unit lies within ratio_tol of THETAE: change the input"
            assert np.array_equal(m["amcrn"], a["amcrn"].astype(np.float32))
            f = AM.final_seg(a["grp"], a["amcrn"], a["cross_ev"], a["pratio"])
            for name in AM.FINAL_STAGES + ("grp_final", "mask"):
                assert np.array_equal(f[name], a[name].astype(np.float32)), f"{k}: the model's {name} differs"
                data[f"{name}_{k}"] = a[name]
            for name in ("cross_ev", "seng", "ratio", "amcrn"):
                data[f"{name}_{k}"] = a[name]
            idx = AM.sample_index(L)
            for name in ("gout", "ampatt", "am"):
                data[f"{name}_crc_{k}"] = AM.channel_crcs(a[name])
                data[f"{name}_s_{k}"] = a[name].ravel()[idx]
            mask = a["mask"].astype(np.float32)
            seen, out, _ = GR.run(exe["resynth"], io, x, mask, "a")
            seen_c, out_c, _ = GR.run(cov["resynth"], io, x, mask, "a")
            assert out.tobytes() == out_c.tobytes() and np.array_equal(seen, mask) and np.array_equal(seen_c, mask)
            assert M.same_bits(RM.resynth(g, mask, 0.0, t), out), f"{k}: the resynthesis model differs from the reference"
            data[f"out_{k}"] = out
            print(f"input {k}: segments {int(r['nseg'])}, voiced {int((a['pitch'] > 0).sum())}, sinModel units {int(run.sum())}, AM labels "
                  f"{int(a['amcrn'].sum())}, mask units {int(a['mask'].sum())}, -1 units {int((a['grp_final'] < 0).sum())}, model ratio rel. "
                  f"diff {float(rel.max()):.3g} (ratio_tol {tol:.3g}), nearest to THETAE {np.abs(a['ratio'][run] - AM.THETAE).min():.3g}, "
                  f"largest |enhanced| {float(np.abs(out).max()):.6g}")
        for k, arrays in edge["pitch_hand"].items():
            r = GP.run(exe["pitch"], io, arrays=arrays)
            assert not isinstance(r, int), f"hand-made {k}: the driver refused it ({r})"
            GP.both(exe["pitch"], cov["pitch"], io, r, arrays=arrays)
            r.pop("acfcrc")
            pm = PM.pitch_stage(*arrays) if bank == "hw25" else PM.pitch_stage(*arrays[:3])
            assert pm["status"] == int(r["nseg"])
            for name in ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES:
                assert M.same_bits(np.asarray(pm[name]).astype(np.float32), np.asarray(r[name]).astype(np.float32)), f"hand-made {k}: the model's {name}"
            for name, v in r.items():
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: segments {int(r['nseg'])}, lFrame / rFrame {r['lrframe'].tolist()}, pitch {r['pitch'].tolist()}")
        for k, c in edge["final"].items():
            r = GA.run_hand(exe["am"], io, c)
            rc = GA.run_hand(cov["am"], io, c)
            assert all(np.array_equal(rc[n], r[n]) for n in r)
            f = AM.final_seg(**c)
            for name, v in r.items():
                assert np.array_equal(f[name], v.astype(np.float32)), f"hand-made {k}: the model's {name} differs"
                data[f"{name}_{k}"] = v
            print(f"hand-made {k}: mask units {int(r['mask'].sum())}, -1 units {int((r['grp_final'] < 0).sum())}")
    from tools import gen_hw25_pitch_golden
    gen_hw25_pitch_golden.save(path_of(bank), data)
    assert os.path.getsize(path_of(bank)) < 1 << 20, "the fixture must stay under 1 MiB"
    print(f"wrote {path_of(bank)}: {os.path.getsize(path_of(bank))} bytes")


if __name__ == "__main__":
    main()
