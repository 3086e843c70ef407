"""tests/hw_edge.py -- TEST INFRASTRUCTURE ONLY: what the Hu-Wang GPU tests share for the edge set (the inputs that take the
outcomes of the reference's HuWang.cpp which no older input takes: tests/test_hw_edge_coverage_cpu.py) -- the two fixtures
tests/golden/hw25_edge_golden.npz and hw64_edge_golden.npz (tools/gen_hw25_edge_golden.py, gen_hw64_edge_golden.py) and a
comparison that counts the 32-bit words it compares and how many differ before it asserts that none does."""
import functools
import os
import zlib

import numpy as np

FRONT_LARGE = ("hOut", "hEv", "acf_hc", "acf_ev")
FRONT_SMALL = ("cross_hc", "cross_ev", "pitch", "pRatio", "mark")
AUDIO = ("edc", "ewhole")


@functools.lru_cache(maxsize=None)
def load(bank):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{bank}_edge_golden.npz")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def differing(got, want):
    """the number of 32-bit words of `got` that differ from `want` (float32 or int32, the same shape), NaNs compared by
    position as tests/hw25_model.same_bits does"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == 4 and want.dtype == got.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        return int((got != want).sum())
    gn, wn = np.isnan(got), np.isnan(want)
    return int(((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))).sum())


class Tally:
    """counts the words compared and those that differ; done() prints both and asserts that none differs"""

    def __init__(self, what):
        self.what, self.words, self.bad, self.where = what, 0, 0, []

    def add(self, got, want, name):
        d = differing(got, want)
        self.words += int(np.asarray(want).size)
        self.bad += d
        if d:
            self.where.append(f"{name} ({d})")

    def add_crc(self, got, crc, idx, samples, name):
        """a large float array against its CRC32 and the values kept beside it: every word is compared through the CRC; where
        that differs, the sampled values say how many of them do (at least one word does)"""
        got = np.ascontiguousarray(got, dtype=np.float32)
        self.words += got.size
        if (zlib.crc32(got.tobytes()) & 0xFFFFFFFF) != int(crc):
            d = max(1, differing(got.ravel()[idx], samples))
            self.bad += d
            self.where.append(f"{name} (CRC; {d} of the {len(idx)} sampled values)")

    def done(self):
        print(f"{self.what}: {self.words} words compared, {self.bad} differ")
        assert not self.bad, f"{self.what}: {self.bad} of {self.words} words differ: " + ", ".join(self.where)
        return self.words


def sample_at(size):
    """the flat indices of the values the fixture keeps beside a large array's CRC: the generating tool's own function"""
    from tools import gen_hw25_edge_golden
    return gen_hw25_edge_golden.sample_at(size)


@functools.lru_cache(maxsize=None)
def model_chain(bank, k):
    """The whole chain from the numpy models for an audio edge input of which the fixture holds the front half alone,
    because the reference finds no segment in it and the tools do not call createIBM then (edc at 25 bands): the fixture's
    names with _k, the patterns ampatt_k / am_k whole, and status_k, the three stages' status words together.  The front
    model's arrays are asserted equal to the fixture's front_* first, so the chain starts from the reference's values."""
    import importlib
    M, PM, AM, RM = (importlib.import_module(f"tests.{bank}_{name}") for name in ("model", "pitch_model", "am_model", "resynth_model"))
    e = load(bank)
    x, t = e[f"x_{k}"], M.tables()
    fr = M.frontend(x, t)
    for name in FRONT_SMALL:
        assert M.same_bits(np.asarray(fr[name]).astype(e[f"front_{name}_{k}"].dtype), e[f"front_{name}_{k}"]), name
    ps = (PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"]) if bank == "hw25" else
          PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"]))
    g = AM.gout(x, t)
    am = AM.am_stage(g, ps["pitch"])
    fin = AM.final_seg(ps["grp"], am["amcrn"], fr["cross_ev"], ps["pratio"])
    out = {f"x_{k}": x, f"pitch_{k}": ps["pitch"], f"grp_{k}": ps["grp"], f"pratio_{k}": ps["pratio"], f"cross_ev_{k}": fr["cross_ev"],
           f"status_{k}": int(ps["status"] | am["status"] | fin["status"]), f"out_{k}": RM.resynth(g, fin["mask"], 0.0, t)}
    out.update({f"{name}_{k}": am[name] for name in ("amcrn", "seng", "ratio", "ampatt", "am")})
    out.update({f"{name}_{k}": fin[name] for name in tuple(AM.FINAL_STAGES) + ("grp_final", "mask")})
    return out


def source(bank, k):
    """where audio edge input k's expected arrays past the front half come from: the fixture, or the models"""
    e = load(bank)
    return e if f"mask_{k}" in e else model_chain(bank, k)


def add_front(tally, got, e, k, what):
    """the nine arrays of one utterance's front half against the fixture's front_* of input k"""
    for name in FRONT_SMALL:
        want = e[f"front_{name}_{k}"]
        tally.add(np.ascontiguousarray(got[name]).astype(want.dtype, copy=False), want, f"{what} {name}")
    for name in FRONT_LARGE:
        a = np.ascontiguousarray(got[name])
        tally.add_crc(a, e[f"front_{name}_crc_{k}"], sample_at(a.size), e[f"front_{name}_s_{k}"], f"{what} {name}")


def pitch_want(e, k, pitch_stages, grp_stages):
    """the pitch stage's expected arrays of input or hand-made case k, as the pitch modules' _from_golden gives them"""
    want = {name: e[f"{name}_{k}"] for name in ("pitch", "pratio") + tuple(pitch_stages)}
    want.update({name: e[f"{name}_{k}"].astype(np.float32) for name in ("grp",) + tuple(grp_stages)})
    want["status"] = int(e[f"nseg_{k}"])
    return want


def add_pitch(tally, got, want, names, what):
    assert got["status"] == want["status"], f"{what}: status {got['status']:#x}, expected {want['status']:#x}"
    for name in names:
        w = np.asarray(want[name])
        tally.add(np.ascontiguousarray(got[name]).astype(w.dtype, copy=False), w, f"{what} {name}")
