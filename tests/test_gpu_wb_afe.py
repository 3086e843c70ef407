"""GPU tests of the wideband (16 kHz) feature chain (sea_wb_denoise_batch_fd + sea_wb_afe_features_batch, Python:
wb_afe_features_batch): NoiseSup with speech flags -> WaveProc -> the 26-band CompCeps -> PostProc -> frame-dropping VAD ->
flush, against the reference's own functions called in the order of its commented-out chain (tests/wb_afe_reference.py) and
against their recorded outputs (tests/golden/wb_afe_golden.npz, tools/gen_wb_afe_golden.py).

Tolerances are those of tests/test_gpu_wb.py: floats |delta| <= 1e-4 max(1, |ref|); cepstral and feature values |delta| <=
1e-3; zero tolerance on n_feat, n_ceps, every VAD flag, every flag byte and on which emitted frames are null vectors.  The
expectation is bit-identical; every test prints what it measured.  Run on an MI355X with ``pytest -m gpu``."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wb_afe_golden.npz")
N_FIXTURE = 7


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _reference():
    from tests import wb_afe_reference as A
    if not A.available():
        pytest.fail("oracle/_ref/libetsi_ref.so is missing: `make -C oracle ref` builds it where the reference's sources "
                    "are; this test needs the built library beside the tree")
    return A


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(utts, use_order=True, keep_raw=False):
    """The whole chain on a batch -> per utterance dicts of numpy arrays (and, keep_raw, the batch and the raw result)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device="cuda:0")
    r = sea.wb_afe_features_batch(b, want_intermediates=True, use_order=use_order)
    torch.cuda.synchronize()
    out, f32 = sea.wb_split(b, r["out"]), sea.wb_split(b, r["f32"])
    flags, hpr, code = (sea.wb_rows(b, r[k]) for k in ("flag_rows", "hp_rows", "code_rows"))
    first, onset, n_ceps = (r[k].cpu().numpy() for k in ("first_out", "onset", "n_ceps"))
    cc, pp, cum = r["feat_cc"].cpu().numpy(), r["feat_pp"].cpu().numpy(), r["ceps_cum"]
    res = []
    for u, x in enumerate(utts):
        nfr, nc = len(x) // 160, int(n_ceps[u])
        res.append(dict(feats=r["feats"][u], n_ceps=nc, feat_cc=cc[cum[u]:cum[u] + nc], feat_pp=pp[cum[u]:cum[u] + nc],
                        cc_cap=cc[cum[u]:cum[u + 1]], flags=flags[u], out=out[u], f32=f32[u].reshape(nfr, 80), hp=hpr[u],
                        code=code[u], first_out=int(first[u]), onset=int(onset[u])))
    return (res, b, r) if keep_raw else res


@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _fixture_run():
    """the fixture batch through the chain, once for the tests that need it (nothing modifies it)"""
    g = _fixture()
    return _run([g[f"x{u}"] for u in range(N_FIXTURE)], keep_raw=True)


class _Stats:
    def __init__(self):
        self.f = {}
        self.exact = {}

    def flt(self, key, got, want):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        m, n, nb = self.f.get(key, (0.0, 0, 0))
        self.f[key] = (max(m, float(d.max()) if d.size else 0.0), n + d.size, nb + int((_u32(got) != _u32(want)).sum()))

    def same(self, key, n):
        self.exact[key] = self.exact.get(key, 0) + int(n)

    def report(self, title):
        print(f"\n{title}:")
        for k, (m, n, nb) in self.f.items():
            print(f"  {k}: max |delta| {m:.3g} (tolerance 1e-3), {nb} of {n} values differ in bits")
        for k, n in self.exact.items():
            print(f"  {k}: {n} compared, all exact")

    def check(self):
        for k, (m, n, nb) in self.f.items():
            assert m <= 1e-3, f"{k}: max |delta| {m}"
            assert nb == 0, f"{k}: {nb} of {n} values differ in bits"


def _compare(st, got, want, nfr, what):
    """got: one entry of _run; want: feat_cc, feat_pp, feat15, flags (per output frame), first_out, onset"""
    assert got["first_out"] == want["first_out"], f"{what}: first_out {got['first_out']} != {want['first_out']}"
    assert got["onset"] == want["onset"], f"{what}: onset {got['onset']} != {want['onset']}"
    fo = want["first_out"]
    nout = nfr - fo if fo >= 0 else 0
    assert len(want["flags"]) == nout
    assert got["n_ceps"] == len(want["feat_cc"]) == max(nout - 2, 0), f"{what}: {got['n_ceps']} cepstral frames, reference {len(want['feat_cc'])}"
    assert len(got["feats"]) == len(want["feat15"]), f"{what}: {len(got['feats'])} emitted frames, reference {len(want['feat15'])}"
    assert not got["cc_cap"][got["n_ceps"]:].any(), f"{what}: rows behind the last cepstral frame were written"
    quiet = fo if fo >= 0 else nfr
    assert not got["flags"][:quiet].any(), f"{what}: flag rows of frames without an output were written"
    assert np.array_equal(got["flags"][quiet:], want["flags"]), \
        f"{what}: flag bytes differ at output frames {np.flatnonzero(got['flags'][quiet:] != want['flags'])[:8]}"
    st.same("flag bytes", nout)
    g15, w15 = got["feats"], want["feat15"]
    assert np.array_equal(g15[:, 14], w15[:, 14]), f"{what}: VAD flags differ at emitted frames {np.flatnonzero(g15[:, 14] != w15[:, 14])[:8]}"
    st.same("VAD flags", len(w15))
    assert np.array_equal(~g15.any(axis=1), ~w15.any(axis=1)), f"{what}: the null vectors are not the reference's"
    st.same("null-vector positions", len(w15))
    st.flt("feat_cc", got["feat_cc"], want["feat_cc"])
    st.flt("feat_pp", got["feat_pp"], want["feat_pp"])
    st.flt("feats", g15[:, :14], w15[:, :14])


def test_a_fixture_batch():
    """(a) all seven fixture utterances in one call against the stored reference outputs; everything the call shares with
    wb_denoise_batch is that call's, bit for bit: recording flags changes nothing else"""
    import speech_enhancement_amd as sea
    torch = _torch()
    g = _fixture()
    res, b, raw = _fixture_run()
    st = _Stats()
    for u in range(N_FIXTURE):
        want = dict(feat_cc=g[f"feat_cc{u}"], feat_pp=g[f"feat_pp{u}"], feat15=g[f"feat15_{u}"], flags=g[f"flags{u}"],
                    first_out=int(g["first_out"][u]), onset=int(g["onset"][u]))
        _compare(st, res[u], want, len(g[f"x{u}"]) // 160, f"fixture utterance {u}")
        nemit, nflag1 = int(g["counts"][u][2]), int(g["counts"][u][4])
        assert len(res[u]["feats"]) == nemit and int((res[u]["feats"][:, 14] == 1).sum()) == nflag1
    st.report("(a) fixture")
    st.check()
    plain = sea.wb_denoise_batch(b, want_f32=True, want_hb=True)
    torch.cuda.synchronize()
    for k in ("out", "f32", "hp_rows", "code_rows", "first_out", "onset"):
        x, y = raw[k].cpu().numpy(), plain[k].cpu().numpy()
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{k} differs from wb_denoise_batch's"
        print(f"  {k}: {x.size} values equal wb_denoise_batch's bit for bit")


def _edge_batch():
    from speech_enhancement_amd import corpus
    z = lambda n: np.zeros(n, np.int16)  # noqa: E731
    utts, what, derived = [], [], []
    for i, n in enumerate((4, 5, 6, 7, 8, 13, 14, 15)):  # around the first output, the first cepstrum and the tile of 8
        utts.append(corpus.synth_wideband(60 + i, 160 * n))
        what.append(f"{n} frames")
        derived.append(max(n - 6, 0))
    utts.append(corpus.synth_wideband(70, 160 * 15 + 77))
    what.append("15 frames + 77 samples")
    derived.append(9)
    utts.append(np.concatenate([z(3 * 160), corpus.synth_wideband(71, 160 * 40)]))
    what.append("40 frames after 3 zero frames")
    derived.append(34)
    utts.append(np.concatenate([z(400), corpus.synth_wideband(72, 160 * 40)]))  # 2 zero frames, the third half zero
    what.append("40 frames after 400 zeros")
    derived.append((400 + 160 * 40) // 160 - 2 - 6)
    utts.append(z(160 * 20))
    what.append("20 zero frames")
    derived.append(0)
    utts.append((corpus.synth_wideband(3, 32000) // 128)[:160 * 60])
    what.append("the quiet utterance cut to 60 frames")
    derived.append(54)
    return utts, what, derived


def test_b_edges_against_the_reference():
    """(b) utterances around the first output, the first cepstral frame and the tile of eight, ragged, behind whole and
    half zero frames, all zero, and quiet, in one batch against the reference run here.  The cepstral frame counts derived
    from the lengths are printed beside the reference's; the reference decides."""
    A = _reference()
    utts, what, derived = _edge_batch()
    res = _run(utts)
    st = _Stats()
    for u, x in enumerate(utts):
        want = A.trace(x)
        nfr = len(x) // 160
        note = "" if len(want["feat_cc"]) == derived[u] else f"  (derived {derived[u]}: the reference decides)"
        print(f"  {what[u]}: {nfr} frames, first_out {want['first_out']}, onset {want['onset']}, {len(want['feat_cc'])} cepstral, "
              f"{len(want['feat15'])} emitted, {want['n_null']} null lead, {int(want['bypass'].sum())} bypassed{note}")
        _compare(st, res[u], want, nfr, what[u])
    st.report("(b) edges")
    st.check()


def test_c_composition():
    """(c) each fixture utterance alone equals its rows of the batch; neither the launch order nor the order of the
    utterances in the batch changes a result"""
    g = _fixture()
    utts = [g[f"x{u}"] for u in range(N_FIXTURE)]
    a = _fixture_run()[0]
    keys = ("feats", "feat_cc", "feat_pp", "flags", "out", "f32", "hp", "code")
    scal = ("n_ceps", "first_out", "onset")

    def same(x, y, why):
        for k in keys:
            assert x[k].shape == y[k].shape and np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), f"{k} {why}"
        assert all(x[k] == y[k] for k in scal), why

    b = _run(utts, use_order=False)
    c = _run(utts[::-1])
    for u in range(N_FIXTURE):
        same(a[u], b[u], f"of utterance {u} depends on the launch order")
        same(a[u], c[N_FIXTURE - 1 - u], f"of utterance {u} depends on its place in the batch")
        same(a[u], _run([utts[u]])[0], f"of utterance {u} alone differs from its rows of the batch")
    print(f"\n(c) {N_FIXTURE} utterances: alone, without the launch order and reversed, {len(keys)} arrays each equal bit for bit")


def test_d_bypassed_frames_equal_the_plain_cepstrum():
    """(d) no reference involved: a cepstral frame that took WaveProc's bypass (recorded in the fixture) has the row
    wb_compceps_batch gives for the same frame, bit for bit, because WaveProc left it alone; of the frames WaveProc ran on, on
    the wideband utterances of 3 s, at least half differ from it (the reference alone: every one of 882,
    tests/test_wb_afe_cpu.py::test_waveproc_changes_the_cepstra_of_the_frames_it_runs_on)"""
    import speech_enhancement_amd as sea
    torch = _torch()
    g = _fixture()
    res, b, raw = _fixture_run()
    ceps, cum, n_ceps = sea.wb_compceps_batch(b, raw)
    torch.cuda.synchronize()
    ceps, n_ceps = ceps.cpu().numpy(), n_ceps.cpu().numpy()
    nbypass = nrun = ndiffer = 0
    for u in range(N_FIXTURE):
        bypass = g[f"bypass{u}"]
        assert int(n_ceps[u]) == res[u]["n_ceps"] == len(bypass)
        plain = ceps[cum[u]:cum[u] + len(bypass)]
        differ = (_u32(plain) != _u32(res[u]["feat_cc"])).any(axis=1) if len(bypass) else np.zeros(0, bool)
        assert not differ[bypass].any(), f"utterance {u}: bypassed frames {np.flatnonzero(differ & bypass)[:8]} differ from the plain cepstrum"
        nbypass += int(bypass.sum())
        if u in (2, 3, 4):
            nrun += int((~bypass).sum())
            ndiffer += int(differ[~bypass].sum())
    print(f"\n(d) {nbypass} bypassed frames equal the plain wideband cepstrum bit for bit; {ndiffer} of {nrun} frames WaveProc ran on differ from it")
    assert nbypass >= 100 and 2 * ndiffer >= nrun > 0
