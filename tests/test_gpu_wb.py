"""GPU tests of the ETSI wideband (16 kHz) mode (sea_wb_denoise_batch / sea_wb_compceps_batch / sea_wb_denoise): QMF split,
NoiseSup on the low band, the high band's spectrally subtracted mel bands and code, the 26-band cepstrum -- against the
reference's own wideband mode (AdvProcessAlloc (16000), driven by tests/wb_reference.py) and against its recorded outputs
(tests/golden/wb_golden.npz, tools/gen_wb_golden.py).

Tolerances are the project's: int16 max |delta| <= 2 LSB and >= 99.9 % exact, zero
tolerance on which samples are zero and on every count; floats |delta| <= 1e-4 max(1, |ref|); cepstra |delta| <= 1e-3.
The expectation is bit-identical; every test prints what it measured.  A high-band VAD decision that differed from the
reference's would show up as a high-band row far outside tolerance.

The corpus utterances (harmonics up to 1.65 kHz) never move the high band's VAD; the wideband signals
(corpus.synth_wideband) do, and every one of 3 s or more used in (a) and (b) must have the REFERENCE's high-band VAD in
each of its three states (speech run / hang-over / idle) for at least 5 % of its frames -- asserted below.
Run on an MI355X with ``pytest -m gpu``."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wb_golden.npz")
MIN_SHARE = 0.05


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _reference():
    from tests import wb_reference as W
    if not W.available():
        pytest.fail("oracle/_ref/libetsi_ref.so is missing: `make -C oracle ref` builds it where the reference's sources "
                    "are; this test needs the built library beside the tree")
    return W


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(utts, use_order=True):
    """The whole wideband path on a batch -> per utterance dicts of numpy arrays."""
    import speech_enhancement_amd as sea
    torch = _torch()
    b = sea.PackedBatch.from_arrays(utts, device="cuda:0")
    r = sea.wb_denoise_batch(b, want_f32=True, want_hb=True, use_order=use_order)
    ceps, cum, n_ceps = sea.wb_compceps_batch(b, r)
    torch.cuda.synchronize()
    out, f32, lp, hp = (sea.wb_split(b, r[k]) for k in ("out", "f32", "qmf_lp", "qmf_hp"))
    hpr, code = sea.wb_rows(b, r["hp_rows"]), sea.wb_rows(b, r["code_rows"])
    first, onset = r["first_out"].cpu().numpy(), r["onset"].cpu().numpy()
    n_ceps, ceps = n_ceps.cpu().numpy(), ceps.cpu().numpy()
    res = []
    for u, x in enumerate(utts):
        nfr = len(x) // 160
        res.append(dict(out=out[u], f32=f32[u].reshape(nfr, 80), qmf_lp=lp[u].reshape(nfr, 80), qmf_hp=hp[u].reshape(nfr, 80),
                        hp=hpr[u], code=code[u], first_out=int(first[u]), onset=int(onset[u]), n_ceps=int(n_ceps[u]),
                        ceps=ceps[cum[u]:cum[u] + int(n_ceps[u])], ceps_cap=ceps[cum[u]:cum[u + 1]]))
    return res


class _Stats:
    def __init__(self):
        self.i16_max = 0
        self.i16_n = self.i16_diff = 0
        self.f = {}

    def i16(self, got, want):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        self.i16_max = max(self.i16_max, int(d.max()) if d.size else 0)
        self.i16_n += d.size
        self.i16_diff += int((d != 0).sum())

    def flt(self, key, got, want, rel):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        if rel:
            d = d / np.maximum(1.0, np.abs(want.astype(np.float64)))
        m, n, nb = self.f.get(key, (0.0, 0, 0))
        self.f[key] = (max(m, float(d.max()) if d.size else 0.0), n + d.size, nb + int((_u32(got) != _u32(want)).sum()))

    def report(self, title):
        print(f"\n{title}: int16 max |delta| {self.i16_max} LSB, {self.i16_diff} of {self.i16_n} samples differ")
        for k, (m, n, nb) in self.f.items():
            print(f"  {k}: max error {m:.3g}, {nb} of {n} values differ in bits")

    def check(self):
        assert self.i16_max <= 2, f"int16 max |delta| {self.i16_max} LSB"
        assert self.i16_diff <= 1e-3 * max(self.i16_n, 1), f"{self.i16_diff} of {self.i16_n} int16 samples differ"
        for k, (m, n, nb) in self.f.items():
            assert m <= (1e-3 if k == "ceps" else 1e-4), f"{k}: max error {m}"
            assert nb == 0, f"{k}: {nb} of {n} values differ in bits"


def _compare(st, got, want, nfr, what, f32=True):
    """got: one entry of _run; want: keys as wb_reference.trace returns them (f32 optional)"""
    assert got["first_out"] == want["first_out"], f"{what}: first_out {got['first_out']} != {want['first_out']}"
    assert got["onset"] == want["onset"], f"{what}: onset {got['onset']} != {want['onset']}"
    fo = want["first_out"]
    nout = nfr - fo if fo >= 0 else 0
    assert len(want["hp"]) == nout
    lead = 80 * (fo if fo >= 0 else nfr)
    assert not got["out"][:lead].any() and not want["out_i16"][:lead].any(), f"{what}: non-zero samples before the first output"
    st.i16(got["out"], want["out_i16"])
    nceps = max(nout - 2, 0)
    assert got["n_ceps"] == nceps == len(want["ceps"]), f"{what}: {got['n_ceps']} cepstral frames, reference {len(want['ceps'])}"
    assert not got["ceps_cap"][nceps:].any(), f"{what}: rows behind the last cepstral frame were written"
    if nout:
        if f32:
            st.flt("float stream", got["f32"][fo:], want["f32"], True)
        st.flt("high-band rows", got["hp"][fo:], want["hp"], True)
        st.flt("code", got["code"][fo:], want["code"], True)
    if nceps:
        st.flt("ceps", got["ceps"], want["ceps"], False)
    quiet = fo if fo >= 0 else nfr  # frames without an output: their rows (zero-filled by the caller) stay untouched
    assert not got["hp"][:quiet].any() and not got["code"][:quiet].any() and not got["f32"][:quiet].any(), \
        f"{what}: rows of frames without an output were written"


def test_a_fixture_batch():
    """(a) the batch entry on all fixture utterances at once against the stored reference outputs; no reference library"""
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    utts = [g[f"x{u}"] for u in range(6)]
    for u in (2, 3, 4):  # the condition that keeps this test honest, from the counts stored at generation
        nfr = len(utts[u]) // 160
        assert nfr >= 300 and (g["vad_states"][u] / nfr).min() >= MIN_SHARE, (u, g["vad_states"][u])
    res = _run(utts)
    st = _Stats()
    for u, x in enumerate(utts):
        want = dict(out_i16=g[f"out{u}"], hp=g[f"hp{u}"], code=g[f"code{u}"], ceps=g[f"ceps{u}"],
                    first_out=int(g["first_out"][u]), onset=int(g["onset"][u]))
        have_f32 = f"f32_{u}" in g
        if have_f32:
            want["f32"] = g[f"f32_{u}"]
        _compare(st, res[u], want, len(x) // 160, f"fixture utterance {u}", f32=have_f32)
    st.report("(a) fixture")
    st.check()


def _live_batch():
    from speech_enhancement_amd import corpus
    z = lambda k: np.zeros(160 * k, np.int16)  # noqa: E731
    utts, wide3 = [], []
    # half corpus: 0.2 .. 6 s, some ragged (L % 160 != 0); every fifth has 400 leading zeros by construction
    clen = [3200, 4800, 8000, 12345, 16000, 20000, 24077, 28800, 32000, 36000, 40000, 44111, 48000, 52000, 56000, 60001,
            64000, 68000, 72000, 76159, 80000, 84000, 88000, 92000, 96000, 6400, 9600, 14400, 19200, 25600, 35200, 51200, 70400, 30000]
    utts += [corpus.synth_utterance(100 + i, L) for i, L in enumerate(clen)]
    # wideband, 3 .. 6 s: the ones the high-band condition is about; some with leading zero frames and a ragged tail
    for i in range(24):
        L = 48000 + 2000 * i + (77 if i % 3 == 0 else 0)
        x = corpus.synth_wideband(i, L)
        if i % 4 == 1:
            x = np.concatenate([z(1 + i % 5), x])
        wide3.append(len(utts))
        utts.append(x)
    # shorter wideband ones (they do not count towards the condition), edge cases
    utts += [corpus.synth_wideband(30 + i, L) for i, L in enumerate([3200, 5000, 8000, 16000, 20001, 24000, 32000, 40000])]
    utts += [np.concatenate([z(3), corpus.synth_wideband(40, 16000)]), z(20), np.zeros(0, np.int16), np.zeros(100, np.int16)]
    utts += [corpus.synth_wideband(50 + n, 160 * n + (13 if n % 2 else 0)) for n in range(1, 7)]
    return utts, wide3


def test_b_live_batch_against_the_reference():
    """(b) >= 64 utterances of 0.2 .. 6 s, half corpus and half wideband, with ragged lengths, leading zero frames, an
    all-zero and an empty utterance and utterances of 1 .. 6 frames, against the reference run here"""
    W = _reference()
    utts, wide3 = _live_batch()
    assert len(utts) >= 64 and 4 * len(wide3) >= len(utts)
    res = _run(utts)
    st = _Stats()
    shares = []
    for u, x in enumerate(utts):
        want = W.trace(x)
        nfr = len(x) // 160
        if u in wide3:
            assert len(x) >= 48000
            share = want["vad_states"] / nfr
            shares.append(share)
            assert share.min() >= MIN_SHARE, f"utterance {u}: the reference's high-band VAD spent {want['vad_states']} of {nfr} frames in (speech run, hang-over, idle)"
        _compare(st, res[u], want, nfr, f"utterance {u} ({len(x)} samples)")
    shares = np.array(shares)
    print(f"\n(b) {len(utts)} utterances, {len(wide3)} wideband of >= 3 s; smallest share of frames per high-band VAD state "
          f"(speech run, hang-over, idle): {shares.min(axis=0).round(3)}")
    st.report("(b) live batch")
    st.check()


def test_c_qmf_streams_bit_identical():
    """(c) the QMF alone: 236 rounded operations per sample in a fixed order -- any difference is a bug"""
    W = _reference()
    from speech_enhancement_amd import corpus
    utts = [corpus.synth_wideband(3, 16000), corpus.synth_utterance(5, 8000), corpus.synth_utterance(7, 12000 + 91),
            np.concatenate([np.zeros(320, np.int16), corpus.synth_wideband(8, 9000)]),
            (corpus.synth_wideband(9, 4800).astype(np.int32) * 3).clip(-32768, 32767).astype(np.int16),
            np.full(1600, -32768, np.int16), np.concatenate([np.zeros(159, np.int16), np.ones(1, np.int16), np.zeros(800, np.int16)])]
    res = _run(utts)
    nbad = ntot = 0
    for u, x in enumerate(utts):
        want = W.trace(x, want_qmf=True)
        on = want["onset"]
        assert res[u]["onset"] == on
        for k in ("qmf_lp", "qmf_hp"):
            assert not res[u][k][:on].any(), f"utterance {u}: {k} before the onset is not zero"
            bad = int((_u32(res[u][k][on:]) != _u32(want[k][on:])).sum())
            nbad += bad
            ntot += want[k][on:].size
            assert bad == 0, f"utterance {u}: {bad} of {want[k][on:].size} {k} samples differ in bits"
    print(f"\n(c) QMF streams: {nbad} of {ntot} samples differ in bits")


def test_d_low_band_equals_the_streaming_kernel():
    """(d) no reference involved: the float low-band output equals sea_ns_streams_push (the one-wave streaming form) on
    the same QMF low-band frames from the onset on, bit for bit"""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    torch = _torch()
    utts = [corpus.synth_wideband(11, 32000), corpus.synth_utterance(12, 24000), corpus.synth_utterance(15, 16000 + 33),
            np.concatenate([np.zeros(480, np.int16), corpus.synth_wideband(13, 20000)]), corpus.synth_wideband(14, 960)]
    res = _run(utts)
    ntot = 0
    for u, x in enumerate(utts):
        nfr, on = len(x) // 160, res[u]["onset"]
        frames = torch.from_numpy(res[u]["qmf_lp"][on:].copy()).to("cuda:0")[None]
        out, produced, _ = sea.ns_streams_push(frames)
        torch.cuda.synchronize()
        produced = produced[0].cpu().numpy().astype(bool)
        want = out[0].cpu().numpy()[produced]
        first = on + int(np.argmax(produced)) if produced.any() else -1
        assert res[u]["first_out"] == first == (on + 4 if nfr - on >= 5 else -1)
        got = res[u]["f32"][first:] if first >= 0 else res[u]["f32"][:0]
        assert got.shape == want.shape
        assert np.array_equal(_u32(got), _u32(want)), f"utterance {u}: {int((_u32(got) != _u32(want)).sum())} of {got.size} samples differ"
        ntot += got.size
    print(f"\n(d) {ntot} float low-band samples equal the streaming kernel's bit for bit")


def test_e_single_call_order_and_batch_composition():
    """(e) sea_wb_denoise on one utterance equals its row of the batch; results depend neither on the launch order nor on
    what else is in the batch"""
    import speech_enhancement_amd as sea
    from speech_enhancement_amd import corpus
    _torch()
    utts = [corpus.synth_wideband(20, 48000), corpus.synth_utterance(21, 16000 + 50), corpus.synth_utterance(25, 30000),
            np.concatenate([np.zeros(160, np.int16), corpus.synth_wideband(22, 24000)]), corpus.synth_wideband(23, 800),
            np.zeros(0, np.int16), corpus.synth_wideband(24, 64000)]
    a = _run(utts)
    b = _run(utts, use_order=False)
    pick = [6, 3, 0, 4]
    c = _run([utts[i] for i in pick])
    keys = ("out", "f32", "qmf_lp", "qmf_hp", "hp", "code", "ceps")
    for u in range(len(utts)):
        for k in keys:
            assert np.array_equal(a[u][k].view(np.uint8), b[u][k].view(np.uint8)), f"utterance {u}: {k} depends on the order"
        assert (a[u]["first_out"], a[u]["onset"], a[u]["n_ceps"]) == (b[u]["first_out"], b[u]["onset"], b[u]["n_ceps"])
        one = sea.wb_denoise(utts[u])
        assert one.shape == a[u]["out"].shape and np.array_equal(one, a[u]["out"]), f"utterance {u}: sea_wb_denoise != batch row"
    for j, u in enumerate(pick):
        for k in keys:
            assert np.array_equal(a[u][k].view(np.uint8), c[j][k].view(np.uint8)), f"utterance {u}: {k} depends on the batch"
        assert (a[u]["first_out"], a[u]["onset"], a[u]["n_ceps"]) == (c[j]["first_out"], c[j]["onset"], c[j]["n_ceps"])
