"""The Hu-Wang AM labels, final grouping and the whole estimator on the GPU (csrc/hw25_am_kernel.hip) against what the
reference's own computeAM / finalSeg / createIBM produced (tests/golden/hw25_am_golden.npz) and, where the fixture holds
nothing, the numpy model that the CPU tests pin to that fixture (tests/hw25_am_model.py).  gOut, the AM pattern before and
after its normalisation and sEng are compared bit for bit, ratio = error / sEng within the fixture's ratio_tol (sinModel's
cosf / sinf / atanf are the double functions rounded to float: DESIGN.md section 5.13), the labels, every stage of finalSeg and
the mask exactly.

The audio batch: the fixture's eight inputs (p12000 has N = 14: four LDS pieces and two stages over global memory); then 0,
79, 80, 240 and 400 samples against the model; then 150001 samples of zeros, one more than the FFT is built for.  Every output
buffer is filled with a sentinel and carries guard rows; every call also runs in a permuted launch order and without its
optional outputs.  A second batch feeds arrays straight to sea_hw25_finalseg_batch; a third one takes the FFT to its largest
size, N = 18; a fourth one is large enough for the FFT to run in five groups of five channels and holds a pitch out of range."""
import ctypes

import numpy as np
import pytest

from tests import hw25_am_model as AM
from tests import hw25_model as M
from tests import hw25_pitch_model as PM

pytestmark = pytest.mark.gpu

NCH = 25
SENT, SENT_I = -7777.25, -77
GUARD = 3
FW = len(AM.FINAL_STAGES) * NCH


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from speech_enhancement_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device="cuda:0")


def _blocks(batch, t):
    """a tensor in gOut's layout -> per utterance (the [25][L] array, its padding columns)"""
    host = t.cpu().numpy()
    out = []
    for off, L in zip(batch.host_offsets, batch.host_lengths):
        pitch = (int(L) + 7) // 8 * 8
        b = host[off * NCH:off * NCH + NCH * pitch].reshape(NCH, pitch)
        out.append((b[:, :int(L)], b[:, int(L):]))
    return out


def _against_crcs(got, g, name, k):
    idx = AM.sample_index(got.shape[1])
    bad = np.flatnonzero(np.ascontiguousarray(got).ravel()[idx].view(np.uint32) != g[f"{name}_s_{k}"].view(np.uint32))
    assert not len(bad), f"{k}: {name} differs first at flat index {idx[bad[0]]}"
    assert np.array_equal(AM.channel_crcs(got), g[f"{name}_crc_{k}"]), f"{k}: {name} CRCs"


# ---- the audio batch -----------------------------------------------------------------------------------------------------------
N_FIX = len(AM.AUDIO_CASES)
PERM = [13, 4, 8, 0, 11, 6, 2, 9, 7, 12, 1, 5, 10, 3]


def extra_inputs():
    """the short inputs of the audio batch that the fixture does not hold (the models judge them): no sample, no frame, one
    frame, three frames, five frames; also what tools/hw_oracle_coverage.py feeds the reference as part of `hw-tests`"""
    n = np.arange(400)
    xs = PM.audio_inputs()
    return [np.zeros(0, np.float32), (40 * np.sin(2 * np.pi * 200 * n[:79] / 8000)).astype(np.float32),
            (900 * np.sin(2 * np.pi * 300 * n[:80] / 8000)).astype(np.float32),
            (3000 * np.sin(2 * np.pi * 125 * n[:240] / 8000) + 1500 * np.sin(2 * np.pi * 250 * n[:240] / 8000)).astype(np.float32),
            xs["p"][2000:2400].copy()]


def am_launch(a, order=None, details=True):
    """sea_hw25_am_batch on sentinel-filled outputs with guard rows -> numpy arrays"""
    import torch
    lib_mod, lib = _lib()
    batch, total, n_utt = a["batch"], int(a["rows"].sum()), len(a["utts"])
    o = dict(amcrn=_full((total + GUARD, NCH), SENT, torch.float32), status=_full((n_utt + GUARD,), SENT_I, torch.int32))
    for k in ("ratio", "seng"):
        o[k] = _full((total + GUARD, NCH), SENT, torch.float32) if details else None
    for k in ("ampatt", "am"):
        o[k] = _full((batch.total * NCH + 64,), SENT, torch.float32) if details else None
    nbytes = int(lib.sea_hw25_am_scratch_bytes(batch.total, n_utt))
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    rc = lib.sea_hw25_am_batch(_ptr(a["gout"]), _ptr(a["pitch"]), _ptr(batch.offsets), _ptr(batch.lengths), _ptr(a["row_offsets"]),
                               _ptr(o["amcrn"]), _ptr(o["ratio"]), _ptr(o["seng"]), _ptr(o["ampatt"]), _ptr(o["am"]), _ptr(o["status"]),
                               _ptr(scratch), batch.total, _ptr(order), n_utt, _stream())
    lib_mod.check(rc, "sea_hw25_am_batch")
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}, o


@pytest.fixture(scope="module")
def audio():
    """the batch, its periphery on the GPU (computed once, never changed) and what every utterance must give"""
    import torch
    import speech_enhancement_amd as sea
    g = AM.load_golden()
    t = M.tables()
    utts = [g[f"x_{k}"] for k in AM.AUDIO_CASES]
    extra = extra_inputs()
    model = []
    for x in extra:  # the whole chain from the models
        fr = M.frontend(x, t) if len(x) >= 80 else None
        nfr = len(x) // 80
        ps = PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"]) if nfr else dict(pitch=np.zeros(0, np.int32), status=0)
        am = AM.am_stage(AM.gout(x, t), ps["pitch"])
        fin = AM.final_seg(ps["grp"], am["amcrn"], fr["cross_ev"], ps["pratio"]) if nfr else dict(mask=np.zeros((0, NCH), np.float32), status=0)
        model.append(dict(pitch=ps["pitch"], am=am, mask=fin["mask"], status=ps["status"] | am["status"] | fin["status"]))
    utts = utts + extra + [np.zeros(150001, np.float32)]
    assert [len(x) // 80 for x in utts] == [50, 50, 50, 50, 50, 25, 20, 150, 0, 0, 1, 3, 5, 1875] and sorted(PERM) == list(range(len(utts)))
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    # the periphery with gOut on a sentinel-filled buffer, and without it
    lib_mod, lib = _lib()
    hout, hev, gout = (_full((batch.total * NCH + 64,), SENT, torch.float32) for _ in range(3))
    lib_mod.check(lib.sea_hw25_periphery_gout_batch(_ptr(batch.data), _ptr(hout), _ptr(hev), _ptr(gout), _ptr(batch.offsets),
                                                    _ptr(batch.lengths), _ptr(batch.order), batch.n_utt, _stream()), "periphery_gout")
    hout0, hev0 = (_full((batch.total * NCH + 64,), SENT, torch.float32) for _ in range(2))
    lib_mod.check(lib.sea_hw25_periphery_batch(_ptr(batch.data), _ptr(hout0), _ptr(hev0), _ptr(batch.offsets), _ptr(batch.lengths),
                                               _ptr(batch.order), batch.n_utt, _stream()), "periphery")
    hout1, hev1, gout1 = (_full((batch.total * NCH + 64,), SENT, torch.float32) for _ in range(3))  # in index order
    lib_mod.check(lib.sea_hw25_periphery_gout_batch(_ptr(batch.data), _ptr(hout1), _ptr(hev1), _ptr(gout1), _ptr(batch.offsets),
                                                    _ptr(batch.lengths), None, batch.n_utt, _stream()), "periphery_gout")
    torch.cuda.synchronize()
    assert not np.array_equal(batch.order.cpu().numpy(), np.arange(batch.n_utt)), "the batch's launch order is no permutation"
    for one, other in ((hout, hout1), (hev, hev1), (gout, gout1)):
        assert torch.equal(one.view(torch.int32), other.view(torch.int32)), "the periphery depends on the launch order"
    # the reference-equal pitch: the fixture's, the model's for the short inputs, none for the over-long one
    pitch = np.concatenate([g[f"pitch_{k}"] for k in AM.AUDIO_CASES] + [m["pitch"] for m in model] + [np.zeros(1875, np.int32)])
    a = dict(g=g, utts=utts, model=model, batch=batch, rows=rows, offs=offs, gout=gout, hout=hout, hev=hev, hout0=hout0, hev0=hev0,
             pitch=torch.from_numpy(pitch.astype(np.int32)).to("cuda:0"), row_offsets=torch.from_numpy(offs).to("cuda:0"))
    a["before"] = {k: a[k].clone() for k in ("gout", "pitch")}
    a["runs"] = {"plain": am_launch(a)[0], "nodetails": am_launch(a, details=False)[0],
                 "permuted": am_launch(a, order=torch.tensor(PERM, dtype=torch.int32, device="cuda:0"))[0]}
    return a


def test_gout_is_the_references_and_hout_hev_are_unchanged(audio):
    import torch
    assert torch.equal(audio["hout"].view(torch.int32), audio["hout0"].view(torch.int32)), "hOut changed with d_gout"
    assert torch.equal(audio["hev"].view(torch.int32), audio["hev0"].view(torch.int32)), "hEv changed with d_gout"
    t = M.tables()
    blocks = _blocks(audio["batch"], audio["gout"])
    for u, k in enumerate(AM.AUDIO_CASES):
        _against_crcs(blocks[u][0], audio["g"], "gout", k)
    for u in range(N_FIX, N_FIX + 5):
        assert M.same_bits(np.ascontiguousarray(blocks[u][0]), AM.gout(audio["utts"][u], t)), f"utterance {u}: gOut"
    for u, (body, pad) in enumerate(blocks):
        assert not (body == SENT).any() and (pad == SENT).all(), f"utterance {u}: gOut's padding was written, or a sample was not"
    assert (audio["gout"][audio["batch"].total * NCH:] == SENT).all()


def _check_am(audio, out, run, details=True):
    g, tol = audio["g"], float(audio["g"]["ratio_tol"])
    total, n_utt = int(audio["rows"].sum()), len(audio["utts"])

    def rows(name, u):
        return out[name][int(audio["offs"][u]):int(audio["offs"][u]) + int(audio["rows"][u])]

    for u, k in enumerate(AM.AUDIO_CASES):
        assert out["status"][u] == 0
        assert np.array_equal(rows("amcrn", u), g[f"amcrn_{k}"].astype(np.float32)), f"{run}, {k}: AmCrn"
        if details:
            assert M.same_bits(np.ascontiguousarray(rows("seng", u)), g[f"seng_{k}"]), f"{run}, {k}: sEng"
            ref, got = g[f"ratio_{k}"], rows("ratio", u)
            on = ref != 0
            assert np.array_equal(got != 0, on), f"{run}, {k}: the units where sinModel runs"
            rel = np.abs(got[on].astype(np.float64) - ref[on]) / ref[on]
            print(f"{run}, {k}: ratio's largest relative difference {rel.max():.3g} (tolerance {tol:.3g})")
            assert rel.max() <= tol, f"{run}, {k}: ratio"
    for i, m in enumerate(audio["model"]):
        u = N_FIX + i
        assert out["status"][u] == m["am"]["status"] == 0
        assert np.array_equal(rows("amcrn", u), m["am"]["amcrn"]), f"{run}, utterance {u}: AmCrn"
        if details:
            assert M.same_bits(np.ascontiguousarray(rows("seng", u)), m["am"]["seng"]), f"{run}, utterance {u}: sEng"
            ref, got = m["am"]["ratio"], rows("ratio", u)
            on = ref != 0
            assert np.array_equal(got != 0, on)
            assert not on.any() or (np.abs(got[on].astype(np.float64) - ref[on]) / ref[on]).max() <= tol, f"{run}, utterance {u}: ratio"
    u = n_utt - 1
    assert out["status"][u] == AM.AM_TOO_LONG and not rows("amcrn", u).any()
    assert (out["amcrn"][total:] == SENT).all() and not (out["amcrn"][:total] == SENT).any()
    assert (out["status"][n_utt:] == SENT_I).all()
    if details:
        assert not rows("ratio", u).any() and not rows("seng", u).any()
        for name in ("ratio", "seng"):
            assert (out[name][total:] == SENT).all() and not (out[name][:total] == SENT).any()
        for name in ("ampatt", "am"):
            host = out[name]
            for v, (off, L) in enumerate(zip(audio["batch"].host_offsets, audio["batch"].host_lengths)):
                pitch = (int(L) + 7) // 8 * 8
                b = host[off * NCH:off * NCH + NCH * pitch].reshape(NCH, pitch)
                assert not (b[:, :int(L)] == SENT).any() and (b[:, int(L):] == SENT).all(), f"{run}, utterance {v}: {name}"
                if v < N_FIX:
                    _against_crcs(b[:, :int(L)], g, name, AM.AUDIO_CASES[v])
                elif v < n_utt - 1:
                    assert M.same_bits(np.ascontiguousarray(b[:, :int(L)]), audio["model"][v - N_FIX]["am"][name]), f"utterance {v}: {name}"
                else:
                    assert not b[:, :int(L)].any()
            assert (host[audio["batch"].total * NCH:] == SENT).all()


@pytest.mark.parametrize("run", ["plain", "permuted"])
def test_am_stage_equals_the_reference_or_the_model(audio, run):
    _check_am(audio, audio["runs"][run], run)


def test_am_stage_without_its_optional_outputs(audio):
    out = audio["runs"]["nodetails"]
    assert out["ratio"] is None and out["ampatt"] is None
    _check_am(audio, out, "nodetails", details=False)
    assert M.same_bits(out["amcrn"], audio["runs"]["plain"]["amcrn"]) and np.array_equal(out["status"], audio["runs"]["plain"]["status"])


def test_am_inputs_are_unchanged(audio):
    import torch
    for k, v in audio["before"].items():
        assert torch.equal(audio[k].view(torch.int32), v.view(torch.int32)), k


def test_an_output_that_is_an_input_is_refused(audio):
    import torch
    _, lib = _lib()
    batch, n_utt = audio["batch"], len(audio["utts"])
    amcrn = torch.zeros((int(audio["rows"].sum()) + 1, NCH), dtype=torch.float32, device="cuda:0")
    status = torch.zeros(n_utt, dtype=torch.int32, device="cuda:0")
    scratch = torch.empty(int(lib.sea_hw25_am_scratch_bytes(batch.total, n_utt)), dtype=torch.uint8, device="cuda:0")
    for am_out, ratio, ampatt in ((audio["gout"], None, None), (amcrn, amcrn, None), (amcrn, None, audio["gout"])):
        rc = lib.sea_hw25_am_batch(_ptr(audio["gout"]), _ptr(audio["pitch"]), _ptr(batch.offsets), _ptr(batch.lengths), _ptr(audio["row_offsets"]),
                                   _ptr(am_out), _ptr(ratio), None, _ptr(ampatt), None, _ptr(status), _ptr(scratch), batch.total, None, n_utt,
                                   _stream())
        assert rc != 0
    rc = lib.sea_hw25_am_batch(_ptr(audio["gout"]), _ptr(audio["pitch"]), _ptr(batch.offsets), _ptr(batch.lengths), _ptr(audio["row_offsets"]),
                               _ptr(amcrn), None, None, None, None, _ptr(amcrn), _ptr(scratch), batch.total, None, n_utt, _stream())
    assert rc != 0, "d_status == d_amcrn must be refused"
    # the whole estimator: the input as an output, and every pair of outputs
    total = int(audio["rows"].sum())
    o = dict(mask=amcrn, pitch=torch.zeros(total + 1, dtype=torch.int32, device="cuda:0"), status=status,
             stages=torch.zeros((total + 1) * FW, dtype=torch.float32, device="cuda:0"))
    big = torch.empty(int(lib.sea_hw25_ibm_scratch_bytes(batch.total, total, n_utt)), dtype=torch.uint8, device="cuda:0")
    pairs = [("mask", batch.data)] + [(a, o[b]) for i, a in enumerate(o) for b in list(o)[:i]]
    assert len(pairs) == 7
    for name, other in pairs:
        p = dict(o, **{name: other})
        rc = lib.sea_hw25_ibm_batch(_ptr(batch.data), _ptr(batch.offsets), _ptr(batch.lengths), _ptr(audio["row_offsets"]), _ptr(p["mask"]),
                                    _ptr(p["pitch"]), _ptr(p["status"]), _ptr(p["stages"]), _ptr(big), batch.total, total, None, n_utt,
                                    _stream())
        assert rc != 0, f"sea_hw25_ibm_batch: {name} shared with another buffer must be refused"
    rc = lib.sea_hw25_periphery_gout_batch(_ptr(batch.data), _ptr(audio["hout"]), _ptr(audio["hev"]), _ptr(audio["hout"]), _ptr(batch.offsets),
                                           _ptr(batch.lengths), None, n_utt, _stream())
    assert rc != 0
    torch.cuda.synchronize()


# ---- the whole estimator ---------------------------------------------------------------------------------------------------------
def ibm_launch(audio, order=None, stages=True):
    import torch
    lib_mod, lib = _lib()
    batch, total, n_utt = audio["batch"], int(audio["rows"].sum()), len(audio["utts"])
    o = dict(mask=_full((total + GUARD, NCH), SENT, torch.float32), pitch=_full((total + GUARD,), SENT_I, torch.int32),
             status=_full((n_utt + GUARD,), SENT_I, torch.int32), stages=_full(((total + GUARD) * FW,), SENT, torch.float32) if stages else None)
    scratch = torch.empty(int(lib.sea_hw25_ibm_scratch_bytes(batch.total, total, n_utt)) + 64, dtype=torch.uint8, device="cuda:0")
    rc = lib.sea_hw25_ibm_batch(_ptr(batch.data), _ptr(batch.offsets), _ptr(batch.lengths), _ptr(audio["row_offsets"]), _ptr(o["mask"]),
                                _ptr(o["pitch"]), _ptr(o["status"]), _ptr(o["stages"]), _ptr(scratch), batch.total, total, _ptr(order), n_utt,
                                _stream())
    lib_mod.check(rc, "sea_hw25_ibm_batch")
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def _check_ibm(audio, out, run):
    g = audio["g"]
    total, n_utt = int(audio["rows"].sum()), len(audio["utts"])
    for u in range(n_utt):
        r0, n = int(audio["offs"][u]), int(audio["rows"][u])
        mask, pitch, status = out["mask"][r0:r0 + n], out["pitch"][r0:r0 + n], int(out["status"][u])
        if u < N_FIX:
            k = AM.AUDIO_CASES[u]
            assert np.array_equal(mask, g[f"mask_{k}"].astype(np.float32)), f"{run}, {k}: the mask is not createIBM's"
            assert np.array_equal(pitch, g[f"pitch_{k}"]) and status >> 16 == 0 and status > 0, f"{run}, {k}: pitch / status {status:#x}"
            if out["stages"] is not None:
                st = out["stages"][r0 * FW:(r0 + n) * FW].reshape(len(AM.FINAL_STAGES), n, NCH)
                for i, name in enumerate(AM.FINAL_STAGES):
                    assert np.array_equal(st[i], g[f"{name}_{k}"].astype(np.float32)), f"{run}, {k}: {name}"
        elif u < n_utt - 1:
            m = audio["model"][u - N_FIX]
            assert np.array_equal(mask, m["mask"]) and np.array_equal(pitch, m["pitch"]) and status == m["status"], f"{run}, utterance {u}"
        else:
            assert status & AM.AM_TOO_LONG and not mask.any(), f"{run}: the over-long utterance, status {status:#x}"
    assert (out["mask"][total:] == SENT).all() and not (out["mask"][:total] == SENT).any()
    assert (out["pitch"][total:] == SENT_I).all() and not (out["pitch"][:total] == SENT_I).any()
    assert (out["status"][n_utt:] == SENT_I).all() and not (out["status"][:n_utt] == SENT_I).any()
    if out["stages"] is not None:
        assert (out["stages"][total * FW:] == SENT).all() and not (out["stages"][:total * FW] == SENT).any()


def test_whole_estimator_gives_createibms_mask(audio):
    import torch
    data = audio["batch"].data.clone()
    plain = ibm_launch(audio)
    _check_ibm(audio, plain, "plain")
    nost = ibm_launch(audio, stages=False)
    _check_ibm(audio, nost, "no stages")
    assert M.same_bits(plain["mask"], nost["mask"])
    _check_ibm(audio, ibm_launch(audio, order=torch.tensor(PERM, dtype=torch.int32, device="cuda:0")), "permuted")
    assert torch.equal(audio["batch"].data.view(torch.int32), data.view(torch.int32)), "the input changed"
    assert sum(int(audio["g"][f"mask_{k}"].sum()) for k in AM.AUDIO_CASES) > 2000


def test_python_layer_and_single_utterance_form(audio):
    import speech_enhancement_amd as sea
    g = audio["g"]
    res = sea.hw25_ibm_batch(audio["batch"], stages=True)
    for u, k in enumerate(AM.AUDIO_CASES):
        got = res.utterance(u)
        assert np.array_equal(got["mask"], g[f"mask_{k}"].astype(np.float32)) and np.array_equal(got["pitch"], g[f"pitch_{k}"]), k
        assert np.array_equal(got["final_reseg2"], g[f"final_reseg2_{k}"].astype(np.float32)), k
    assert sea.hw25_ibm_batch(audio["batch"], use_order=False).stages is None
    for u in (0, 5, 6):
        k = AM.AUDIO_CASES[u]
        got = sea.hw25_ibm(audio["utts"][u])
        assert np.array_equal(got["mask"], g[f"mask_{k}"].astype(np.float32)) and np.array_equal(got["pitch"], g[f"pitch_{k}"]), k
        assert got["status"] >> 16 == 0
    for u in (9, 11, 12):
        got, m = sea.hw25_ibm(audio["utts"][u]), audio["model"][u - N_FIX]
        assert np.array_equal(got["mask"], m["mask"]) and got["status"] == m["status"], u
    assert sea.hw25_ibm(np.zeros(1600, np.float32))["mask"].shape == (20, 25)
    empty = sea.hw25_ibm(np.zeros(0, np.float32))
    assert empty["mask"].shape == (0, 25) and empty["pitch"].shape == (0,) and empty["status"] == 0
    hout, hev, gout = sea.hw25_periphery_gout_batch(audio["batch"])
    assert M.same_bits(sea.hw25_split(audio["batch"], gout)[6], _blocks(audio["batch"], audio["gout"])[6][0])
    am = sea.hw25_am_batch(audio["batch"], gout, audio["pitch"], want_details=True)
    assert np.array_equal(am.utterance(6)["amcrn"], g["amcrn_w1600"].astype(np.float32))
    _against_crcs(am.utterance(6)["am"], g, "am", "w1600")
    t = sea.hw25_am_tables()
    a, beta = AM.kaiser_constants()
    assert t["a"] == a and t["beta"] == beta and np.array_equal(t["n_at_pow2"], g["n_at_pow2"])
    assert M.same_bits(t["twiddles"][:1023], g["tw_fwd"])
    assert M.same_bits(t["twiddles"][(1 << 13) - 1:(1 << 14) - 1], AM.twiddles(1 << 13))


# ---- arrays straight into sea_hw25_finalseg_batch ---------------------------------------------------------------------------------
def final_launch(cases, order=None, stages=True, grp_final=True):
    import torch
    lib_mod, lib = _lib()
    rows = np.array([c["grp"].shape[0] for c in cases], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    total, n_utt = int(rows.sum()), len(cases)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    inp = {k: dev(np.concatenate([np.asarray(c[k], np.float32) for c in cases])) for k in ("grp", "amcrn", "cross_ev", "pratio")}
    before = {k: v.clone() for k, v in inp.items()}
    o = dict(mask=_full((total + GUARD, NCH), SENT, torch.float32), status=_full((n_utt + GUARD,), SENT_I, torch.int32),
             grp_final=_full((total + GUARD, NCH), SENT, torch.float32) if grp_final else None,
             stages=_full(((total + GUARD) * FW,), SENT, torch.float32) if stages else None)
    scratch = torch.empty(int(lib.sea_hw25_finalseg_scratch_bytes(total, n_utt)) + 64, dtype=torch.uint8, device="cuda:0")
    d_lengths, d_offs = dev(rows * 80 + 7), dev(offs)
    rc = lib.sea_hw25_finalseg_batch(_ptr(inp["grp"]), _ptr(inp["amcrn"]), _ptr(inp["cross_ev"]), _ptr(inp["pratio"]), _ptr(d_lengths),
                                     _ptr(d_offs), _ptr(o["mask"]), _ptr(o["grp_final"]), _ptr(o["status"]), _ptr(o["stages"]),
                                     _ptr(scratch), _ptr(order), n_utt, _stream())
    lib_mod.check(rc, "sea_hw25_finalseg_batch")
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(inp[k].view(torch.int32), v.view(torch.int32)), f"input {k} changed"
    out = {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}
    assert (out["mask"][total:] == SENT).all() and not (out["mask"][:total] == SENT).any()
    assert (out["status"][n_utt:] == SENT_I).all() and not (out["status"][:n_utt] == SENT_I).any()
    if grp_final:
        assert (out["grp_final"][total:] == SENT).all() and not (out["grp_final"][:total] == SENT).any()
    if stages:
        assert (out["stages"][total * FW:] == SENT).all() and not (out["stages"][:total * FW] == SENT).any()
    return out, rows, offs


def test_final_grouping_on_handmade_and_audio_arrays():
    """The fixture's hand-made cases (a pruned and a kept component in each reSegmentation; growth that needs several sweeps
    in both directions; units that turn -2 and then 1; no unit) and the audio cases' stage inputs against the reference's
    arrays; then more than 400 segments and two rows against the model."""
    import torch
    g = AM.load_golden()
    names = tuple(AM.HAND_CASES) + AM.AUDIO_CASES
    cases = [AM.HAND_CASES[k]() for k in AM.HAND_CASES] + [{n: g[f"{n}_{k}"].astype(np.float32) for n in ("grp", "amcrn", "cross_ev", "pratio")}
                                                          for k in AM.AUDIO_CASES]
    want = [{n: g[f"{n}_{k}"].astype(np.float32) for n in AM.FINAL_STAGES + ("grp_final", "mask")} | {"status": 0} for k in names]
    more = [AM.many_final_segments_case(), {k: v[:2] for k, v in AM.hand_minus2().items()}]
    cases += more
    want += [AM.final_seg(**c) for c in more]
    assert want[-2]["status"] == AM.FINAL_TOO_MANY_SEGMENTS and want[-1]["status"] == 0
    perm = torch.tensor(list(reversed(range(len(cases)))), dtype=torch.int32, device="cuda:0")
    base = None
    for run, kw in (("plain", {}), ("permuted", dict(order=perm)), ("bare", dict(stages=False, grp_final=False))):
        out, rows, offs = final_launch(cases, **kw)
        for u, w in enumerate(want):
            r0, n = int(offs[u]), int(rows[u])
            assert int(out["status"][u]) == w["status"], f"{run}, case {u}: status {int(out['status'][u]):#x}"
            assert np.array_equal(out["mask"][r0:r0 + n], w["mask"]), f"{run}, case {u}: mask"
            if out["grp_final"] is not None:
                assert np.array_equal(out["grp_final"][r0:r0 + n], w["grp_final"]), f"{run}, case {u}: grp_final"
            if out["stages"] is not None:
                st = out["stages"][r0 * FW:(r0 + n) * FW].reshape(len(AM.FINAL_STAGES), n, NCH)
                for i, name in enumerate(AM.FINAL_STAGES):
                    assert np.array_equal(st[i], w[name]), f"{run}, case {u}: {name}"
        base = base if base is not None else out["mask"]
        assert M.same_bits(out["mask"], base)
    _, lib = _lib()
    t = torch.zeros((16, NCH), dtype=torch.float32, device="cuda:0")
    meta = torch.tensor([1287, 0], dtype=torch.int64, device="cuda:0")
    st = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    scratch = torch.empty(int(lib.sea_hw25_finalseg_scratch_bytes(16, 1)), dtype=torch.uint8, device="cuda:0")
    rc = lib.sea_hw25_finalseg_batch(_ptr(t), _ptr(t.clone()), _ptr(t.clone()), _ptr(t.clone()), _ptr(meta), _ptr(meta[1:]), _ptr(t), None,
                                     _ptr(st), None, _ptr(scratch), None, 1, _stream())
    assert rc != 0, "mask == grp must be refused"
    ins = [t.clone() for _ in range(3)]
    out = t.clone()
    rc = lib.sea_hw25_finalseg_batch(_ptr(t), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(meta), _ptr(meta[1:]), _ptr(out), None,
                                     _ptr(out), None, _ptr(scratch), None, 1, _stream())
    assert rc != 0, "status == mask must be refused"
    torch.cuda.synchronize()


# ---- the largest FFT ---------------------------------------------------------------------------------------------------------------
def test_longest_supported_utterance_against_the_model():
    """150000 samples, N = 18: 64 LDS pieces per channel (eight trips of the piece loop) and all six stages over global memory,
    on a made-up gOut (noise with a slow envelope) with two short voiced stretches; beside it 4097 samples (N = 13: two pieces,
    one global stage) and 300 samples, so that workgroups of utterances with a smaller N leave the later stages.  Expected
    values from the model; ratio within the fixture's tolerance, labels compared where no ratio lies in the band."""
    import torch
    import speech_enhancement_amd as sea
    rng = np.random.default_rng(18)
    g = AM.load_golden()
    tol = float(g["ratio_tol"])
    lens = [150000, 4097, 300]
    gouts, pitches = [], []
    for L in lens:
        env = 1 + 0.8 * np.sin(2 * np.pi * 100 * np.arange(L) / 8000)
        a = (rng.normal(0, 300, (NCH, L)) * env).astype(np.float32)
        if L > 100000:
            a[[c for c in range(NCH) if c not in (0, 7, 24)]] = 0  # the model transforms the channels that are not all zeros
        gouts.append(a)
        p = np.zeros(L // 80, np.int32)
        p[1:3] = 80
        if L > 4000:
            p[20:27] = [60, 61, 0, 63, 64, 100, 16]
            p[L // 80 - 3:] = 40
        pitches.append(p)
    want = [AM.am_stage(a, p) for a, p in zip(gouts, pitches)]
    batch = sea.PackedBatch.from_arrays([np.zeros(L, np.float32) for L in lens], device="cuda:0", dtype=np.float32)
    packed = np.zeros(batch.total * NCH, np.float32)
    for a, off, L in zip(gouts, batch.host_offsets, lens):
        pitch = (L + 7) // 8 * 8
        packed[off * NCH:off * NCH + NCH * pitch].reshape(NCH, pitch)[:, :L] = a
    res = sea.hw25_am_batch(batch, torch.from_numpy(packed).to("cuda:0"), torch.from_numpy(np.concatenate(pitches)).to("cuda:0"),
                            want_details=True)
    torch.cuda.synchronize()
    for u, w in enumerate(want):
        got = res.utterance(u)
        assert got["status"] == 0
        for name in ("ampatt", "am", "seng"):
            assert M.same_bits(np.ascontiguousarray(got[name]), w[name]), f"L = {lens[u]}: {name}"
        on = w["ratio"] != 0
        assert np.array_equal(got["ratio"] != 0, on) and on.sum() >= (30, 200, 25)[u]
        rel = np.abs(got["ratio"][on].astype(np.float64) - w["ratio"][on]) / w["ratio"][on]
        assert rel.max() <= tol, f"L = {lens[u]}: ratio differs by {rel.max():.3g}"
        clear = ~(np.abs(w["ratio"].astype(np.float64) - AM.THETAE) <= tol * AM.THETAE)
        assert np.array_equal(got["amcrn"][clear], w["amcrn"][clear]), f"L = {lens[u]}: AmCrn"


# ---- the FFT in five groups of five channels, and a pitch out of range --------------------------------------------------------
def test_fft_in_five_channel_groups_and_a_pitch_out_of_range(audio):
    """A batch whose padded extent is above 335 544 samples, where the size rule runs the FFT in five launch groups of five
    channels on buffers laid out per group: the fixture's eight inputs (against the reference's CRCs, sEng, ratio and AmCrn), a
    copy of w1600 whose pitch holds 101 at one frame (AM_BAD_PITCH, every output zero) and three silent utterances of 150 000
    samples that bring the extent there (no voiced frame: they skip the stage, every output zero)."""
    import torch
    import speech_enhancement_amd as sea
    _, lib = _lib()
    g = audio["g"]
    tol = float(g["ratio_tol"])
    utts = [g[f"x_{k}"] for k in AM.AUDIO_CASES] + [g["x_w1600"]] + [np.zeros(150000, np.float32)] * 3
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    n_utt, total = len(utts), int(batch.total)
    up = lambda v: (v + 255) // 256 * 256
    size = lambda chunk: up(4 * n_utt) + 2 * up(total * NCH * 4 + 64) + 2 * up(total * 2 * chunk * 8 + 64)
    assert total > 335544 and total * 2 * NCH * 16 > 256 << 20
    assert int(lib.sea_hw25_am_scratch_bytes(total, n_utt)) == size(5) != size(NCH), "the size rule did not select five groups"
    rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    bad = g["pitch_w1600"].copy()
    bad[3] = 101
    pitch = np.concatenate([g[f"pitch_{k}"] for k in AM.AUDIO_CASES] + [bad] + [np.zeros(1875, np.int32)] * 3).astype(np.int32)
    _, _, gout = sea.hw25_periphery_gout_batch(batch)
    a = dict(batch=batch, rows=rows, utts=utts, gout=gout, pitch=torch.from_numpy(pitch).to("cuda:0"),
             row_offsets=torch.from_numpy(offs).to("cuda:0"))
    out, _ = am_launch(a)
    rows_total = int(rows.sum())
    for name in ("amcrn", "ratio", "seng"):
        assert (out[name][rows_total:] == SENT).all() and not (out[name][:rows_total] == SENT).any(), name
    assert (out["status"][n_utt:] == SENT_I).all()
    for u in range(n_utt):
        r0, n = int(offs[u]), int(rows[u])
        off, L = int(batch.host_offsets[u]), len(utts[u])
        pitch_u = (L + 7) // 8 * 8
        blocks = {name: out[name][off * NCH:off * NCH + NCH * pitch_u].reshape(NCH, pitch_u) for name in ("ampatt", "am")}
        for name, b in blocks.items():
            assert not (b[:, :L] == SENT).any() and (b[:, L:] == SENT).all(), f"utterance {u}: {name}"
        if u < N_FIX:
            k = AM.AUDIO_CASES[u]
            assert out["status"][u] == 0
            for name, b in blocks.items():
                _against_crcs(b[:, :L], g, name, k)
            assert M.same_bits(np.ascontiguousarray(out["seng"][r0:r0 + n]), g[f"seng_{k}"]), f"{k}: sEng"
            assert np.array_equal(out["amcrn"][r0:r0 + n], g[f"amcrn_{k}"].astype(np.float32)), f"{k}: AmCrn"
            ref, got = g[f"ratio_{k}"], out["ratio"][r0:r0 + n]
            on = ref != 0
            assert np.array_equal(got != 0, on) and (np.abs(got[on].astype(np.float64) - ref[on]) / ref[on]).max() <= tol, f"{k}: ratio"
        else:
            assert out["status"][u] == (AM.AM_BAD_PITCH if u == N_FIX else 0), f"utterance {u}: status {int(out['status'][u]):#x}"
            assert not any(out[name][r0:r0 + n].any() for name in ("amcrn", "ratio", "seng")), f"utterance {u}"
            assert not blocks["ampatt"][:, :L].any() and not blocks["am"][:, :L].any(), f"utterance {u}"


# ---- the edge set ------------------------------------------------------------------------------------------------------------
def test_edge_set_through_the_am_stage_the_whole_estimator_and_final_grouping():
    """The edge set (tests/test_hw_edge_coverage_cpu.py) against tests/golden/hw25_edge_golden.npz.

    Audio, in one batch after the fixture's w1600: edc (a step whose ACF rows are exactly 0 and whose pRatio is 0 / 0) and
    ewhole (voiced up to the last frame, its last block of five frames three frames long, so that the pattern filter's window
    runs past the signal's end).  Where the reference finds no segment in edc (at 25 bands) the fixture holds its front half
    alone and the expected arrays are the models' (tests/hw_edge.model_chain): no voiced frame, no label, an empty mask,
    status 0.  The AM stage runs from the expected pitch (AmCrn exact, sEng and the patterns bit for bit, ratio within the
    fixture's ratio_tol), then the whole estimator (mask, pitch, status, finalSeg's stages), each in plain and permuted order
    and without the optional outputs.

    finalSeg: eframe0 (units of the growing value at frame 0 and at the last frame, in the top channel) and the edge audio's
    stage inputs, after the fixture's prune.

    Units of both signs come from eframe0 alone, which is asserted.  The edge audio is not meant to give a -1 unit and gives
    none at either bank: it is there for the ends of the signal and for the zero rows.  The -1 units from audio are those of
    the fixture's own cases, among them w1600, the neighbour in this batch."""
    import torch
    import speech_enhancement_amd as sea
    from tests import hw_edge as E
    e, g = E.load("hw25"), AM.load_golden()
    keys = ["w1600"] + list(E.AUDIO)
    src = [g] + [E.source("hw25", k) for k in E.AUDIO]
    modelled = [False] + [f"status_{k}" in s for s, k in zip(src[1:], keys[1:])]
    assert keys[1:] == ["edc", "ewhole"] and not modelled[2] and modelled[1] == True
    utts = [s[f"x_{k}"] for s, k in zip(src, keys)]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    rows = np.asarray(batch.host_lengths, dtype=np.int64) // 80
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    gout = sea.hw25_periphery_gout_batch(batch)[2]
    pitch = np.concatenate([s[f"pitch_{k}"] for s, k in zip(src, keys)]).astype(np.int32)
    a = dict(utts=utts, batch=batch, rows=rows, offs=offs, gout=gout, pitch=torch.from_numpy(pitch).to("cuda:0"),
             row_offsets=torch.from_numpy(offs).to("cuda:0"))
    tol = float(e["ratio_tol"])
    assert tol == float(g["ratio_tol"])
    assert (e["pitch_ewhole"] > 0).sum() >= 25 and e["pitch_ewhole"][-1] > 0 and e["amcrn_ewhole"].sum() > 100 and e["mask_ewhole"].sum() > 100
    assert not (e["grp_final_ewhole"] < 0).any() and (g["grp_final_w1600"] < 0).any()    # see the docstring
    order = torch.tensor(list(reversed(range(len(keys)))), dtype=torch.int32, device="cuda:0")
    for run, kw in (("plain", {}), ("permuted", dict(order=order)), ("no details", dict(details=False))):
        out = am_launch(a, **kw)[0]
        tally = E.Tally(f"hw25 AM stage, edge audio, {run}")
        for u, (s, k) in enumerate(zip(src, keys)):
            r0, n, L = int(offs[u]), int(rows[u]), len(utts[u])
            assert out["status"][u] == 0
            tally.add(out["amcrn"][r0:r0 + n], s[f"amcrn_{k}"].astype(np.float32), f"{k} amcrn")
            if out["seng"] is None:
                continue
            tally.add(out["seng"][r0:r0 + n], s[f"seng_{k}"], f"{k} seng")
            ref, got = s[f"ratio_{k}"], out["ratio"][r0:r0 + n]
            on = ref != 0
            assert np.array_equal(got != 0, on), f"{run}, {k}: the units where sinModel runs"
            if on.any():
                rel = np.abs(got[on].astype(np.float64) - ref[on]) / ref[on]
                print(f"{run}, {k}: ratio's largest relative difference {rel.max():.3g} (tolerance {tol:.3g}) over {int(on.sum())} units")
                assert rel.max() <= tol, f"{run}, {k}: ratio"
            else:
                assert modelled[u], f"{k}: sinModel runs on no unit"
            for name in ("ampatt", "am"):
                off, pitch_ = int(batch.host_offsets[u]), (L + 7) // 8 * 8
                b = out[name][off * NCH:off * NCH + NCH * pitch_].reshape(NCH, pitch_)
                assert (b[:, L:] == SENT).all(), f"{run}, {k}: {name}'s padding"
                if modelled[u]:
                    tally.add(b[:, :L], s[f"{name}_{k}"], f"{k} {name}")
                else:
                    _against_crcs(b[:, :L], s, name, k)
                    tally.words += NCH * L
        tally.done()
        assert (out["amcrn"][int(rows.sum()):] == SENT).all()
    for run, kw in (("plain", {}), ("permuted", dict(order=order)), ("no stages", dict(stages=False))):
        out = ibm_launch(a, **kw)
        tally = E.Tally(f"hw25 whole estimator, edge audio, {run}")
        for u, (s, k) in enumerate(zip(src, keys)):
            r0, n = int(offs[u]), int(rows[u])
            status = int(out["status"][u])
            if modelled[u]:
                assert status == s[f"status_{k}"] == 0, f"{run}, {k}: status {status:#x}, expected no segment (0)"
            else:
                assert status >> 16 == 0 and status > 0, f"{run}, {k}: status {status:#x}"
            tally.add(out["mask"][r0:r0 + n], s[f"mask_{k}"].astype(np.float32), f"{k} mask")
            tally.add(out["pitch"][r0:r0 + n], s[f"pitch_{k}"], f"{k} pitch")
            if out["stages"] is not None:
                st = out["stages"][r0 * FW:(r0 + n) * FW].reshape(len(AM.FINAL_STAGES), n, NCH)
                for i, name in enumerate(AM.FINAL_STAGES):
                    tally.add(st[i], s[f"{name}_{k}"].astype(np.float32), f"{k} {name}")
        tally.done()
        total = int(rows.sum())
        assert (out["mask"][total:] == SENT).all() and (out["pitch"][total:] == SENT_I).all() and (out["status"][len(keys):] == SENT_I).all()
    # finalSeg
    names = [("prune", g), ("eframe0", e)] + list(zip(keys[1:], src[1:]))
    cases = [AM.HAND_CASES["prune"](), AM.EDGE_HAND_CASES["eframe0"]()]
    cases += [{n: np.asarray(s[f"{n}_{k}"]).astype(np.float32) for n in ("grp", "amcrn", "cross_ev", "pratio")} for k, s in names[2:]]
    w0 = e["grp_final_eframe0"]
    assert (w0 < 0).sum() > 0 and e["mask_eframe0"].sum() > 0 and e["mask_eframe0"][0].any() and w0[-1, NCH - 1] < 0 and w0[-1, NCH - 2] < 0
    perm = torch.tensor(list(reversed(range(len(cases)))), dtype=torch.int32, device="cuda:0")
    for run, kw in (("plain", {}), ("permuted", dict(order=perm)), ("bare", dict(stages=False, grp_final=False))):
        out, frows, foffs = final_launch(cases, **kw)
        tally = E.Tally(f"hw25 finalSeg, edge set, {run}")
        for u, (k, s) in enumerate(names):
            r0, n = int(foffs[u]), int(frows[u])
            assert int(out["status"][u]) == 0
            tally.add(out["mask"][r0:r0 + n], s[f"mask_{k}"].astype(np.float32), f"{k} mask")
            if out["grp_final"] is not None:
                tally.add(out["grp_final"][r0:r0 + n], s[f"grp_final_{k}"].astype(np.float32), f"{k} grp_final")
            if out["stages"] is not None:
                st = out["stages"][r0 * FW:(r0 + n) * FW].reshape(len(AM.FINAL_STAGES), n, NCH)
                for i, name in enumerate(AM.FINAL_STAGES):
                    tally.add(st[i], s[f"{name}_{k}"].astype(np.float32), f"{k} {name}")
        tally.done()
