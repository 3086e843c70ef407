"""The Hu-Wang initial grouping and pitch tracking on the GPU (csrc/hw25_pitch_kernel.hip) against what the reference's own
initGroup / pitchDtm produced (tests/golden/hw25_pitch_golden.npz) and, where the fixture holds nothing, the numpy model that
the CPU tests pin to that fixture (tests/hw25_pitch_model.py).  Every output and every stage array is compared bit for bit.

The audio batch, through sea_hw25_frontend_batch and then sea_hw25_pitch_batch: the fixture's inputs p, q, r, t, m9; s (white
noise, no segment); 79 samples (no row); 240 samples (3 rows); p[2000:2400] (5 rows).  Every output buffer is filled with a
sentinel and carries guard rows.  A second batch feeds hand-made arrays straight to sea_hw25_pitch_batch."""
import ctypes

import numpy as np
import pytest

from tests import hw25_model as M
from tests import hw25_pitch_model as PM

pytestmark = pytest.mark.gpu

NCH, NDEL, WORDS = 25, 101, 55
SENT, SENT_I = -7777.25, -77
GUARD = 3
NAMES = ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from speech_enhancement_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _from_golden(g, k):
    want = {name: g[f"{name}_{k}"] for name in ("pitch", "pratio") + PM.PITCH_STAGES}
    want.update({name: g[f"{name}_{k}"].astype(np.float32) for name in ("grp",) + PM.GRP_STAGES})
    want["status"] = int(g[f"nseg_{k}"])
    return want


def pitch_launch(inp, rows, order=None, stages=True):
    """sea_hw25_pitch_batch on sentinel-filled outputs with guard rows.  inp: device tensors acf, cross, pratio, mark and
    lengths / row_offsets (int64); rows: host row counts.  Returns numpy arrays per output."""
    import torch
    lib_mod, lib = _lib()
    dev = inp["acf"].device
    n_utt, total = len(rows), int(np.sum(rows))

    def full(shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=dev)

    o = dict(pitch=full((total + GUARD,), SENT_I, torch.int32), grp=full((total + GUARD, NCH), SENT, torch.float32),
             pratio=full((total + GUARD, NCH), SENT, torch.float32), status=full((n_utt + GUARD,), SENT_I, torch.int32),
             stages=full(((total + GUARD) * WORDS,), SENT_I, torch.int32) if stages else None)
    nbytes = int(lib.sea_hw25_pitch_scratch_bytes(total, n_utt))
    assert nbytes == 4 * (n_utt * 800 + total * 76)
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    rc = lib.sea_hw25_pitch_batch(_ptr(inp["acf"]), _ptr(inp["cross"]), _ptr(inp["pratio"]), _ptr(inp["mark"]), _ptr(inp["lengths"]),
                                  _ptr(inp["row_offsets"]), _ptr(o["pitch"]), _ptr(o["grp"]), _ptr(o["pratio"]), _ptr(o["status"]),
                                  _ptr(o["stages"]), _ptr(scratch), _ptr(order), n_utt, _stream())
    lib_mod.check(rc, "sea_hw25_pitch_batch")
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def utterance(out, offs, rows, u):
    """one utterance's arrays out of pitch_launch()'s, the stage arrays under the model's names"""
    r0, n = int(offs[u]), int(rows[u])
    got = dict(pitch=out["pitch"][r0:r0 + n], grp=out["grp"][r0:r0 + n], pratio=out["pratio"][r0:r0 + n], status=int(out["status"][u]))
    if out["stages"] is not None:
        block = out["stages"][r0 * WORDS:(r0 + n) * WORDS]
        for k, name in enumerate(PM.PITCH_STAGES):
            got[name] = block[k * n:(k + 1) * n]
        grp = block[5 * n:].view(np.float32).reshape(2, n, NCH)
        for k, name in enumerate(PM.GRP_STAGES):
            got[name] = grp[k]
    return got


def assert_equal(got, want, what, names=NAMES):
    assert got["status"] == want["status"], f"{what}: status {got['status']:#x}, expected {want['status']:#x}"
    for name in names:
        assert M.same_bits(np.ascontiguousarray(got[name]), want[name]), f"{what}: {name}"


def assert_guards(out, total, n_utt):
    assert (out["pitch"][total:] == SENT_I).all() and (out["status"][n_utt:] == SENT_I).all()
    assert (out["grp"][total:] == SENT).all() and (out["pratio"][total:] == SENT).all()
    assert not (out["pitch"][:total] == SENT_I).any() and not (out["status"][:n_utt] == SENT_I).any()
    assert not (out["grp"][:total] == SENT).any() and not (out["pratio"][:total] == SENT).any()
    if out["stages"] is not None:
        assert (out["stages"][total * WORDS:] == SENT_I).all() and not (out["stages"][:total * WORDS] == SENT_I).any()


# ---- the audio batch -----------------------------------------------------------------------------------------------------------
PERM = [4, 8, 0, 6, 2, 7, 1, 5, 3]


def extra_inputs():
    """the inputs of the audio batch that the fixture does not hold (the models judge them): s (no segment), no frame, three
    frames, five frames; also what tools/hw_oracle_coverage.py feeds the reference as part of `hw-tests`"""
    xs = PM.audio_inputs()
    n = np.arange(240)
    return [xs["s"], (40 * np.sin(2 * np.pi * 200 * n[:79] / 8000)).astype(np.float32),
            (3000 * np.sin(2 * np.pi * 125 * n / 8000) + 1500 * np.sin(2 * np.pi * 250 * n / 8000)).astype(np.float32),
            xs["p"][2000:2400].copy()]


@pytest.fixture(scope="module")
def audio():
    """the batch, its front half on the GPU (computed once, never changed) and what every utterance must give"""
    import torch
    import speech_enhancement_amd as sea
    g = PM.load_golden()
    xs = PM.audio_inputs()
    t = M.tables()
    utts = [g[f"x_{k}"] for k in PM.AUDIO_CASES]
    want = [_from_golden(g, k) for k in PM.AUDIO_CASES]
    extra = extra_inputs()
    for x in extra:
        fr = M.frontend(x, t)
        want.append(PM.pitch_stage(fr["acf_hc"], fr["pRatio"], fr["mark"], fr["cross_hc"]))
    utts += extra
    assert [len(x) // 80 for x in utts] == [150, 150, 175, 125, 125, 100, 0, 3, 5]
    assert want[5]["status"] == 0 and want[6]["status"] == 0
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    front = sea.hw25_frontend_batch(batch, want_acf=True)
    torch.cuda.synchronize()
    rows = np.asarray(front.host_rows)
    inp = dict(acf=front.acf_hc, cross=front.cross_hc, pratio=front.pratio, mark=front.mark, lengths=batch.lengths,
               row_offsets=front.row_offsets)
    before = {k: inp[k].clone() for k in ("acf", "cross", "pratio", "mark")}
    runs = {"plain": pitch_launch(inp, rows), "nostages": pitch_launch(inp, rows, stages=False),
            "permuted": pitch_launch(inp, rows, order=torch.tensor(PERM, dtype=torch.int32, device="cuda:0"))}
    return dict(g=g, utts=utts, want=want, batch=batch, front=front, rows=rows, offs=np.asarray(front.host_row_offsets), inp=inp,
                before=before, runs=runs)


def test_front_half_acf_is_the_references(audio):
    for u, k in enumerate(PM.AUDIO_CASES):
        got = audio["front"].utterance(u)["acf_hc"]
        assert PM.crc32(got) == int(audio["g"][f"acfcrc_{k}"]), f"{k}: the FRONT half's ACF differs from the reference's"


@pytest.mark.parametrize("run", ["plain", "permuted"])
def test_every_output_and_stage_equals_the_reference_or_the_model(audio, run):
    out = audio["runs"][run]
    for u, want in enumerate(audio["want"]):
        assert_equal(utterance(out, audio["offs"], audio["rows"], u), want, f"{run}, utterance {u}")
    assert_guards(out, int(audio["rows"].sum()), len(audio["utts"]))
    pitch = np.concatenate([w["pitch"] for w in audio["want"]])
    assert (pitch > 0).sum() > 100 and sum((w["grp"] > 0).sum() for w in audio["want"]) > 300


def test_null_stages_gives_the_same_outputs(audio):
    a, b = audio["runs"]["plain"], audio["runs"]["nostages"]
    assert b["stages"] is None
    for name in ("pitch", "grp", "pratio", "status"):
        assert M.same_bits(a[name], b[name]), name
    assert_guards(b, int(audio["rows"].sum()), len(audio["utts"]))


def test_inputs_are_unchanged(audio):
    import torch
    for k, v in audio["before"].items():
        assert torch.equal(audio["inp"][k].view(torch.int32), v.view(torch.int32)), k


def test_python_layer_and_single_utterance_form(audio):
    import speech_enhancement_amd as sea
    res = sea.hw25_pitch_batch(audio["batch"], stages=True)
    for u, want in enumerate(audio["want"]):
        assert_equal(res.utterance(u), want, f"hw25_pitch_batch, utterance {u}")
    res = sea.hw25_pitch_batch(audio["batch"], use_order=False)
    assert res.stages is None
    for u in (0, 5, 6, 8):
        assert_equal(res.utterance(u), audio["want"][u], f"hw25_pitch_batch without stages, utterance {u}", ("pitch", "grp", "pratio"))
    for u in (3, 6, 7, 8):
        assert_equal(sea.hw25_pitch(audio["utts"][u]), audio["want"][u], f"hw25_pitch, utterance {u}", ("pitch", "grp", "pratio"))


# ---- hand-made arrays straight into sea_hw25_pitch_batch ---------------------------------------------------------------------
def _device_inputs(cases):
    """acf / pratio / mark / cross tuples -> the device tensors of one batch and the row counts"""
    import torch
    rows = np.array([c[0].shape[0] for c in cases], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    acf, pratio, mark, cross = (np.concatenate([c[k] for c in cases]) for k in range(4))
    inp = dict(acf=dev(acf), cross=dev(cross), pratio=dev(pratio), mark=dev(mark), lengths=dev(rows * 80 + 7), row_offsets=dev(offs))
    return inp, rows, offs


def test_handmade_arrays():
    """The fixture's hand-made cases against the reference's arrays -- h (the only input that reaches `number == 0` in both
    Developes), v (a frame that loses findPitch's vote outside the frames that keep their pitch: lFrame comes from before the
    vote, so leftDevelope reaches it) and x (a cross value that decides a bit through number2's forty-channel loop) --, then
    more than 400 segments and no streak of three frames (chan_mark read before it is computed) against the model with their
    status bits."""
    g = PM.load_golden()
    zero = lambda c: c + (np.zeros_like(c[1]),)
    cases = [PM.hand_inputs(k) for k in ("h", "v", "x")] + [zero(PM.many_segments_case()), zero(PM.no_streak_case())]
    want = [_from_golden(g, k) for k in ("h", "v", "x")] + [PM.pitch_stage(*c) for c in cases[3:]]
    assert want[0]["status"] == 4 and want[3]["status"] == (442 | PM.TOO_MANY_SEGMENTS)
    assert want[4]["status"] == (1 | PM.CHANMARK_UNSET)
    assert want[1]["pitch_find2"][3] == 0 and want[1]["pitch"][3] == 40 and want[2]["pitch"][5] == 20
    inp, rows, offs = _device_inputs(cases)
    out = pitch_launch(inp, rows)
    for u, w in enumerate(want):
        assert_equal(utterance(out, offs, rows, u), w, f"hand-made {u}")
    assert_guards(out, int(rows.sum()), len(cases))


def test_an_output_that_is_an_input_is_refused():
    _, lib = _lib()
    inp, rows, _ = _device_inputs([PM.hand_inputs("v")])
    import torch
    o = {k: torch.zeros(16 * 25 + 8, dtype=torch.float32, device="cuda:0") for k in ("grp", "pratio")}
    o["pitch"] = torch.zeros(32, dtype=torch.int32, device="cuda:0")
    scratch = torch.empty(int(lib.sea_hw25_pitch_scratch_bytes(16, 1)), dtype=torch.uint8, device="cuda:0")
    for grp, pratio in ((inp["mark"], o["pratio"]), (o["grp"], inp["pratio"]), (inp["cross"], o["pratio"]), (o["grp"], o["grp"])):
        rc = lib.sea_hw25_pitch_batch(_ptr(inp["acf"]), _ptr(inp["cross"]), _ptr(inp["pratio"]), _ptr(inp["mark"]), _ptr(inp["lengths"]),
                                      _ptr(inp["row_offsets"]), _ptr(o["pitch"]), _ptr(grp), _ptr(pratio), _ptr(o["pitch"][20:]),
                                      None, _ptr(scratch), None, 1, _stream())
        assert rc != 0
    torch.cuda.synchronize()


def launch_constants():
    """the waves-per-utterance formula of the frame kernels, read out of the launch code: (multiplier of n_cu, upper clamp)"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech_enhancement_amd", "csrc")
    rule, text = open(os.path.join(path, "capi.hip")).read(), open(os.path.join(path, "hw_bank_capi.hip")).read()
    per_cu = re.findall(r"int per_utt = \((\d+) \* c->n_cu \+ n_utt - 1\) / n_utt;", rule)
    clamp = re.findall(r"per_utt = per_utt < 1 \? 1 : \(per_utt > (\d+) \? (\d+) : per_utt\);", rule)
    assert len(per_cu) == 1 and len(clamp) == 1 and clamp[0][0] == clamp[0][1], "the launch code's grid formula was reworded"
    assert text.count("const int waves = per_utterance(n_utt);") == 1, "the frame launches left the formula"
    assert text.count("per_frame, block") == 4 and text.count("per_frame(n_utt, waves)") == 1, "a frame launch left the formula"
    return int(per_cu[0]), int(clamp[0][0])


def test_grid_stride_loops_reach_their_third_trip(audio):
    """The frame kernels (hw25_pitch_max_kernel, hw25_pitch_frame_kernel) run on a grid (n_utt, G), G = ceil (K n_cu / n_utt)
    clamped to 1..C, and wave (u, g) takes the frames g, g + G, ... of utterance u: they are the new launch code's only
    grid-stride loops.  K and C are read out of capi.hip's per_utterance (8 and 1024).  With n_utt = K n_cu + 52 utterances G is 1
    (256 CUs: ceil (2048 / 2100) = 1), so every wave walks all 5 rows of its utterance: 5 trips.  The utterances are five-row
    cut-outs of the audio batch's front half (about 106 MB of ACF), expected values from the model on the same arrays."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_cu, clamp = launch_constants()
    n_utt = per_cu * n_cu + 52
    waves = min(max((per_cu * n_cu + n_utt - 1) // n_utt, 1), clamp)
    assert waves == 1 and -(-5 // waves) >= 3
    host = {k: audio["before"][k].cpu().numpy() for k in ("acf", "cross", "pratio", "mark")}
    starts = []
    for u in range(5):
        r0, n = int(audio["offs"][u]), int(audio["rows"][u])
        starts += list(range(r0, r0 + n - 4, 3))
    assert len(starts) > 200
    wants = {}
    for s in starts:
        wants[s] = PM.pitch_stage(host["acf"][s:s + 5], host["pratio"][s:s + 5], host["mark"][s:s + 5], host["cross"][s:s + 5])
    assert sum(w["status"] > 0 for w in wants.values()) > 50 and sum(w["pitch"].any() for w in wants.values()) > 20
    pick = [starts[i % len(starts)] for i in range(n_utt)]
    idx = torch.from_numpy((np.asarray(pick)[:, None] + np.arange(5)[None, :]).ravel()).to("cuda:0")
    inp = {k: audio["before"][k][idx].contiguous() for k in ("acf", "cross", "pratio", "mark")}
    rows = np.full(n_utt, 5, np.int64)
    offs = np.arange(n_utt, dtype=np.int64) * 5
    inp["lengths"] = torch.full((n_utt,), 400, dtype=torch.int64, device="cuda:0")
    inp["row_offsets"] = torch.from_numpy(offs).to("cuda:0")
    out = pitch_launch(inp, rows)
    assert_guards(out, 5 * n_utt, n_utt)
    for u in range(n_utt):
        assert_equal(utterance(out, offs, rows, u), wants[pick[u]], f"utterance {u} (rows from {pick[u]})")


# ---- the edge set ------------------------------------------------------------------------------------------------------------
def test_edge_set_audio_and_handmade_arrays():
    """The edge set (tests/test_hw_edge_coverage_cpu.py) against tests/golden/hw25_edge_golden.npz, every output and stage bit
    for bit.  Audio: ewhole (voiced up to the last frame) and edc (whole ACF rows exactly 0, pRatio 0 / 0; where the reference
    finds no segment in it the fixture holds nothing and the model judges) in one batch after the fixture's m9, through the
    front half on the GPU, in plain and permuted order and with null d_stages.  Hand-made: egrid (a segment against frame 0,
    the last frame and the top channel), ecrn (pitchCrn decided by its last test) and erclamp / elclamp (the Developes' search bound
    clamped at MIN_DELAY, where it decides Pitch) in one batch after the fixture's v."""
    import torch
    import speech_enhancement_amd as sea
    from tests import hw_edge as E
    e, g = E.load("hw25"), PM.load_golden()
    utts = [g["x_m9"], e["x_ewhole"], e["x_edc"]]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    front = sea.hw25_frontend_batch(batch, want_acf=True)
    torch.cuda.synchronize()
    rows, offs = np.asarray(front.host_rows), np.asarray(front.host_row_offsets)
    inp = dict(acf=front.acf_hc, cross=front.cross_hc, pratio=front.pratio, mark=front.mark, lengths=batch.lengths,
               row_offsets=front.row_offsets)
    for u, k in ((1, "ewhole"), (2, "edc")):
        assert PM.crc32(front.utterance(u)["acf_hc"]) == int(e[f"front_acf_hc_crc_{k}"]), f"{k}: the FRONT half's ACF differs"
    want = [_from_golden(g, "m9"), E.pitch_want(e, "ewhole", PM.PITCH_STAGES, PM.GRP_STAGES)]
    if "nseg_edc" in e:
        want.append(E.pitch_want(e, "edc", PM.PITCH_STAGES, PM.GRP_STAGES))
    else:
        fr = {k: inp[k].cpu().numpy()[int(offs[2]):int(offs[2] + rows[2])] for k in ("acf", "pratio", "mark", "cross")}
        want.append(PM.pitch_stage(fr["acf"], fr["pratio"], fr["mark"], fr["cross"]))
        assert want[2]["status"] == 0
    assert (want[1]["pitch"] > 0).sum() >= 25 and want[1]["pitch"][-1] > 0 and (want[1]["grp"] > 0).sum() > 100
    runs = {"plain": pitch_launch(inp, rows), "nostages": pitch_launch(inp, rows, stages=False),
            "permuted": pitch_launch(inp, rows, order=torch.tensor([1, 2, 0], dtype=torch.int32, device="cuda:0"))}
    for run, out in runs.items():
        tally = E.Tally(f"hw25 pitch stage, edge audio, {run}")
        for u, w in enumerate(want):
            E.add_pitch(tally, utterance(out, offs, rows, u), w, NAMES if out["stages"] is not None else ("pitch", "grp", "pratio"),
                        f"utterance {u}")
        tally.done()
        assert_guards(out, int(rows.sum()), len(utts))
    hand = ("egrid", "ecrn", "erclamp", "elclamp")
    cases = [PM.hand_inputs("v")] + [PM.hand_inputs(k) for k in hand]
    want = [_from_golden(g, "v")] + [E.pitch_want(e, k, PM.PITCH_STAGES, PM.GRP_STAGES) for k in hand]
    assert want[1]["grp"][0].any() and want[1]["grp"][-1].any() and want[1]["grp"][:, NCH - 1].any()
    assert (want[2]["pitch"] > 0).any() and (want[3]["pitch"] > 0).any() and want[3]["pitch"][12] == 0 and want[4]["pitch"][3] == 0
    assert all((w["grp"] > 0).any() for w in want[1:])    # no - unit: none of these inputs is meant to give one
    inp, rows, offs = _device_inputs(cases)
    for run, kw in (("plain", {}), ("permuted", dict(order=torch.tensor([3, 1, 4, 0, 2], dtype=torch.int32, device="cuda:0"))),
                    ("nostages", dict(stages=False))):
        out = pitch_launch(inp, rows, **kw)
        tally = E.Tally(f"hw25 pitch stage, edge hand-made arrays, {run}")
        for u, w in enumerate(want):
            E.add_pitch(tally, utterance(out, offs, rows, u), w, NAMES if out["stages"] is not None else ("pitch", "grp", "pratio"),
                        f"hand-made {u}")
        tally.done()
        assert_guards(out, int(rows.sum()), len(cases))
