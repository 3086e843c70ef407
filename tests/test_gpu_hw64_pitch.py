"""The Hu-Wang initial grouping and pitch tracking at 16 kHz on the 64-channel bank on the GPU (csrc/hw64_pitch_kernel.hip)
against what the reference's own initGroup / pitchDtm produced when compiled against the 64-band header (tests/golden/
hw64_pitch_golden.npz) and, where the fixture holds nothing, the numpy model that the CPU tests pin to that fixture
(tests/hw64_pitch_model.py).  Every output and every stage array is compared bit for bit.

The audio batch, through sea_hw64_frontend_batch and then sea_hw64_pitch_batch: the fixture's five inputs; s (white noise); 159
samples (no row); 320 samples (2 rows); 480 samples (3 rows); p[4000:4800] (5 rows).  For the five that the fixture does not
hold the expected values are the model's on the front half's arrays as the GPU computed them (the front-half model takes ten
seconds per input; tests/test_gpu_hw64.py is what pins the front half).  Every output buffer is filled with a sentinel and
carries guard rows.  A second batch feeds hand-made arrays straight to sea_hw64_pitch_batch."""
import ctypes

import numpy as np
import pytest

from tests import hw25_model as M
from tests import hw64_pitch_model as PM

pytestmark = pytest.mark.gpu

NCH, NDEL, HOP, WORDS = PM.NCH, PM.NDEL, PM.HOP, PM.STAGE_WORDS
SENT, SENT_I = -7777.25, -77
GUARD = 3
NAMES = ("pitch", "grp", "pratio") + PM.PITCH_STAGES + PM.GRP_STAGES
ROW_BYTES = 4 * NCH * NDEL


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


def _call(lib, inp, o, scratch, order, n_utt):
    return lib.sea_hw64_pitch_batch(_ptr(inp["acf"]), _ptr(inp["pratio"]), _ptr(inp["mark"]), _ptr(inp["lengths"]),
                                    _ptr(inp["row_offsets"]), _ptr(o["pitch"]), _ptr(o["grp"]), _ptr(o["pratio"]), _ptr(o["status"]),
                                    _ptr(o["stages"]), _ptr(scratch), _ptr(order), n_utt, _stream())


def pitch_launch(inp, rows, order=None, stages=True):
    """sea_hw64_pitch_batch on sentinel-filled outputs with guard rows.  inp: device tensors acf, pratio, mark and lengths /
    row_offsets (int64); rows: host row counts.  Returns numpy arrays per output."""
    import torch
    lib_mod, lib = _lib()
    dev = inp["acf"].device
    n_utt, total = len(rows), int(np.sum(rows))

    def full(shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=dev)

    o = dict(pitch=full((total + GUARD,), SENT_I, torch.int32), grp=full((total + GUARD, NCH), SENT, torch.float32),
             pratio=full((total + GUARD, NCH), SENT, torch.float32), status=full((n_utt + GUARD,), SENT_I, torch.int32),
             stages=full(((total + GUARD) * WORDS,), SENT_I, torch.int32) if stages else None)
    nbytes = int(lib.sea_hw64_pitch_scratch_bytes(total, n_utt))
    assert nbytes == 4 * (n_utt * 800 + total * 193)
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    lib_mod.check(_call(lib, inp, o, scratch, order, n_utt), "sea_hw64_pitch_batch")
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
PERM = [4, 8, 0, 6, 2, 9, 7, 1, 5, 3]
NGOLD = len(PM.AUDIO_CASES)


def extra_inputs():
    """the inputs of the audio batch that the fixture does not hold (the model judges them): s, no frame, two, three and five
    frames; also what tools/hw_oracle_coverage.py feeds the reference as part of `hw-tests`"""
    xs = PM.audio_inputs()
    n = np.arange(480)
    tone = (3000 * np.sin(2 * np.pi * 125 * n / 16000) + 1500 * np.sin(2 * np.pi * 250 * n / 16000)).astype(np.float32)
    return [xs["s"], tone[:159].copy(), tone[:320].copy(), tone, xs["p"][4000:4800].copy()]


@pytest.fixture(scope="module")
def audio():
    """the batch, its front half on the GPU (computed once, never changed) and what every utterance must give"""
    import torch
    import speech_enhancement_amd as sea
    g = PM.load_golden()
    xs = PM.audio_inputs()
    utts = [g[f"x_{k}"] for k in PM.AUDIO_CASES]
    utts += extra_inputs()
    assert [len(x) // HOP for x in utts] == [75, 75, 87, 62, 62, 50, 0, 2, 3, 5]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    front = sea.hw64_frontend_batch(batch, want_acf=True)
    torch.cuda.synchronize()
    rows, offs = np.asarray(front.host_rows), np.asarray(front.host_row_offsets)
    inp = dict(acf=front.acf_hc, pratio=front.pratio, mark=front.mark, lengths=batch.lengths, row_offsets=front.row_offsets)
    before = {k: inp[k].clone() for k in ("acf", "pratio", "mark")}
    host = {k: before[k].cpu().numpy() for k in before}
    want = [_from_golden(g, k) for k in PM.AUDIO_CASES]
    for u in range(NGOLD, len(utts)):
        r0, r1 = int(offs[u]), int(offs[u] + rows[u])
        want.append(PM.pitch_stage(host["acf"][r0:r1], host["pratio"][r0:r1], host["mark"][r0:r1]))
    assert want[6]["status"] == 0 and want[7]["status"] == 0
    runs = {"plain": pitch_launch(inp, rows), "nostages": pitch_launch(inp, rows, stages=False),
            "permuted": pitch_launch(inp, rows, order=torch.tensor(PERM, dtype=torch.int32, device="cuda:0"))}
    return dict(g=g, utts=utts, want=want, batch=batch, front=front, rows=rows, offs=offs, inp=inp, before=before, host=host, runs=runs)


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
    assert sum((w["grp"][:, 40:] > 0).sum() for w in audio["want"][:NGOLD]) > 100


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
    res = sea.hw64_pitch_batch(audio["batch"], stages=True)
    assert isinstance(res, sea.Hw64PitchResult) and isinstance(res.front, sea.Hw64Result)
    for u, want in enumerate(audio["want"]):
        assert_equal(res.utterance(u), want, f"hw64_pitch_batch, utterance {u}")
    res = sea.hw64_pitch_batch(audio["batch"], use_order=False)
    assert res.stages is None
    for u in (0, 5, 6, 9):
        assert_equal(res.utterance(u), audio["want"][u], f"hw64_pitch_batch without stages, utterance {u}", ("pitch", "grp", "pratio"))
    for u in (3, 6, 7, 8, 9):
        got = sea.hw64_pitch(audio["utts"][u])
        assert got["grp"].shape == (len(audio["utts"][u]) // HOP, NCH)
        assert_equal(got, audio["want"][u], f"hw64_pitch, utterance {u}", ("pitch", "grp", "pratio"))


# ---- hand-made arrays straight into sea_hw64_pitch_batch ---------------------------------------------------------------------
def _device_inputs(cases):
    """acf / pratio / mark tuples -> the device tensors of one batch, the row counts and the row offsets"""
    import torch
    rows = np.array([c[0].shape[0] for c in cases], np.int64)
    offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    acf, pratio, mark = (np.concatenate([c[k] for c in cases]) for k in range(3))
    inp = dict(acf=dev(acf), pratio=dev(pratio), mark=dev(mark), lengths=dev(rows * HOP + 7), row_offsets=dev(offs))
    return inp, rows, offs


def _flat(rows, marked=True):
    acf = np.full((rows, NCH, NDEL), 100, np.float32)
    acf[:, :, 90] = 700
    return acf, np.full((rows, NCH), 0.99, np.float32), np.full((rows, NCH), 1 if marked else 0, np.float32)


def test_handmade_arrays():
    """The fixture's hand-made cases against the reference's arrays -- h (`number == 0` in both Developes), v (lFrame from before
    findPitch's vote) and ml, nl, mr, nr, where units in channels 40..63 would change Pitch if the Developes' chan_mark or
    number2 ran over 64 channels instead of the reference's 40 --, then the model-only cases with their status bits: more than
    400 segments, no streak of three frames (chan_mark read before it is computed), no segment, and 0, 2, 3 and 5 rows."""
    g = PM.load_golden()
    hand = ("h", "v", "ml", "nl", "mr", "nr")
    cases = [PM.hand_inputs(k) for k in hand] + [PM.many_segments_case(), PM.no_streak_case(), _flat(9, marked=False)]
    cases += [_flat(r) for r in (0, 2, 3, 5)]
    want = [_from_golden(g, k) for k in hand] + [PM.pitch_stage(*c) for c in cases[len(hand):]]
    assert want[0]["status"] == 4 and want[6]["status"] == (1088 | PM.TOO_MANY_SEGMENTS)
    assert want[7]["status"] == (1 | PM.CHANMARK_UNSET) and [w["status"] for w in want[8:]] == [0, 0, 0, 1, 1]
    assert want[1]["pitch_find2"][3] == 0 and want[1]["pitch"][3] == 40 and want[12]["pitch"].tolist() == [90] * 5
    for bound, (k, frame, at40, at64) in PM.SEPARATES.items():
        w = want[hand.index(k)]
        assert w["pitch"][frame] == at40 and PM.pitch_stage(*PM.hand_inputs(k), bounds={bound: 64})["pitch"][frame] == at64 != at40
    inp, rows, offs = _device_inputs(cases)
    before = {k: inp[k].clone() for k in ("acf", "pratio", "mark")}
    out = pitch_launch(inp, rows)
    for u, w in enumerate(want):
        assert_equal(utterance(out, offs, rows, u), w, f"hand-made {u}")
    assert_guards(out, int(rows.sum()), len(cases))
    import torch
    for k, v in before.items():
        assert torch.equal(inp[k].view(torch.int32), v.view(torch.int32)), k


def test_an_output_that_is_an_input_and_a_null_input_are_refused():
    import torch
    _, lib = _lib()
    inp, rows, _ = _device_inputs([PM.hand_inputs("v")])
    o = {k: torch.zeros(16 * NCH + 8, dtype=torch.float32, device="cuda:0") for k in ("grp", "pratio")}
    o.update(pitch=torch.zeros(32, dtype=torch.int32, device="cuda:0"), stages=None)
    o["status"] = o["pitch"][20:]
    scratch = torch.empty(int(lib.sea_hw64_pitch_scratch_bytes(16, 1)), dtype=torch.uint8, device="cuda:0")
    assert lib.sea_hw64_pitch_batch(*([None] * 12), 0, None) == 0
    for grp, pratio in ((inp["mark"], o["pratio"]), (o["grp"], inp["pratio"]), (inp["acf"], o["pratio"]), (o["grp"], o["grp"])):
        assert _call(lib, inp, dict(o, grp=grp, pratio=pratio), scratch, None, 1) != 0
        assert b"of its own" in lib.sea_last_error()
    for k in ("acf", "pratio", "mark", "lengths", "row_offsets"):
        assert _call(lib, dict(inp, **{k: None}), o, scratch, None, 1) != 0
        assert b"null" in lib.sea_last_error()
    assert _call(lib, inp, o, None, None, 1) != 0
    torch.cuda.synchronize()
    assert not o["grp"].any() and not o["pitch"].any()  # nothing was launched
    assert _call(lib, inp, o, scratch, None, 1) == 0  # the same buffers, each its own
    torch.cuda.synchronize()
    assert int(o["status"][0]) == 2


def test_grid_stride_loops_reach_their_third_trip(audio):
    """The frame kernels (hw64_pitch_max_kernel, hw64_pitch_frame_kernel) run on a grid (n_utt, G), and wave (u, g) takes the
    frames g, g + G, ... of utterance u: they are this launch code's only grid-stride loops.  G comes from the exported
    sea_hw64_pitch_waves_per_utterance.  The batch is the smallest number of five-row utterances for which G is at most 2
    (1024 on 256 CUs: wave 0 takes rows 0, 2 and 4, three trips), 51 456 B of ACF per row: 263 MB there.  The utterances are
    five-row cut-outs of the audio batch's front half, expected values from the model on the same arrays."""
    import torch
    import speech_enhancement_amd as sea
    n_utt = 1
    while sea.hw64_pitch_waves_per_utterance(n_utt) > 2:
        n_utt *= 2
    lo = n_utt // 2  # waves (lo) > 2 >= waves (n_utt): the smallest such count lies in (lo, n_utt]
    while n_utt - lo > 1:
        mid = (lo + n_utt) // 2
        lo, n_utt = (lo, mid) if sea.hw64_pitch_waves_per_utterance(mid) <= 2 else (mid, n_utt)
    waves = sea.hw64_pitch_waves_per_utterance(n_utt)
    assert 1 <= waves <= 2 and -(-5 // waves) >= 3
    assert n_utt * 5 * ROW_BYTES < 400 << 20, f"{n_utt} utterances: more ACF than this test may allocate"
    host = audio["host"]
    starts = []
    for u in range(NGOLD):
        r0, n = int(audio["offs"][u]), int(audio["rows"][u])
        starts += list(range(r0, r0 + n - 4, 3))
    assert len(starts) > 100
    wants = {s: PM.pitch_stage(host["acf"][s:s + 5], host["pratio"][s:s + 5], host["mark"][s:s + 5]) for s in starts}
    assert sum(w["status"] > 0 for w in wants.values()) > 30 and sum(bool(w["pitch"].any()) for w in wants.values()) > 10
    pick = [starts[i % len(starts)] for i in range(n_utt)]
    idx = torch.from_numpy((np.asarray(pick)[:, None] + np.arange(5)[None, :]).ravel()).to("cuda:0")
    inp = {k: audio["before"][k][idx].contiguous() for k in ("acf", "pratio", "mark")}
    rows = np.full(n_utt, 5, np.int64)
    offs = np.arange(n_utt, dtype=np.int64) * 5
    inp["lengths"] = torch.full((n_utt,), 5 * HOP, dtype=torch.int64, device="cuda:0")
    inp["row_offsets"] = torch.from_numpy(offs).to("cuda:0")
    out = pitch_launch(inp, rows)
    assert_guards(out, 5 * n_utt, n_utt)
    for u in range(n_utt):
        assert_equal(utterance(out, offs, rows, u), wants[pick[u]], f"utterance {u} (rows from {pick[u]})")


# ---- the edge set ------------------------------------------------------------------------------------------------------------
def test_edge_set_audio_and_handmade_arrays():
    """The edge set (tests/test_hw_edge_coverage_cpu.py) against tests/golden/hw64_edge_golden.npz, every output and stage bit
    for bit.  Audio: ewhole (voiced up to the last frame) and edc (whole ACF rows exactly 0, pRatio 0 / 0; where the reference
    finds no segment in it the fixture holds nothing and the model judges) in one batch after the fixture's m9, through the
    front half on the GPU, in plain and permuted order and with null d_stages.  Hand-made: egrid (a segment against frame 0,
    the last frame and the top channel), ecrn (pitchCrn decided by its last test) and erclamp / elclamp (the Developes' search bound
    clamped at MIN_DELAY, where it decides Pitch) in one batch after the fixture's v."""
    import torch
    import speech_enhancement_amd as sea
    from tests import hw_edge as E
    e, g = E.load("hw64"), PM.load_golden()
    utts = [g["x_m9"], e["x_ewhole"], e["x_edc"]]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0", dtype=np.float32)
    front = sea.hw64_frontend_batch(batch, want_acf=True)
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
        want.append(PM.pitch_stage(fr["acf"], fr["pratio"], fr["mark"]))
        assert want[2]["status"] == 0
    assert (want[1]["pitch"] > 0).sum() >= 25 and want[1]["pitch"][-1] > 0 and (want[1]["grp"] > 0).sum() > 100
    runs = {"plain": pitch_launch(inp, rows), "nostages": pitch_launch(inp, rows, stages=False),
            "permuted": pitch_launch(inp, rows, order=torch.tensor([1, 2, 0], dtype=torch.int32, device="cuda:0"))}
    for run, out in runs.items():
        tally = E.Tally(f"hw64 pitch stage, edge audio, {run}")
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
        tally = E.Tally(f"hw64 pitch stage, edge hand-made arrays, {run}")
        for u, w in enumerate(want):
            E.add_pitch(tally, utterance(out, offs, rows, u), w, NAMES if out["stages"] is not None else ("pitch", "grp", "pratio"),
                        f"hand-made {u}")
        tally.done()
        assert_guards(out, int(rows.sum()), len(cases))
