"""Round 13 took address and operand set-up off the steady beats of the six-wave NoiseSup kernels (ns_pipe6_kernel.hip, sea_device.h,
ns_core.h): FA's steady copies get the onset and their pair counter through v_readfirstlane, so ticks, ring slots and the next frame's
address are scalar; the twiddled butterfly's four output additions read the halves of their operand pairs through the instruction's
op_sel / neg fields; FB's neighbour fetches take no zero `old` operand and repair their two wrap lanes with v_writelane.  Same operations
on the same operands in the same order, so forms 6 (dense) and 3 (plain) and the frame-dropping kernel must equal the CPU oracle exactly:
int16 audio against etsi_denoise, index of the first output frame, float stream bit for bit, untouched tail.

What can go wrong, and the smallest shapes that show it:
  a wrong onset or counter in FA's steady copies puts a frame into the wrong slot of the 8- or 16-slot ring, or loads the wrong frame --
    full frames per utterance 0, 1, 2 (no steady range), 11 .. 17 (the range is empty, one pair, begins and ends on even and odd beats:
    FA's begins 8 beats behind the onset and ends one before the last frame), 24, 25, 40, 41 (every slot of both rings several times)
    and 130, behind 0, 1, 2, 3, 5 and 9 leading all-zero frames (onset parity, ring phase), with tails of 0, 1 and 79 samples;
  a wrong half or sign in the butterfly's output additions changes every spectrum -- speech-like noise; a single impulse (every bin
    equal); a full-scale square wave that reaches -32768 (the largest PSDs int16 input allows);
  a wrong wrap lane in FB's PSD changes the PSD values made of slot 31: bins 0 and 64 of the 65 -- a constant (all energy in bin 0)
    and an alternating +-A signal (all of it at the Nyquist frequency, PSD bin 64).
One batch of 304 utterances (more than CUs: launch order, priority rule, two launch rows) and one of seven (neither)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 2, 11, 12, 13, 14, 15, 16, 17, 24, 25, 40, 41, 130)
LEADS = (0, 1, 2, 3, 5, 9)
TAILS = (0, 1, 79)
SPECIAL_FRAMES = (13, 16, 25, 41, 130)
SPECIAL_LEADS = (0, 1, 2)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _constant(n):
    return np.full(n, 12345, np.int16)


def _alternating(n):
    return np.where(np.arange(n) % 2 == 0, 20001, -20001).astype(np.int16)


def _impulse(n):
    x = np.zeros(n, np.int16)
    if n:
        x[min(n - 1, 37)] = 30000
    return x


def _square_min(n):
    """full-scale square wave, 7 samples per half cycle, whose negative half is -32768"""
    return np.where((np.arange(n) // 7) % 2 == 0, 32767, -32768).astype(np.int16)


CONTENT = (_constant, _alternating, _impulse, _square_min)


def _distinct():
    """152 utterances: every (frames, lead) with speech-like noise, the four special signals on a sub-grid, an empty and an all-zero one"""
    utts = []
    for frames in FRAMES:
        for lead in LEADS:
            tail = TAILS[len(utts) % 3]
            sig = _speech(13000 + 16 * frames + lead, 80 * frames + tail)
            utts.append(np.concatenate([np.zeros(80 * lead, np.int16), sig]))
    for make in CONTENT:
        for frames in SPECIAL_FRAMES:
            for lead in SPECIAL_LEADS:
                tail = TAILS[(len(utts) + lead) % 3]
                utts.append(np.concatenate([np.zeros(80 * lead, np.int16), make(80 * frames + tail)]))
    utts.append(np.zeros(80 * 40 + 1, np.int16))  # all zero: the gate never opens
    utts.append(np.zeros(0, np.int16))            # empty
    assert len(utts) == len(FRAMES) * len(LEADS) + len(CONTENT) * len(SPECIAL_FRAMES) * len(SPECIAL_LEADS) + 2 == 152
    return utts


@pytest.fixture(scope="module")
def off_corpus():
    return _distinct()


@pytest.fixture(scope="module")
def off_want(oracle, off_corpus):
    """Per distinct utterance, computed once and only read: etsi_denoise's audio, and the oracle's trace for the float stream and the
    number of output frames (first output frame = frames - that number)."""
    want = []
    for x in off_corpus:
        tr = oracle.ns_trace(x, want_state=False)
        audio = oracle.etsi_denoise(x)
        assert np.array_equal(audio, tr["out_i16"])  # the two oracle entry points agree; what is compared below is etsi_denoise's
        want.append(dict(audio=audio, den_f32=tr["den_f32"], nout=tr["nout"]))
    return want


def _check(got, gotf, first_h, utts, want, what):
    for u, (x, w) in enumerate(zip(utts, want)):
        nfr = len(x) // 80
        assert np.array_equal(got[u][: nfr * 80], w["audio"][: nfr * 80]), f"{what}, utterance {u} (L={len(x)}): audio"
        assert not np.any(got[u][nfr * 80:]), f"{what}, utterance {u}: the tail beyond the last whole frame was written"
        assert int(first_h[u]) == (nfr - w["nout"] if w["nout"] else -1), f"{what}, utterance {u}: first output"
        if w["nout"]:
            f0 = nfr - w["nout"]
            assert np.array_equal(gotf[u][f0 * 80: nfr * 80].view(np.uint32), w["den_f32"].view(np.uint32)), \
                f"{what}, utterance {u}: float stream"


def _forced(sea, torch, utts, want, what):
    lib = sea.load()
    batch = sea.PackedBatch.from_arrays(utts)
    prev = lib.sea_ns_kernel_form(0)
    try:
        for form in (6, 3):
            lib.sea_ns_kernel_form(form)
            out, f32, first = sea.ns_denoise_batch(batch, want_f32=True)
            torch.cuda.synchronize()
            _check(batch.split(out), batch.split(f32, full_frames_only=True), first.cpu().numpy(), utts, want, f"form {form}{what}")
    finally:
        lib.sea_ns_kernel_form(prev)


def _order_304(n):
    idx = list(range(n)) + [(7 * j + 3) % n for j in range(n)]
    assert len(idx) == 304 and sorted(idx[n:]) == list(range(n))
    return idx


def test_ns6_offstream_304_utterances_exact(off_corpus, off_want):
    """Forms 6 and 3 forced on 304 utterances: every distinct one twice, the second time in another order."""
    import speech_enhancement_amd as sea
    idx = _order_304(len(off_corpus))
    _forced(sea, _torch(), [off_corpus[u] for u in idx], [off_want[u] for u in idx], "")


def test_ns6_offstream_seven_utterances_exact(off_corpus, off_want):
    """The same two forms on seven utterances (fewer than CUs: no launch order, no priorities): 130 frames of each kind of signal behind
    its largest lead, and the 41- and 17-frame speech behind nine leading zero frames."""
    import speech_enhancement_amd as sea
    base = len(FRAMES) * len(LEADS)
    per = len(SPECIAL_FRAMES) * len(SPECIAL_LEADS)
    pick = [base - 1] + [base + k * per + per - 1 for k in range(len(CONTENT))] + [FRAMES.index(41) * len(LEADS) + 5, FRAMES.index(17) * len(LEADS) + 5]
    assert len(pick) == 7 and len(set(pick)) == 7
    _forced(sea, _torch(), [off_corpus[u] for u in pick], [off_want[u] for u in pick], ", seven utterances")


def test_ns6_offstream_frame_dropping_kernel_exact(oracle, off_corpus, off_want):
    """The frame-dropping six-wave kernel is afe_features_batch's NoiseSup launch: the same 304 utterances.  NoiseSup's outputs exactly as
    above; the feature rows' count and VAD flags (the speech bits that kernel leaves per frame) exactly, the cepstra to the tolerance
    smoke() holds them to."""
    import speech_enhancement_amd as sea
    torch = _torch()
    idx = _order_304(len(off_corpus))
    utts, want = [off_corpus[u] for u in idx], [off_want[u] for u in idx]
    batch = sea.PackedBatch.from_arrays(utts, device="cuda:0")
    res = sea.afe_features_batch(batch, want_intermediates=True)
    torch.cuda.synchronize()
    _check(batch.split(res["out"]), batch.split(res["den_f32"], full_frames_only=True), res["first_out"].cpu().numpy(), utts, want,
           "frame-dropping kernel")
    feats = {}
    for k, u in enumerate(idx):
        if u not in feats:
            feats[u] = oracle.afe_trace(off_corpus[u])["vad_out"]
        w, f15 = feats[u], res["feats"][k]
        assert f15.shape == w.shape and np.array_equal(f15[:, 14], w[:, 14]), f"utterance {k}: feature rows / VAD flags"
        if len(w):
            assert np.abs(f15[:, :14] - w[:, :14]).max() <= 1e-3, f"utterance {k}: cepstra"
