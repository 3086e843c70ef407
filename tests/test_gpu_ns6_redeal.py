"""The dense six-wave NoiseSup kernel deals three pieces of feed-forward work to other waves than the plain six-wave kernel does
(ns_pipe6_kernel.hip, REDEAL): N1 takes the VAD's log-energy one beat after S left the frame's sum of squares, FA runs the stage-0
17-tap filter of frame i-3 from the IDCT sums B0 left, in the beat in which it windows that frame's stage-1 input, and G1 keeps its
taps and filter outputs in registers.  Same operations in the same order, so forms 6 (dense) and 3 (plain) must both equal the CPU
oracle exactly: int16 audio, float stream bit for bit, index of the first output frame, untouched tail.

The corpus is sized for where the moved pieces can go wrong: signal lengths 1 .. 40 frames cover ticks 3 and 4 (stage 0 filters,
stage 1 does not yet) and the drain (FA filters frames nfr-3 .. nfr-1 without a frame of its own); 13 .. 16 leading zero frames
put those on the mirrored slots 0..2 of the second trip round the 16-slot stage-1 ring; the gated and the +-1 utterances move
flagVAD, hangOver and the nbFrame < 100 boundary, which the log-energy feeds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3, 13, 14, 15, 16)
MAX_SIGNAL = 40


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _gated(seed, frames, on=40, off=40):
    """speech of the corpus, `on` frames kept and `off` frames zeroed in turn"""
    x = _speech(seed, 80 * frames).copy()
    for f in range(0, frames, on + off):
        x[80 * (f + on): 80 * (f + on + off)] = 0
    return x


def _corpus():
    """More than 256 and at most 512 utterances: the launch orders them longest first and the waves set their priority by remaining
    frames."""
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in range(1, MAX_SIGNAL + 1):
            ragged = (len(utts) % 3 == 0) * (3 + (lead + n) % 70)
            utts.append(np.concatenate([z(lead), _speech(3000 + 64 * lead + n, 80 * n + ragged)]))
    assert len(utts) == 320
    utts.append(np.zeros(0, np.int16))                           # empty
    utts.append(z(30))                                           # all zero: the gate never opens
    last = z(25)
    last[80 * 24 + 41] = -3                                      # the gate opens on the last frame
    utts.append(last)
    one = z(61)
    one[7] = 1                                                   # one sample, then 60 zero frames
    utts.append(one)
    utts.append(np.concatenate([_speech(3900, 80 * 30), z(20), _speech(3901, 80 * 30 + 17)]))
    utts.append(_gated(3902, 240))                               # the VAD state the log-energy feeds: on / off, past frame 100
    utts.append(np.concatenate([z(2), _gated(3903, 210, 40, 40), np.zeros(11, np.int16)]))
    utts.append(np.sign(_gated(3904, 220).astype(np.int32)).astype(np.int16))   # amplitude +-1
    for j, n in enumerate((300, 700, 1204)):                     # long ones: the priority levels differ across the launch
        utts.append(np.concatenate([z(j), _speech(3910 + j, 80 * n + 9 * j)]))
    assert 256 < len(utts) <= 512, len(utts)
    return utts


N_SWEEP = len(LEADS) * MAX_SIGNAL


@pytest.fixture(scope="module")
def redeal_corpus():
    return _corpus()


@pytest.fixture(scope="module")
def redeal_traces(oracle, redeal_corpus):
    """The oracle's trace of every utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in redeal_corpus]


def _check_ns(sea, torch, batch, utts, traces, what):
    out, f32, first = sea.ns_denoise_batch(batch, want_f32=True)
    torch.cuda.synchronize()
    got = batch.split(out)
    gotf = batch.split(f32, full_frames_only=True)
    first_h = first.cpu().numpy()
    for u, (x, tr) in enumerate(zip(utts, traces)):
        nfr = len(x) // 80
        assert np.array_equal(got[u][: nfr * 80], tr["out_i16"][: nfr * 80]), f"{what}, utterance {u} (L={len(x)})"
        assert not np.any(got[u][nfr * 80:]), f"{what}, utterance {u}: the tail beyond the last whole frame was written"
        assert int(first_h[u]) == (nfr - tr["nout"] if tr["nout"] else -1), f"{what}, utterance {u}: first output"
        if tr["nout"]:
            f0 = nfr - tr["nout"]
            assert np.array_equal(gotf[u][f0 * 80: nfr * 80].view(np.uint32), tr["den_f32"].view(np.uint32)), \
                f"{what}, utterance {u}: float stream"


def _forced(sea, torch, utts, traces, what):
    lib = sea.load()
    batch = sea.PackedBatch.from_arrays(utts)
    prev = lib.sea_ns_kernel_form(0)
    try:
        for form in (6, 3):
            lib.sea_ns_kernel_form(form)
            _check_ns(sea, torch, batch, utts, traces, f"form {form}{what}")
    finally:
        lib.sea_ns_kernel_form(prev)


def test_ns6_redeal_corpus_exact(redeal_corpus, redeal_traces):
    """Forms 6 (dense, re-dealt) and 3 (plain) forced on the whole corpus: launch order and priorities on."""
    import speech_enhancement_amd as sea
    _forced(sea, _torch(), redeal_corpus, redeal_traces, "")


def test_ns6_redeal_small_batch_without_priorities(redeal_corpus, redeal_traces):
    """The same two forms on fewer utterances than CUs (no priority rule, no launch order): 7 is prime to the 40 lengths per lead,
    so every lead keeps lengths of every residue and ragged ones, and the special utterances all stay."""
    import speech_enhancement_amd as sea
    n = len(redeal_corpus)
    pick = [u for u in range(n) if u % 7 in (0, 3, 5) or u >= N_SWEEP]
    assert len(pick) < 256
    _forced(sea, _torch(), [redeal_corpus[u] for u in pick], [redeal_traces[u] for u in pick], ", small batch")
