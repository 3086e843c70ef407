"""In the dense six-wave NoiseSup kernel the helper wave S adds up DoMelIDCT's sums of both stages (ns_pipe6_kernel.hip, IDCTS): B0 and G1
leave the 9 x 25 rounded products of the mel gains and the basis, S adds each row up in order in one of its idle lanes (from +0, the
reference's h[t] += W[f] * idct[t][f]), multiplies by the Hanning weight and leaves the nine taps; FA filters stage 0 one beat later
than before and G1 filters stage 1 two beats after it took the frame's gains, so the pipeline is twelve beats deep instead of nine.
Same operations on the same operands in the same order, so forms 6 (dense) and 3 (plain) must both equal the CPU oracle exactly: int16
audio, float stream bit for bit, index of the first output frame, untouched tail.

The corpus is sized for where the deeper pipeline can go wrong: signal lengths 1 .. 2 x 12 + 4 frames behind 0, 1, 2, 3 and 5 leading
zero frames cover the fill (the first taps of each stage, the first stage-1 window), the first trip round each ring and the drain, in
which G1 filters frames with no gains left to take and S adds up rows with no DC frame left; the empty and the all-zero utterance never
leave the general copies; in the gated utterances flagVAD toggles while both stages run; the +-1 utterance has its gains on their
floors; 300 frames take every ring round many times."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3, 5)
DEPTH = 12
MAX_SIGNAL = 2 * DEPTH + 4


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


def _distinct():
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in range(1, MAX_SIGNAL + 1):
            ragged = (len(utts) % 3 == 0) * (3 + (lead + n) % 70)
            utts.append(np.concatenate([z(lead), _speech(7400 + 64 * lead + n, 80 * n + ragged)]))
    assert len(utts) == len(LEADS) * MAX_SIGNAL
    special = len(utts)
    utts.append(np.zeros(0, np.int16))                           # empty
    utts.append(z(30))                                           # all zero: the gate never opens
    last = z(25)
    last[80 * 24 + 41] = -3                                      # the gate opens on the last frame
    utts.append(last)
    one = z(61)
    one[7] = 1                                                   # one non-zero sample, then 60 zero frames
    utts.append(one)
    utts.append(_gated(7902, 240))                               # flagVAD toggles while both stages run
    utts.append(np.concatenate([z(2), _gated(7903, 238), np.zeros(11, np.int16)]))
    utts.append(np.sign(_gated(7904, 220).astype(np.int32)).astype(np.int16))   # amplitude +-1: gains on their floors
    utts.append(_speech(7910, 80 * 300 + 9))                     # 300 frames
    return utts, special


@pytest.fixture(scope="module")
def idct_corpus():
    return _distinct()


@pytest.fixture(scope="module")
def idct_traces(oracle, idct_corpus):
    """The oracle's trace of every distinct utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in idct_corpus[0]]


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


def test_ns6_idct_sums_corpus_exact(idct_corpus, idct_traces):
    """Forms 6 (dense) and 3 (plain) forced on more than 256 utterances -- the distinct ones and copies of them, in another order --
    so the launch orders them longest first and the waves set their priority by remaining frames."""
    import speech_enhancement_amd as sea
    utts, _ = idct_corpus
    n = len(utts)
    idx = list(range(n)) + [(7 * j + 3) % n for j in range(n)] + list(range(n - 1, n - 9, -1))
    assert len(idx) > 256, len(idx)
    _forced(sea, _torch(), [utts[u] for u in idx], [idct_traces[u] for u in idx], "")


def test_ns6_idct_sums_seven_utterances_without_priorities(idct_corpus, idct_traces):
    """The same two forms on seven utterances (fewer than CUs: no priority rule, no launch order): the two gated ones, the +-1 one, the
    300 frames, the single sample, and the longest signal behind no and behind five leading zero frames."""
    import speech_enhancement_amd as sea
    utts, special = idct_corpus
    pick = [special + 4, special + 5, special + 6, special + 7, special + 3, MAX_SIGNAL - 1, len(LEADS) * MAX_SIGNAL - 1]
    assert len(pick) == 7
    _forced(sea, _torch(), [utts[u] for u in pick], [idct_traces[u] for u in pick], ", seven utterances")
