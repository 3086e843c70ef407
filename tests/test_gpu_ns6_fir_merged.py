"""In the dense six-wave NoiseSup kernel G1 runs both 17-tap filters as one pass on its two lane halves (ns_pipe6_kernel.hip, FIRP;
ns_core.h, ns_fir_pair3): lane 32 h + j, j < 27, computes outputs 3j .. 3j + 2 of stage h -- stage-0 frame i-4 into the stage-1
buffer, stage-1 frame i-12 into the output record -- from per-lane taps and 19 samples at a stride of three words.  FA filters no more,
the filtered stage-0 frame crosses a frame barrier before FA windows it, every stage-1 job sits one beat later and the pipeline is
thirteen beats deep instead of twelve.  Every output is the same in-order 17-term sum of the same rounded products, so forms 6 (dense)
and 3 (plain, the control: its listing did not change) must both equal the CPU oracle exactly: int16 audio, float stream bit for bit,
index of the first output frame, untouched tail.

The corpus is the smallest at which the new schedule can go wrong.  Signal lengths of 0 .. 5, 12 .. 20, 25, 26, 41 and 130 whole frames
behind 0, 1, 2, 3, 5 and 9 leading zero frames, each with a ragged tail of 0, 1 or 79 samples: the pipeline never steady (G1's range
opens 16 beats after the onset and closes 4 beats after the last frame: a range of 0 beats with 12 signal frames), ranges of 1 and 2
beats (13 and 14 frames: a lone beat goes to the general copy of the paired loop), ranges that begin on odd and on even beats (the leads), the fill in
which only the low half of the pass is live, the drain in which only the high half is, one trip and many round the sixteen-slot rings.
Beside the speech-like noise: a constant, impulses at samples 78 .. 82 of a frame (outputs 78 and 79 are lane 26's first two, 80 is its
third, which must not be stored, and 0 .. 2 of the next frame are lane 0's: the slot edge), a full-scale square wave with -32768, an
all-zero and an empty utterance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = (0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17, 18, 19, 20, 25, 26, 41, 130)
LEADS = (0, 1, 2, 3, 5, 9)
TAILS = (0, 1, 79)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _distinct():
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in FRAMES:
            for tail in TAILS:
                utts.append(np.concatenate([z(lead), _speech(9100 + 1000 * lead + 3 * n + (tail > 0) + (tail > 1), 80 * n + tail)]))
    assert len(utts) == len(LEADS) * len(FRAMES) * len(TAILS)
    special = len(utts)
    utts.append(np.zeros(0, np.int16))                                           # empty
    utts.append(z(30))                                                           # all zero: the gate never opens
    utts.append(np.full(80 * 26 + 1, 1000, np.int16))                            # a constant
    utts.append(np.concatenate([z(3), np.full(80 * 41, -32768, np.int16)]))      # the most negative constant
    for s in (78, 79, 80, 81, 82):                                               # impulses at the slot edge, alone ...
        x = z(26)
        x[80 * 6 + s] = 20000
        x[80 * 15 + s] = -32768
        utts.append(x)
    for s in (78, 79, 80, 81, 82):                                               # ... and on top of speech-like noise, behind a lead
        x = np.concatenate([z(s - 77), _speech(9900 + s, 80 * 41 + 79) // 4])
        x[80 * 9 + s] = 32767
        x[80 * 22 + s] = -32768
        utts.append(x)
    k = np.arange(80 * 41 + 1)
    utts.append(np.where((k // 8) % 2 == 0, 32767, -32768).astype(np.int16))     # full-scale square wave, period 16
    utts.append(np.concatenate([z(1), np.where((k // 40) % 2 == 0, -32768, 32767).astype(np.int16)]))   # period 80: one edge per frame
    return utts, special


@pytest.fixture(scope="module")
def fir_corpus():
    return _distinct()


@pytest.fixture(scope="module")
def fir_traces(oracle, fir_corpus):
    """The oracle's trace of every distinct utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in fir_corpus[0]]


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


def test_ns6_fir_merged_corpus_twice_exact(fir_corpus, fir_traces):
    """Forms 6 (dense) and 3 (plain) forced on every utterance twice, the second time in another order: more utterances than two
    launch rows hold, so the launch orders them longest first and the waves set their priority by remaining frames."""
    import speech_enhancement_amd as sea
    utts, _ = fir_corpus
    n = len(utts)
    step = next(s for s in (7, 11, 13, 17) if n % s)
    idx = list(range(n)) + [(step * j + 3) % n for j in range(n)]
    assert sorted(idx) == sorted(2 * list(range(n))) and len(idx) > 512, len(idx)
    _forced(sea, _torch(), [utts[u] for u in idx], [fir_traces[u] for u in idx], "")


def test_ns6_fir_merged_seven_utterances_without_priorities(fir_corpus, fir_traces):
    """The same two forms on seven utterances (fewer than CUs: no priority rule, no launch order): 130 frames behind no and behind
    nine leading zero frames, G1's lone steady beat (13 frames behind one zero frame), an impulse at sample 80 alone and one on noise,
    the square wave and the empty utterance."""
    import speech_enhancement_amd as sea
    utts, special = fir_corpus
    at = lambda lead, n, tail: (LEADS.index(lead) * len(FRAMES) + FRAMES.index(n)) * len(TAILS) + TAILS.index(tail)
    pick = [at(0, 130, 79), at(9, 130, 0), at(1, 13, 1), special + 4 + 2, special + 9 + 2, special + 14, special]
    assert len(pick) == 7 and len(utts) == special + 16
    _forced(sea, _torch(), [utts[u] for u in pick], [fir_traces[u] for u in pick], ", seven utterances")
