"""The six-wave NoiseSup kernels run every role's beat in two copies (ns_pipe6_kernel.hip, run_beats): a general one that derives
the frame's flags from (frame, onset, frame count), and a steady one without any of them on the beats where all are true
(ns6_beat_plan.h).  The roles switch at different beats, and back for the drain.  This corpus walks every role's steady trip count
through negative, 0, 1, 2 and both sides of 16 and 32, and compares with the CPU oracle exactly: int16 audio, float stream bit
for bit, index of the first output frame, untouched tail; and, for the frame-dropping kernel that shares the body, onset and speech
flags.

A role's steady trip count is (signal frames) - c with c between 3 (B0) and 14 (S), so signal lengths 1 .. 48 give every role the
counts -2 .. 34; the leading zero frames put the switch on either side of the priority rule's period of 16 beats."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3, 5, 15, 16, 17)
MAX_SIGNAL = 48


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _corpus():
    """More than 256 and at most 512 utterances: the launch orders them longest first and the waves set their priority by remaining
    frames; at most two per CU, so the frame-dropping chain takes its six-wave kernel."""
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in range(1, MAX_SIGNAL + 1):
            ragged = (len(utts) % 3 == 0) * (5 + (lead + n) % 70)
            utts.append(np.concatenate([z(lead), _speech(2000 + 64 * lead + n, 80 * n + ragged)]))
    assert len(utts) == 384
    utts.append(z(30))                                           # all zero: the gate never opens, no role goes steady
    utts.append(np.zeros(0, np.int16))                           # empty
    last = z(25)
    last[80 * 24 + 41] = -3                                      # the gate opens on the last frame
    utts.append(last)
    one = z(61)
    one[7] = 1                                                   # one sample, then 60 zero frames: the steady loop runs on zero frames
    utts.append(one)
    utts.append(np.concatenate([_speech(2900, 80 * 30), z(20), _speech(2901, 80 * 30 + 17)]))   # zero frames inside the steady range
    for j, n in enumerate((300, 700, 1204)):                     # long ones: the priority levels differ across the launch
        utts.append(np.concatenate([z(j), _speech(2910 + j, 80 * n + 9 * j)]))
    assert 256 < len(utts) <= 512, len(utts)
    return utts


@pytest.fixture(scope="module")
def steady_corpus():
    return _corpus()


@pytest.fixture(scope="module")
def steady_traces(oracle, steady_corpus):
    """The oracle's trace of every utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in steady_corpus]


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
        for form in (3, 6):
            lib.sea_ns_kernel_form(form)
            _check_ns(sea, torch, batch, utts, traces, f"form {form}{what}")
    finally:
        lib.sea_ns_kernel_form(prev)


def test_ns6_steady_corpus_exact(steady_corpus, steady_traces):
    """Forms 3 (six waves) and 6 (six waves, seven per SIMD) forced on the whole corpus."""
    import speech_enhancement_amd as sea
    _forced(sea, _torch(), steady_corpus, steady_traces, "")


def test_ns6_steady_small_batch_without_priorities(steady_corpus, steady_traces):
    """The same two forms on fewer utterances than CUs (no priority rule, no launch order); 7 is prime to the 48 lengths per lead, so
    every lead keeps lengths of every residue, and the eight special utterances all stay."""
    import speech_enhancement_amd as sea
    n = len(steady_corpus)
    pick = [u for u in range(n) if u % 7 in (0, 3, 5) or u >= 384]
    assert len(pick) < 256
    _forced(sea, _torch(), [steady_corpus[u] for u in pick], [steady_traces[u] for u in pick], ", small batch")


def test_ns6_steady_frame_dropping_chain(oracle, steady_corpus, steady_traces):
    """sea.afe_features_batch on the corpus (ns_denoise_pipe6_fd_kernel, the same body): onset, index of the first output frame and
    the speech flags of every output frame exact, the audio equal to the plain kernel's and to the oracle's."""
    import speech_enhancement_amd as sea
    torch = _torch()
    utts = steady_corpus
    batch = sea.PackedBatch.from_arrays(utts)
    res = sea.afe_features_batch(batch, want_intermediates=True)
    flags = res["flags"].cpu().numpy()
    first, onset = res["first_out"].cpu().numpy(), res["onset"].cpu().numpy()
    got = batch.split(res["out"])
    for u, (x, trn) in enumerate(zip(utts, steady_traces)):
        tr = oracle.afe_trace(x)
        nfr = len(x) // 80
        nz = np.nonzero(x[: nfr * 80])[0]
        assert int(onset[u]) == (int(nz[0]) // 80 if nz.size else nfr), f"utt {u}: onset"
        assert np.array_equal(got[u][: nfr * 80], trn["out_i16"][: nfr * 80]), f"utt {u}: audio"
        if tr["nout"]:
            f0 = int(first[u])
            assert f0 == nfr - tr["nout"], f"utt {u}: first output"
            g = flags[batch.host_offsets[u] // 8 + 10 * np.arange(f0, nfr)]
            want = tr["flags"][f0:nfr, :4] @ np.array([1, 2, 4, 8])
            assert np.array_equal(g, want), f"utt {u}: speech flags differ at {np.nonzero(g != want)[0][:5]}"
        else:
            assert int(first[u]) == -1, f"utt {u}: first output"
    plain, _, _ = sea.ns_denoise_batch(batch)
    assert torch.equal(plain, res["out"])
