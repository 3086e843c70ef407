"""The six-wave NoiseSup kernels run their steady beats two by two (ns_pipe6_kernel.hip, run_beats, PAIRED): an even beat and the odd
one after it are two copies of the role's steady code in which the frame parity -- the index of every double-buffered record between
the roles and of the two transform work areas -- is a constant.  A steady range that starts on an odd beat gives its first beat to the
general copy, one that ends behind an even beat its last.  Same operations on the same operands in the same order, so forms 6 (dense)
and 3 (plain, which takes the steady copies with this change) must both equal the CPU oracle exactly: int16 audio, float stream bit
for bit, index of the first output frame, untouched tail.

The corpus is the smallest at which the pairing can go wrong: signal lengths 1 .. 2 x 12 + 4 frames behind 0, 1, 2, 3 and 5 leading
zero frames give every role steady ranges that are empty, one beat, two beats and longer, that begin on even and on odd beats (the
range begins a fixed number of beats behind the onset) and end on even and on odd beats (it ends a fixed number before the last
frame) -- a copy with the wrong parity reads the other record of a pair, or the other work area, and the output differs; they also
cover the beats on which only one side of the dual transform is active (fill: stage 0 only; drain: stage 1 only).  The empty and the
all-zero utterance never leave the general copies; a gate that opens on the last frame; a +-1 utterance (the smallest non-zero
spectra); a full-scale square wave (+-32767: PSDs near 2^45, the largest the int16 input allows); 300 frames take every ring round
many times.

The frame-dropping kernel (ns_denoise_pipe6_fd_kernel, up to two utterances per CU) pairs its beats too: the same utterances go
through afe_features_batch, whose NoiseSup launch it is -- audio, float stream and first output frame against the same traces, and
the VAD column of the feature rows, which is made of the speech bits that kernel leaves per frame, against the oracle's feature chain."""
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


def _square(frames, period):
    """full-scale square wave: +-32767, `period` samples per half cycle"""
    n = np.arange(80 * frames)
    return np.where((n // period) % 2 == 0, 32767, -32767).astype(np.int16)


def _distinct():
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in range(1, MAX_SIGNAL + 1):
            ragged = (len(utts) % 3 == 0) * (3 + (lead + n) % 70)
            utts.append(np.concatenate([z(lead), _speech(9100 + 64 * lead + n, 80 * n + ragged)]))
    assert len(utts) == len(LEADS) * MAX_SIGNAL
    special = len(utts)
    utts.append(np.zeros(0, np.int16))                           # empty
    utts.append(z(30))                                           # all zero: the gate never opens
    last = z(25)
    last[80 * 24 + 17] = 5                                       # the gate opens on the last frame
    utts.append(last)
    utts.append(np.sign(_gated(9204, 120).astype(np.int32)).astype(np.int16))   # amplitude +-1
    utts.append(_square(40, 5))                                  # full scale, 800 Hz and its odd harmonics
    utts.append(np.concatenate([z(1), _square(30, 1)]))          # full scale at the Nyquist bin
    utts.append(_gated(9205, 120))                               # flagVAD toggles while both stages run
    utts.append(_speech(9210, 80 * 300 + 9))                     # 300 frames
    return utts, special


@pytest.fixture(scope="module")
def chain_corpus():
    return _distinct()


@pytest.fixture(scope="module")
def chain_traces(oracle, chain_corpus):
    """The oracle's trace of every distinct utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in chain_corpus[0]]


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


def test_ns6_paired_beats_corpus_exact(chain_corpus, chain_traces):
    """Forms 6 (dense) and 3 (plain) forced on more than 256 utterances -- the distinct ones and copies of them, in another order --
    so the launch orders them longest first and the waves set their priority by remaining frames."""
    import speech_enhancement_amd as sea
    utts, _ = chain_corpus
    n = len(utts)
    idx = list(range(n)) + [(5 * j + 2) % n for j in range(n)] + list(range(n - 1, n - 9, -1))
    assert len(idx) > 256, len(idx)
    _forced(sea, _torch(), [utts[u] for u in idx], [chain_traces[u] for u in idx], "")


def test_ns6_paired_beats_seven_utterances_without_priorities(chain_corpus, chain_traces):
    """The same two forms on seven utterances (fewer than CUs: no priority rule, no launch order): the two square waves, the +-1 one,
    the gated one, the 300 frames, and the longest signal behind no and behind five leading zero frames."""
    import speech_enhancement_amd as sea
    utts, special = chain_corpus
    pick = [special + 4, special + 5, special + 3, special + 6, special + 7, MAX_SIGNAL - 1, len(LEADS) * MAX_SIGNAL - 1]
    assert len(pick) == 7
    _forced(sea, _torch(), [utts[u] for u in pick], [chain_traces[u] for u in pick], ", seven utterances")


def test_ns6_paired_beats_frame_dropping_kernel(oracle, chain_corpus, chain_traces):
    """The six-wave frame-dropping kernel on the distinct utterances and copies of them (more than 256, at most 512: launch order and
    priorities on).  NoiseSup's outputs exactly as above; the feature rows' VAD flags exactly, their count, and the cepstra to the
    tolerance smoke() holds them to."""
    import speech_enhancement_amd as sea
    torch = _torch()
    utts, special = chain_corpus
    n = len(utts)
    idx = list(range(n)) + [(5 * j + 2) % n for j in range(n)]
    assert 256 < len(idx) <= 512, len(idx)
    batch = sea.PackedBatch.from_arrays([utts[u] for u in idx], device="cuda:0")
    res = sea.afe_features_batch(batch, want_intermediates=True)
    torch.cuda.synchronize()
    got = batch.split(res["out"])
    gotf = batch.split(res["den_f32"], full_frames_only=True)
    first_h = res["first_out"].cpu().numpy()
    want_feats = {}
    for k, u in enumerate(idx):
        x, tr = utts[u], chain_traces[u]
        nfr = len(x) // 80
        assert np.array_equal(got[k][: nfr * 80], tr["out_i16"][: nfr * 80]), f"utterance {k} (L={len(x)})"
        assert not np.any(got[k][nfr * 80:]), f"utterance {k}: the tail beyond the last whole frame was written"
        assert int(first_h[k]) == (nfr - tr["nout"] if tr["nout"] else -1), f"utterance {k}: first output"
        if tr["nout"]:
            f0 = nfr - tr["nout"]
            assert np.array_equal(gotf[k][f0 * 80: nfr * 80].view(np.uint32), tr["den_f32"].view(np.uint32)), f"utterance {k}: float stream"
        if u not in want_feats:
            want_feats[u] = oracle.afe_trace(x)["vad_out"]
        want, f15 = want_feats[u], res["feats"][k]
        assert f15.shape == want.shape and np.array_equal(f15[:, 14], want[:, 14]), f"utterance {k}: feature rows / VAD flags"
        if len(want):
            assert np.abs(f15[:, :14] - want[:, :14]).max() <= 1e-3, f"utterance {k}: cepstra"
