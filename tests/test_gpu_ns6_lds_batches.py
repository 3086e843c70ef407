"""The six-wave NoiseSup kernels fetch what three of their roles used to wait for in turn as one batch of LDS reads each
(ns_pipe6_kernel.hip, round 9): the helper wave S takes the frame's squares and the DC filter's input differences from one batch
(lanes 0..39, samples 2l and 2l + 1, lane 0's predecessor the carried last sample), B0 and G1 the 25 IDCT basis values ahead of the
in-order sum, G1 the mean PSD with its first batch.  Scheduling only, so forms 6 (dense) and 3 (plain) must both equal the CPU oracle
exactly: int16 audio, float stream bit for bit, index of the first output frame, untouched tail -- with the float stream (both store
paths of S) and without it.

The corpus is sized for where the new prep can go wrong: 0 .. 3 leading zero frames before 1 .. 24 frames of signal cover the fill
(squares taken on ticks 1 .. 4 without an output), the drain (outputs without squares), utterances whose steady range of S is empty
(below about 15 frames) and the first produced frame, whose predecessor sample is 0; 40 .. 60 frames run the steady copy; 20 zero
frames in the middle give zero differences while outputs go on; amplitude +-1; and the full-scale DC, square and Nyquist signals of
tests/ns_edge_cases.py give the DC filter's largest transients with distinct values in samples 0, 63 / 64 and 79."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 2, 3)
MAX_SIGNAL = 24


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _corpus():
    """Fewer than 256 utterances: one launch without an order's priorities; _padded() takes it past 256."""
    from tests import ns_edge_cases as E
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    for lead in LEADS:
        for n in range(1, MAX_SIGNAL + 1):
            ragged = (len(utts) % 3 == 0) * (3 + (lead + n) % 70)
            utts.append(np.concatenate([z(lead), _speech(5000 + 32 * lead + n, 80 * n + ragged)]))
    assert len(utts) == len(LEADS) * MAX_SIGNAL
    for j, n in enumerate((40, 47, 53, 60)):                     # the steady copy of every role runs
        utts.append(np.concatenate([z(j), _speech(5200 + j, 80 * n + 7 * j)]))
    utts.append(np.concatenate([_speech(5210, 80 * 30), z(20), _speech(5211, 80 * 30 + 17)]))   # zero differences, outputs go on
    utts.append(np.sign(_speech(5212, 80 * 50).astype(np.int32)).astype(np.int16))              # amplitude +-1
    utts.extend(E.signals_8k().values())
    assert len(utts) < 256, len(utts)
    return utts


def _padded(utts):
    """The same utterances followed by short ones, more than 256 in all: the launch orders them longest first and the waves set
    their priority by remaining frames."""
    pad = [_speech(5300 + k, 80 * (1 + k % 9) + (k % 4) * 5) for k in range(257 - len(utts) + 8)]
    return list(utts) + pad


@pytest.fixture(scope="module")
def batch_corpus():
    return _padded(_corpus())


@pytest.fixture(scope="module")
def batch_traces(oracle, batch_corpus):
    """The oracle's trace of every utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in batch_corpus]


def _check_ns(sea, torch, batch, utts, traces, want_f32, what):
    out, f32, first = sea.ns_denoise_batch(batch, want_f32=want_f32)
    torch.cuda.synchronize()
    assert (f32 is not None) == want_f32
    got = batch.split(out)
    gotf = batch.split(f32, full_frames_only=True) if want_f32 else None
    first_h = first.cpu().numpy()
    for u, (x, tr) in enumerate(zip(utts, traces)):
        nfr = len(x) // 80
        assert np.array_equal(got[u][: nfr * 80], tr["out_i16"][: nfr * 80]), f"{what}, utterance {u} (L={len(x)})"
        assert not np.any(got[u][nfr * 80:]), f"{what}, utterance {u}: the tail beyond the last whole frame was written"
        assert int(first_h[u]) == (nfr - tr["nout"] if tr["nout"] else -1), f"{what}, utterance {u}: first output"
        if want_f32 and tr["nout"]:
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
            for want_f32 in (True, False):
                _check_ns(sea, torch, batch, utts, traces, want_f32, f"form {form}{what}, {'with' if want_f32 else 'without'} f32")
    finally:
        lib.sea_ns_kernel_form(prev)


def test_ns6_lds_batches_small_batch_exact(batch_corpus, batch_traces):
    """Forms 6 (dense) and 3 (plain) forced on the corpus alone: fewer than 256 utterances, the plain launch."""
    import speech_enhancement_amd as sea
    n = len(_corpus())
    assert n < 256
    _forced(sea, _torch(), batch_corpus[:n], batch_traces[:n], ", small batch")


def test_ns6_lds_batches_padded_batch_exact(batch_corpus, batch_traces):
    """The same utterances padded past 256 with short ones: launch order and priorities on."""
    import speech_enhancement_amd as sea
    assert len(batch_corpus) > 256
    _forced(sea, _torch(), batch_corpus, batch_traces, ", padded batch")
