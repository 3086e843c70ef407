"""The six-wave NoiseSup kernels derive every frame's bookkeeping (valid / tick / produced) from ONE published number,
the index of the utterance's first non-zero frame (ns_pipe6_kernel.hip, onset_poll / tick_ge).  These tests walk that
number and the frame count over everything the pipeline's fill and drain can meet and compare with the CPU oracle
exactly: int16 audio, float stream, index of the first output frame; and, for the frame-dropping kernel that shares the
body, onset, speech flags and features.

The corpus is laid out around two round numbers of frames, K = 16 (the period of the priority rule, kPrioStep) and
A = 12: it reaches beyond K + A leading zero frames, beyond the pipeline's seven beats and the eight slots of its rings,
both sides of every multiple of K, and 2 K + 8 frames of length.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 16
A = 12
MAX_LEAD = 40      # > K + A, > the pipeline depth, both sides of every multiple of K below it
MAX_FRAMES = 2 * K + 8


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _speech(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


def _corpus():
    """More than 256 and at most 512 short utterances: more than an MI355X has CUs, so the launch orders them longest
    first and the waves set their priority by remaining frames; at most two per CU, so the frame-dropping chain takes
    its six-wave kernel."""
    z = lambda frames: np.zeros(80 * frames, np.int16)
    utts = []
    # leading zero frames 0 .. 40 before 12 frames of signal; every third with a ragged tail
    for k in range(MAX_LEAD + 1):
        utts.append(np.concatenate([z(k), _speech(100 + k, 80 * 12 + (k % 3 == 0) * (7 + k))]))
    # utterances of 0 .. 2K + 8 frames; odd ones with a tail that is not a whole frame
    for n in range(MAX_FRAMES + 1):
        utts.append(_speech(200 + n, 80 * n + (n % 2) * ((n * 13) % 80)))
    utts.append(z(30))                                        # all zero: the gate never opens
    utts.append(np.zeros(0, np.int16))                        # empty
    last = z(20)
    last[-1] = 1234                                           # the only non-zero sample is the last of the last frame
    utts.append(last)
    last = np.concatenate([z(33), np.zeros(41, np.int16)])    # the same with a tail beyond the last whole frame
    last[80 * 33 - 1] = -77
    utts.append(last)
    one = z(26)
    one[80 * 9 + 3] = 1                                       # one sample opens the gate, only zeros follow: ticks keep counting
    utts.append(one)
    # all-zero frames AFTER the onset stay valid: runs shorter and longer than K, up to the end, right after the onset
    for j, run in enumerate((1, 2, 3, 4, 5, 7, 8, K - 1, K, K + 1, K + A, K + A + 1, 2 * K + 8)):
        utts.append(np.concatenate([_speech(300 + j, 80 * 6), z(run), _speech(320 + j, 80 * 6 + 11 * (j % 2))]))
        utts.append(np.concatenate([z(j), _speech(340 + j, 80 * (1 + j % 4)), z(run)]))
    # leading zeros x length grid around the batch and pipeline boundaries
    for lead in (1, 3, 4, 5, 6, 7, 8, A - 1, A, A + 1, K - 1, K, K + 1, K + A - 1, K + A, K + A + 1, 2 * K - 1, 2 * K, 2 * K + 1):
        for n in (1, 2, 3, 4, 5, 6, 7, 8, K + 1):
            utts.append(np.concatenate([z(lead), _speech(1000 + 50 * lead + n, 80 * n + ((lead + n) % 4 == 0) * 33)]))
    # a few long ones so that the priority levels differ across the launch
    utts.append(_speech(400, 80 * 300 + 5))
    utts.append(np.concatenate([z(37), _speech(401, 80 * 200)]))
    assert 256 < len(utts) <= 512, len(utts)
    return utts


@pytest.fixture(scope="module")
def onset_corpus():
    return _corpus()


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


def test_ns6_onset_corpus_exact(oracle, onset_corpus):
    """Forms 3 (six waves) and 6 (six waves, seven per SIMD) forced on the onset corpus: bit for bit the oracle's int16
    audio, float stream and first output frame; the samples beyond the last whole frame stay untouched (zero)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    utts = onset_corpus
    batch = sea.PackedBatch.from_arrays(utts)
    traces = [oracle.ns_trace(x, want_state=False) for x in utts]
    prev = lib.sea_ns_kernel_form(0)
    try:
        for form in (3, 6):
            lib.sea_ns_kernel_form(form)
            _check_ns(sea, torch, batch, utts, traces, f"form {form}")
    finally:
        lib.sea_ns_kernel_form(prev)


def test_ns6_onset_small_batch_without_priorities(oracle, onset_corpus):
    """The same two forms on a batch of fewer utterances than CUs (no priority rule, no launch order)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    utts = onset_corpus[::3][:100]
    batch = sea.PackedBatch.from_arrays(utts)
    traces = [oracle.ns_trace(x, want_state=False) for x in utts]
    prev = lib.sea_ns_kernel_form(0)
    try:
        for form in (3, 6):
            lib.sea_ns_kernel_form(form)
            _check_ns(sea, torch, batch, utts, traces, f"form {form}, small batch")
    finally:
        lib.sea_ns_kernel_form(prev)


def test_ns6_onset_frame_dropping_chain(oracle, onset_corpus):
    """sea.afe_features_batch on the onset corpus (at most two utterances per CU: ns_denoise_pipe6_fd_kernel, the same
    body): onset, speech flags per output frame, VAD decisions exact, features within the CompCeps tolerance -- the
    comparison of test_afe_feature_chain_vs_oracle -- and the audio equal to the plain kernel's."""
    import speech_enhancement_amd as sea
    torch = _torch()
    utts = onset_corpus
    batch = sea.PackedBatch.from_arrays(utts)
    res = sea.afe_features_batch(batch, want_intermediates=True)
    flags = res["flags"].cpu().numpy()
    fcc, fpp = res["feat_cc"].cpu().numpy(), res["feat_pp"].cpu().numpy()
    n_ceps, first = res["n_ceps"].cpu().numpy(), res["first_out"].cpu().numpy()
    onset = res["onset"].cpu().numpy()
    for u, x in enumerate(utts):
        tr = oracle.afe_trace(x)
        nfr = len(x) // 80
        assert int(n_ceps[u]) == tr["nceps"], f"utt {u}"
        nz = np.nonzero(x[: nfr * 80])[0]
        assert int(onset[u]) == (int(nz[0]) // 80 if nz.size else nfr), f"utt {u}: onset"
        if tr["nout"]:
            f0 = int(first[u])
            assert f0 == nfr - tr["nout"], f"utt {u}: first output"
            got = flags[batch.host_offsets[u] // 8 + 10 * np.arange(f0, nfr)]
            want = tr["flags"][f0:nfr, :4] @ np.array([1, 2, 4, 8])
            assert np.array_equal(got, want), f"utt {u}: speech flags differ at {np.nonzero(got != want)[0][:5]}"
        else:
            assert int(first[u]) == -1, f"utt {u}: first output"
        c0 = res["ceps_cum"][u]
        if tr["nceps"]:
            for name, g, w in (("feat_cc", fcc, tr["feat_cc"]), ("feat_pp", fpp, tr["feat_pp"])):
                d = float(np.abs(g[c0:c0 + tr["nceps"]] - w).max())
                assert d <= 1e-3, f"utt {u} {name}: off by {d}"
        got15 = res["feats"][u]
        assert got15.shape == tr["vad_out"].shape, f"utt {u}: {got15.shape} vs {tr['vad_out'].shape}"
        if len(got15):
            assert np.array_equal(got15[:, 14], tr["vad_out"][:, 14]), f"utt {u}: VAD flags differ"
            d = float(np.abs(got15[:, :14] - tr["vad_out"][:, :14]).max())
            assert d <= 1e-3, f"utt {u} emitted features: off by {d}"
    plain, _, _ = sea.ns_denoise_batch(batch)
    assert torch.equal(plain, res["out"])
