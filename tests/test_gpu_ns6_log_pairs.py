"""In the dense six-wave NoiseSup kernel N1 takes the VAD log-energies of a steady pair of beats (2h, 2h+1) as ONE pass in the odd
beat, the two sums in its even and odd lanes (ns_pipe6_kernel.hip, LOGP; ns_core.h, ns_log_lanes_request / ns_log_lanes_take): the
even beat's value is written one beat later than before, still one barrier ahead of B0's read, and the general copy -- the fill, the
drain, an odd first or last beat -- keeps one logarithm per beat.  Per lane the pass is operation by operation the complete site, so
forms 6 (dense) and 3 (plain, the control: its listing did not change) must both equal the CPU oracle exactly: int16 audio, float
stream bit for bit, index of the first output frame, untouched tail.

The corpus is the smallest at which the hand-over between the two copies can go wrong.  N1's steady range is the beats
onset + 13 <= i < nfr + 2 (lead and tail of ns6plan::kPlanFirPair's N1, which tests/test_ns6_fir_plan_cpu.py holds to the header),
and the paired loop runs the pairs that lie wholly inside it.  Behind 0, 1, 2 and 3 all-zero frames (ranges that start on odd and on
even beats, and end behind both): 1, 2 and 13 .. 17 signal frames, which straddle the pipeline's depth of 13, and for zero, one, two
and three pairs the shortest signal that gives that many (for zero also the longest), computed below from the range.  One length has
a ragged tail of 79 samples; one utterance has a second of silence in its middle, on which the VAD sum is 64 and its logarithm the
expression's constant; an all-zero and an empty utterance close the list.  No utterance is longer than 200 frames."""
import numpy as np
import pytest

N1_LEAD, N1_TAIL = 13, 2
LEADS = (0, 1, 2, 3)
STRADDLE = (1, 2, 13, 14, 15, 16, 17)


def _pairs(lead, n):
    """steady pairs of N1 for n signal frames behind `lead` zero frames: even beats 2h with [2h, 2h + 1] inside the range"""
    begin, end = lead + N1_LEAD, lead + n + N1_TAIL
    return max(0, (end >> 1) - ((begin + 1) >> 1))


def _lengths(lead):
    ns = set(STRADDLE)
    for p in (0, 1, 2, 3):
        ns.add(next(n for n in range(1, 200) if _pairs(lead, n) == p))
    ns.add(max(n for n in range(1, 200) if _pairs(lead, n) == 0))
    return sorted(ns)


def test_pair_counts_follow_from_the_range():
    """the lengths the corpus takes from the range: every lead sees zero to three pairs, and the hand-over on both parities"""
    assert [_pairs(0, n) for n in (12, 13, 14, 15, 16, 18)] == [0, 0, 1, 1, 2, 3]     # range [13, n + 2): first pair (14, 15)
    assert [_pairs(1, n) for n in (12, 13, 14, 15, 17)] == [0, 1, 1, 2, 3]            # range [14, n + 3): first pair (14, 15)
    for lead in LEADS:
        assert {_pairs(lead, n) for n in _lengths(lead)} >= {0, 1, 2, 3}, lead


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
        for n in _lengths(lead):
            utts.append(np.concatenate([z(lead), _speech(15100 + 100 * lead + n, 80 * n)]))
    special = len(utts)
    utts.append(np.concatenate([z(1), _speech(15900, 80 * 16 + 79)]))                            # a ragged tail of 79 samples
    utts.append(np.concatenate([_speech(15901, 80 * 45), z(100), _speech(15902, 80 * 45)]))      # a second of silence inside steady pairs
    utts.append(z(30))                                                                           # all zero: the gate never opens
    utts.append(np.zeros(0, np.int16))                                                           # empty
    assert max(len(x) for x in utts) <= 80 * 200
    return utts, special


@pytest.fixture(scope="module")
def log_corpus():
    return _distinct()


@pytest.fixture(scope="module")
def log_traces(oracle, log_corpus):
    """The oracle's trace of every distinct utterance, computed once and only read by the tests."""
    return [oracle.ns_trace(x, want_state=False) for x in log_corpus[0]]


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


@pytest.mark.gpu
def test_ns6_log_pairs_corpus_twice_exact(log_corpus, log_traces):
    """Forms 6 (dense) and 3 (plain) forced on every utterance twice in one batch, the second time in another order."""
    import speech_enhancement_amd as sea
    utts, _ = log_corpus
    n = len(utts)
    step = next(s for s in (7, 11, 13, 17) if n % s)
    idx = list(range(n)) + [(step * j + 3) % n for j in range(n)]
    assert sorted(idx) == sorted(2 * list(range(n)))
    _forced(sea, _torch(), [utts[u] for u in idx], [log_traces[u] for u in idx], "")


@pytest.mark.gpu
def test_ns6_log_pairs_seven_utterances(log_corpus, log_traces):
    """The same two forms on seven utterances (fewer than CUs: no priority rule, no launch order): the silence, the ragged tail, the
    first lengths with one pair behind no and behind one zero frame, three pairs behind three, and the two without signal."""
    import speech_enhancement_amd as sea
    utts, special = log_corpus
    at = lambda lead, n: sum(len(_lengths(l)) for l in LEADS[: LEADS.index(lead)]) + _lengths(lead).index(n)
    one = lambda lead: next(n for n in range(1, 200) if _pairs(lead, n) == 1)
    three = next(n for n in range(1, 200) if _pairs(3, n) == 3)
    pick = [special + 1, special, at(0, one(0)), at(1, one(1)), at(3, three), special + 2, special + 3]
    assert len(set(pick)) == 7 and len(utts) == special + 4
    _forced(sea, _torch(), [utts[u] for u in pick], [log_traces[u] for u in pick], ", seven utterances")


@pytest.mark.gpu
@pytest.mark.parametrize("all_vad", (0, 1))
def test_log_lanes_equal_the_complete_sites_on_every_argument(all_vad):
    """sea_selftest_log_lanes: the lane form against ns_vad_energy_expr<false> and ns_aversnr_expr<false> on every float argument of
    either site, two neighbouring arguments per wave and pass -- as both sites at once (four logarithms per pass) and as the VAD site
    alone, which is how N1 runs it.  No result and no guard decision may differ; the guard must have fired, and each pass that took
    the slow branch did so for at least one counted lane."""
    import speech_enhancement_amd as sea
    _torch()
    stats = np.zeros(8, np.uint64)
    assert sea.load().sea_selftest_log_lanes(all_vad, stats.ctypes.data) == 0, sea.load().sea_last_error()
    n1, n2, hit1, hit2, bad1, bad2, slow, _ = (int(v) for v in stats)
    print(f"all_vad={all_vad}: arguments {n1} / {n2}, guard hits {hit1} / {hit2}, differing {bad1} / {bad2}, slow passes {slow}")
    assert n1 == 0x7F7FFFFF - 0x42800000 + 1                      # every finite float >= 64
    assert n2 == (0 if all_vad else 0x7F7FFFFF - 0x3727C5AD + 1)  # every finite float above 1e-5
    assert bad1 == 0 and bad2 == 0
    assert hit1 > 0 and (all_vad or hit2 > 0)
    assert 0 < slow <= hit1 + hit2
