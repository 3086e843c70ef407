"""GPU tests of the NoiseSup kernels, the feature chain, the 16 k-native variant and the wideband mode on the edge signals of
tests/ns_edge_cases.py: inputs that take the branches of the frame loop which the speech-like corpus never takes (the
meanEn floor, both eps floors of the noise estimate, the SNR jump and the acceleration latch inside the first frames,
PostProc's middle weight, the raised VAD hang-over, WaveProc's wrapped sums and its search without a maximum --
tests/test_edge_coverage_cpu.py measures this; tests/test_oracle.py pins the restatement to the reference on the same
inputs).  Every kernel form carries that arithmetic separately, so every form runs here.

All comparisons are bit for bit (the kernels are written to be bit-identical; SURVEY 8(c)'s tolerances are the outer
contract, not the bar here), and within a test all signals share one batch, so that neighbouring workgroups are in
different regimes.  Every test prints how many words it compared.  Run on an MI355X with ``pytest -m gpu``."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def edge(oracle):
    """the 8 kHz edge signals with the restatement's traces, computed once and left unchanged"""
    from tests import ns_edge_cases as E
    sig = E.signals_8k()
    names, utts = list(sig), list(sig.values())
    assert all(len(x) % 80 == 0 and np.any(x[:80]) for x in utts)      # whole frames, the gate opens on the first one
    ns = [oracle.ns_trace(x, want_state=False) for x in utts]
    afe = [oracle.afe_trace(x) for x in utts]
    assert all(tr["nout"] == len(x) // 80 - 4 for tr, x in zip(ns, utts))
    return dict(names=names, utts=utts, ns=ns, afe=afe, nfr=[len(x) // 80 for x in utts])


def _check_ns(edge, got_i16, got_f32, first, what, idx=None):
    """int16 audio, float stream and first_out of utterances idx (default: all, in order) against the traces; an entry
    (u, n) of idx is the first n frames of signal u (the loop is causal: the trace's prefix).  Returns words"""
    words = 0
    idx = range(len(edge["utts"])) if idx is None else idx
    for k, e in enumerate(idx):
        u, nfr = e if isinstance(e, tuple) else (e, edge["nfr"][e])
        tr, name = edge["ns"][u], edge["names"][u]
        f0 = edge["nfr"][u] - tr["nout"]
        want = tr["out_i16"][: nfr * 80]
        assert np.array_equal(got_i16[k], want), \
            f"{what}, {name}: {int(np.sum(got_i16[k] != want))} of {want.size} int16 samples differ, first at {int(np.argmax(got_i16[k] != want))}"
        if first is not None:
            assert int(first[k]) == f0, f"{what}, {name}: first_out {int(first[k])} != {f0}"
        words += want.size
        if got_f32 is not None:
            g, w = _u32(got_f32[k][f0 * 80: nfr * 80]), _u32(tr["den_f32"][: (nfr - f0) * 80])
            assert np.array_equal(g, w), f"{what}, {name}: {int(np.sum(g != w))} of {w.size} floats differ, first at frame {f0 + int(np.argmax(g != w)) // 80}"
            words += w.size
    return words


def test_a_batch_kernels_every_form(edge):
    """(a) sea_ns_denoise_batch with the kernel form forced to 2, 3, 4 and 6 and chosen by the library, with and without the
    launch order: int16 audio, float stream and first_out equal oracle.ns_trace"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    batch = sea.PackedBatch.from_arrays(edge["utts"])
    prev = lib.sea_ns_kernel_form(0)
    words = 0
    try:
        for form in (2, 3, 4, 6, 0):
            lib.sea_ns_kernel_form(form)
            for use_order in (True, False):
                out, f32, first = sea.ns_denoise_batch(batch, want_f32=True, use_order=use_order)
                torch.cuda.synchronize()
                words += _check_ns(edge, batch.split(out, full_frames_only=True), batch.split(f32, full_frames_only=True),
                                   first.cpu().numpy(), f"form {form or 'auto'}, use_order={use_order}")
    finally:
        lib.sea_ns_kernel_form(prev)
    print(f"\n(a) {words} words (int16 samples + floats) equal the restatement's over 5 forms x 2 launch orders")


def _slices(sea, torch, lib, ulist, bounds, big_until, n_cu):
    """ulist (longest first) through sea_ns_denoise_batch_slice at the frame bounds -> (int16 per utterance, f32 per
    utterance, first).  The entry picks the lower-register form for a launch of more than 4 * n_cu utterances, the four-wave
    form otherwise: asserted per launch -- the former for every slice that starts before frame big_until, the latter after."""
    n = len(ulist)
    nf = np.array([len(x) // 80 for x in ulist])
    assert np.all(np.diff(nf) <= 0)
    state = torch.zeros((n, lib.sea_ns_slice_state_floats()), dtype=torch.float32, device="cuda")
    first = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    outs, outf = [[] for _ in range(n)], [[] for _ in range(n)]
    for k in range(len(bounds) - 1):
        b0, b1 = bounds[k], bounds[k + 1]
        act = int(np.sum(nf > b0))                      # a prefix, by the sort
        if act == 0:
            break
        assert (act > 4 * n_cu) == (b0 < big_until), f"slice from frame {b0}: {act} utterances active, {4 * n_cu} is the threshold between the forms"
        sl = sea.PackedBatch.from_arrays([x[80 * b0: 80 * min(b1, len(x) // 80)] for x in ulist[:act]])
        o = torch.full_like(sl.data, -5)
        f32 = torch.zeros(sl.total, dtype=torch.float32, device="cuda")
        rc = lib.sea_ns_denoise_batch_slice(sl.data.data_ptr(), o.data_ptr(), f32.data_ptr(), sl.offsets.data_ptr(), sl.lengths.data_ptr(),
                                            None, first.data_ptr(), state.data_ptr(), act, b0, int(k > 0), None)
        assert rc == 0, lib.sea_last_error()
        torch.cuda.synchronize()
        for u, (a, b) in enumerate(zip(sl.split(o, full_frames_only=True), sl.split(f32, full_frames_only=True))):
            outs[u].append(a)
            outf[u].append(b)
    return [np.concatenate(v) for v in outs], [np.concatenate(v) for v in outf], first.cpu().numpy()


# frames of ones_then_zeros kept in the copies that fill the lower-register form's batch: its second stage sits on the eps
# floor from about frame 190 on (tools/oracle_coverage.py --only: 200 zero frames reach it), meanEn on its floor long before
FILL_FRAMES = 260


def test_b_time_slices_equal_one_launch(edge):
    """(b) sea_ns_denoise_batch_slice with cut points inside the long zero runs (140, 230, 300, 600: loud_then_zeros is
    silent from frame 60, utt_gap_utt from 100 to 400, ones_then_zeros from 10), one frame after the loud onsets (7:
    onset_tone's tone starts in frame 6; 11: square4_burst's in frame 10), at frames 9 / 10 / 11 where the `nbFrame < 10`
    rules change and at 99 / 100 / 101 where lambda changes -- the state blob carries a floored, a latched and a freshly
    jumped recursion across launches.  Both forms the slices use, each with all of these cuts up to frame 230: the
    four-wave form (the 14 signals), and the lower-register form, which the entry takes for more than four utterances
    per CU: every edge signal once plus 4 n_cu + 1 copies of the first 260 frames of ones_then_zeros, so that every launch
    up to the one from frame 230 is over the threshold (asserted per launch) and that one loads a state whose meanEn and
    second-stage noise estimate sit on their floors.  The FIRST stage's eps floor (frame 1000 on) is carried across a cut
    by the four-wave form only (the launches from 260, 300 and 600 of either run): reaching it under the lower-register form
    would take a thousand utterances of a thousand frames."""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    every = list(range(len(edge["utts"])))
    longest = max(edge["nfr"])
    otz = edge["names"].index("ones_then_zeros")
    assert longest > 700 and len(every) <= 4 * n_cu
    bounds = (0, 7, 9, 10, 11, 99, 100, 101, 140, 230, FILL_FRAMES, 300, 600, longest)
    words = 0
    for what, fill, big_until in (("four-wave form", 0, 0), ("lower-register form", 4 * n_cu + 1, FILL_FRAMES)):
        idx = sorted(every + [(otz, FILL_FRAMES)] * fill, key=lambda e: -(e[1] if isinstance(e, tuple) else edge["nfr"][e]))   # longest first
        ulist = [edge["utts"][e[0]][: 80 * e[1]] if isinstance(e, tuple) else edge["utts"][e] for e in idx]
        o, f, first = _slices(sea, torch, lib, ulist, bounds, big_until, n_cu)
        words += _check_ns(edge, o, f, first, f"{what}, {len(bounds) - 1} slices", idx)
    print(f"\n(b) {words} words equal the restatement's (= the one launch) over both slice forms")


def _vad_column(rows, raise_hangover):
    """DoVADProc / DoVADFlush's flag column (VAD.c:219-433) from the per-cepstral-frame speech flags and frame counter
    [n, 5]; raise_hangover=False leaves out `if (FrameCounter <= 35) hangOver = 50`.  None: emitted without a decision."""
    buf, st = [0] * 7, dict(hang=23, hc=0, vc=0)

    def decide(focus, fc):
        run = trig = 0
        for i in range(7):
            if buf[(focus + i + 1) % 7]:
                run += 1
            else:
                trig, run = max(trig, run), 0
        trig = max(trig, run)
        if trig >= 4:
            st["hc"] = st["hang"]
            if fc <= 35 and raise_hangover:
                st["hang"] = 50
        if st["hc"] and trig < 3:
            st["hc"] -= 1
        if trig >= 3:
            st["vc"] = 5
        if st["vc"] and trig < 3:
            st["vc"] -= 1
        return 1 if (st["vc"] or st["hc"] or trig >= 3) else 0

    col, focus, fc = [], 0, 0
    for r in rows:
        focus = (focus + 1) % 7
        buf[focus], fc = int(np.any(r[:4])), int(r[4])
        if fc > 10:
            col.append(decide(focus, fc))
    stop = focus
    while (focus + 1) % 7 != stop:
        focus = (focus + 1) % 7
        fc += 1
        col.append(decide(focus, fc) if fc > 10 else None)
    return col


def _chain_conditions(edge):
    """what keeps (c) honest, from the restatement's traces: frames in PostProc's middle branch; an utterance whose VAD
    column holds a 1 that only the hang-over of 50 explains"""
    middle, by_hang = 0, []
    for name, tr, nfr in zip(edge["names"], edge["afe"], edge["nfr"]):
        logE = tr["feat_cc"][:, 13]
        middle += int(np.sum((logE > np.float32(211.0 / 64)) & (logE < np.float32(275.0 / 64))))
        rows = tr["flags"][nfr - tr["nceps"]:]                          # the frames that produced a cepstral frame
        want = tr["vad_out"][:, 14]
        with50, with23 = _vad_column(rows, True), _vad_column(rows, False)
        assert len(with50) == len(want) and all(a is None or a == b for a, b in zip(with50, want)), f"{name}: the VAD model of this test is wrong"
        if any(a == 0 and b == 1 for a, b in zip(with23, want)):
            by_hang.append(name)
    return middle, by_hang


def _check_chain(edge, sea, idx, what):
    batch = sea.PackedBatch.from_arrays([edge["utts"][u] for u in idx])
    res = sea.afe_features_batch(batch, want_intermediates=True)
    flags = res["flags"].cpu().numpy()
    fcc, fpp = res["feat_cc"].cpu().numpy(), res["feat_pp"].cpu().numpy()
    n_ceps, first = res["n_ceps"].cpu().numpy(), res["first_out"].cpu().numpy()
    out = batch.split(res["out"], full_frames_only=True)
    words = 0
    for k, u in enumerate(idx):
        tr, nfr, name = edge["afe"][u], edge["nfr"][u], f"{what}, {edge['names'][u]}"
        assert int(n_ceps[k]) == tr["nceps"] and int(first[k]) == nfr - tr["nout"], f"{name}: frame counts"
        f0 = int(first[k])
        got = flags[batch.host_offsets[k] // 8 + 10 * np.arange(f0, nfr)]
        want = tr["flags"][f0:nfr, :4] @ np.array([1, 2, 4, 8])
        assert np.array_equal(got, want), f"{name}: speech flags differ at output frames {np.flatnonzero(got != want)[:8]}"
        c0 = res["ceps_cum"][k]
        for key, g in (("feat_cc", fcc), ("feat_pp", fpp)):
            a, b = _u32(g[c0:c0 + tr["nceps"]]), _u32(tr[key])
            assert np.array_equal(a, b), f"{name}: {int(np.sum(a != b))} of {b.size} words of {key} differ, first in cepstral frame {int(np.argmax((a != b).any(axis=1)))}"
        g15 = res["feats"][k]
        assert g15.shape == tr["vad_out"].shape, f"{name}: {g15.shape[0]} emitted frames, restatement {tr['vad_out'].shape[0]}"
        assert np.array_equal(g15[:, 14], tr["vad_out"][:, 14]), f"{name}: VAD column differs at {np.flatnonzero(g15[:, 14] != tr['vad_out'][:, 14])[:8]}"
        a, b = _u32(g15), _u32(tr["vad_out"])
        assert np.array_equal(a, b), f"{name}: {int(np.sum(a != b))} of {b.size} words of the emitted frames differ"
        assert np.array_equal(out[k], edge["ns"][u]["out_i16"]), f"{name}: int16 audio"
        words += want.size + 2 * tr["feat_cc"].size + b.size + out[k].size
    return words


def test_c_flags_and_feature_chain(edge):
    """(c) sea.afe_features_batch (the _fd kernels, WaveProc, CompCeps, PostProc, VAD, flush) against oracle.afe_trace:
    speech flags, VAD column and counts exact; feat_cc, feat_pp and the emitted frames bit for bit.  Twice: the edge batch
    alone (the six-wave _fd kernel) and inside a batch of more than two utterances per CU (the four-wave _fd kernel)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    middle, by_hang = _chain_conditions(edge)
    print(f"\n(c) {middle} cepstral frames with PostProc's weight inside (0, 1); VAD held by the hang-over of 50 in {by_hang}")
    assert middle >= 20 and by_hang
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    every = list(range(len(edge["utts"])))
    short = [u for u in every if edge["nfr"][u] <= 60]
    words = _check_chain(edge, sea, every, "six-wave _fd")
    words += _check_chain(edge, sea, every + [short[k % len(short)] for k in range(2 * n_cu + 1 - len(every))], "four-wave _fd")
    print(f"(c) {words} words (flag bytes, features, emitted frames, int16 samples) equal the restatement's")


def test_d_streaming_and_host_entries(edge, oracle):
    """(d) the same words as (a) from sea_ns_streams_push and sea_ns_streams_push_fd (float frames, two pushes, the shorter
    signals padded with zero frames, which the stream -- no gate -- processes), etsi_denoise per signal, one
    sea_denoise_utterances call and one sea_packed_* round over the whole list"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    utts, n = edge["utts"], len(edge["utts"])
    longest = max(edge["nfr"])
    x = np.zeros((n, longest, 80), np.float32)
    for u, s in enumerate(utts):
        x[u, : edge["nfr"][u]] = s.astype(np.float32).reshape(-1, 80)
    fr = torch.from_numpy(x).cuda()
    cut = 10                                                             # the `nbFrame < 10` rules change inside the second push
    o1, p1, st = sea.ns_streams_push(fr[:, :cut].contiguous())
    o2, p2, st = sea.ns_streams_push(fr[:, cut:].contiguous(), state=st, reset=False)
    q1, r1, st, f1, c1 = sea.ns_streams_push(fr[:, :cut].contiguous(), want_flags=True)
    q2, r2, st, f2, c2 = sea.ns_streams_push(fr[:, cut:].contiguous(), state=st, reset=False, want_flags=True)
    torch.cuda.synchronize()
    plain, fd = torch.cat([o1, o2], 1).cpu().numpy(), torch.cat([q1, q2], 1).cpu().numpy()
    prod = (np.arange(longest) >= 4).astype(np.int32)
    flags, counter = torch.cat([f1, f2], 1).cpu().numpy(), torch.cat([c1, c2], 1).cpu().numpy()
    words = 0
    for u in range(n):
        name, nfr, want = edge["names"][u], edge["nfr"][u], _u32(edge["ns"][u]["den_f32"])
        for what, o, p in (("sea_ns_streams_push", plain, torch.cat([p1, p2], 1)), ("sea_ns_streams_push_fd", fd, torch.cat([r1, r2], 1))):
            assert np.array_equal(p[u].cpu().numpy(), prod), f"{what}, {name}: produced"
            g = _u32(o[u, 4:nfr].reshape(-1))
            assert np.array_equal(g, want), f"{what}, {name}: {int(np.sum(g != want))} of {want.size} floats differ, first at frame {4 + int(np.argmax(g != want)) // 80}"
            words += want.size
        tf = edge["afe"][u]["flags"]
        assert np.array_equal(flags[u, :nfr], tf[:, :4] @ np.array([1, 2, 4, 8])), f"sea_ns_streams_push_fd, {name}: speech flags"
        assert np.array_equal(counter[u, :nfr], tf[:, 4]), f"sea_ns_streams_push_fd, {name}: frame counter"
        words += 2 * nfr
    # the padded tail too: the restatement's stream on the same padded frames (the floors hold while zeros keep coming)
    for u in range(n):
        want, wprod = oracle.ns_stream_f32(x[u])
        assert np.array_equal(_u32(plain[u, 4:].reshape(-1)), _u32(want)), f"sea_ns_streams_push, {edge['names'][u]}: the zero-padded tail"
        words += want.size

    for u, s in enumerate(utts):
        got = sea.etsi_denoise(s, fill=-7777)
        assert np.array_equal(got, edge["ns"][u]["out_i16"]), f"etsi_denoise, {edge['names'][u]}"
        words += got.size

    lens = [len(s) for s in utts]
    outs = [np.full(s.shape, 77, np.int16) for s in utts]
    pin = (ctypes.c_void_p * n)(*[s.ctypes.data for s in utts])
    po = (ctypes.c_void_p * n)(*[y.ctypes.data for y in outs])
    pl = (ctypes.c_long * n)(*lens)
    assert lib.sea_denoise_utterances(pin, po, pl, n) == 0, lib.sea_last_error()
    words += _check_ns(edge, outs, None, None, "sea_denoise_utterances")

    p = lib.sea_packed_create()
    assert p
    try:
        assert lib.sea_packed_plan(p, pl, n) == 0, lib.sea_last_error()
        K = lib.sea_packed_slices(p)
        assert K >= 1
        segs = []
        for u, s in enumerate(utts):
            qin, qout, cnt = (ctypes.c_void_p * K)(), (ctypes.c_void_p * K)(), (ctypes.c_long * K)()
            k = lib.sea_packed_segments(p, u, qin, qout, cnt, K)
            assert sum(cnt[i] for i in range(k)) == lens[u]
            pos = 0
            for i in range(k):
                dst = np.ctypeslib.as_array(ctypes.cast(qin[i], ctypes.POINTER(ctypes.c_short)), shape=(cnt[i],))
                dst[:] = s[pos:pos + cnt[i]]
                pos += cnt[i]
            segs.append((k, qout, cnt))
        assert lib.sea_packed_denoise(p) == 0, lib.sea_last_error()
        got = [np.concatenate([np.ctypeslib.as_array(ctypes.cast(qout[i], ctypes.POINTER(ctypes.c_short)), shape=(cnt[i],)) for i in range(k)])
               for k, qout, cnt in segs]
        words += _check_ns(edge, got, None, None, f"sea_packed_* ({K} slices)")
    finally:
        lib.sea_packed_destroy(p)
    print(f"\n(d) {words} words equal the restatement's over the two streaming entries, etsi_denoise, sea_denoise_utterances and sea_packed_*")


def test_e_ns16k_native(oracle):
    """(e) the float edge streams (sub-integer amplitudes included; both eps floors of filter_calc16, the latch, the SNR
    jump and averSNR <= 1e-5 occur: tests/test_edge_coverage_cpu.py) through sea_ns16k_streams_push in three pushes, an odd
    number of streams, against Ns16k.push"""
    import speech_enhancement_amd as sea
    from tests import ns_edge_cases as E
    from tests.test_gpu_ns16k import _compare
    torch = _torch()
    sig = E.streams_16k()
    names = list(sig)
    assert len(names) % 2 == 1
    nfr = max(len(s) // 160 for s in sig.values())
    x = np.zeros((len(names), nfr * 160), np.float32)                    # zero frames behind the shorter ones: the gate drops them
    for b, s in enumerate(sig.values()):
        x[b, : len(s)] = s
    want = [oracle.ns16k_new().push(x[b]) for b in range(len(x))]
    fr = torch.from_numpy(x.reshape(len(x), nfr, 160)).cuda()
    cuts = (0, 9, 57, nfr)                                               # inside the first ten frames; where dc_rise_small's second stage reaches its floor
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = sea.ns16k_streams_push(fr[:, a:b].contiguous(), state=state)
        state = r["state"]
        parts.append({k: v.cpu().numpy() for k, v in r.items() if k != "state"})
    torch.cuda.synchronize()
    total = 0
    for b, name in enumerate(names):
        got = {k: np.concatenate([p[k][b] for p in parts]) for k in parts[0]}
        total += _compare(got, want[b], nfr, name)
    print(f"\n(e) {total} output frames ({total * 185} words: samples and gains) of {len(names)} streams bit-identical")


def test_f_wideband():
    """(f) the quiet, onset, loud-then-zero and fade signals at 16 kHz and the wideband edge set (the noise floors of both
    bands, WaveProc without a neighbouring maximum, speech found by one measure alone, the flush's raised hang-over:
    tests/test_wb_edge_coverage_cpu.py) through the wideband mode and its feature chain, against the reference's own code
    (tests/wb_reference.py, tests/wb_afe_reference.py); every value bit for bit"""
    from tests import ns_edge_cases as E
    from tests import test_gpu_wb as WB
    from tests import test_gpu_wb_afe as WA
    _torch()
    W, A = WB._reference(), WA._reference()
    sig = E.signals_wb()
    names, utts = list(sig), list(sig.values())
    res, st = WB._run(utts), WB._Stats()
    for u, x in enumerate(utts):
        WB._compare(st, res[u], W.trace(x), len(x) // 160, names[u])
    st.report("(f) wideband mode")
    assert st.i16_diff == 0 and all(nb == 0 for _, _, nb in st.f.values()), "the wideband mode differs from the reference in bits"
    res, sa = WA._run(utts), WA._Stats()
    for u, x in enumerate(utts):
        WA._compare(sa, res[u], A.trace(x), len(x) // 160, names[u])
    sa.report("(f) wideband feature chain")
    assert all(nb == 0 for _, _, nb in sa.f.values()), "the wideband feature chain differs from the reference in bits"
    print(f"(f) {st.i16_n + sum(n for _, n, _ in st.f.values()) + sum(n for _, n, _ in sa.f.values()) + sum(sa.exact.values())} words compared")
