"""Every device-pointer entry point on a side stream, behind a delay, after a decoy (tests/stream_cases.py has the protocol
and the table): the call's launches are all on the caller's stream, the call does not wait for it, and the bytes are those the
module's own test accepts.  Then two streams at once, and the launch-only chains captured in a graph and replayed on two inputs.

Each RUNS entry is the smallest case its module already proves: it launches through the module's helper or the Python layer
and asserts with the module's own comparison; variant "decoy" is the same utterances at other indices (the same sizes, another
answer everywhere).  One entry may cover several entry points (a producer and its consumer; the slices of one utterance list).
Run on an MI355X with ``pytest -m gpu``."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _torch():
    import torch
    return torch


def _sea():
    import speech_enhancement_amd as sea
    return sea


def _order(n, variant):
    """the indices of the true list in the order the variant holds them"""
    k = {"true": 0, "decoy": 1}[variant]
    return [S.rotated_index(i, n, k) for i in range(n)]


def _pick(items, variant):
    items = list(items)
    return [items[i] for i in _order(len(items), variant)]


def _fpack(utts):
    return _sea().PackedBatch.from_arrays([np.ascontiguousarray(x, np.float32) for x in utts], device=DEV, dtype=np.float32)


# ---- the Hu-Wang chain, both banks ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bank(n):
    sea = _sea()
    if n == 25:
        from tests import hw25_am_model as AM, hw25_model as M, hw25_pitch_model as PM
        from tests import test_gpu_hw25 as TF, test_gpu_hw25_am as TA, test_gpu_hw25_pitch as TP
        return SimpleNamespace(n=25, hop=80, M=M, PM=PM, AM=AM, TF=TF, TA=TA, TP=TP, g=M.load_golden(), front=sea.hw25_frontend_batch,
                               periph=sea.hw25_periphery_batch, gout=sea.hw25_periphery_gout_batch, corr=sea.hw25_correlogram_batch,
                               pitch=sea.hw25_pitch_batch, am=sea.hw25_am_batch, final=sea.hw25_finalseg_batch, ibm=sea.hw25_ibm_batch,
                               equal=lambda got, g, name, k: M.same_bits(np.ascontiguousarray(got), g[f"{name}_{k}"]))
    from tests import hw64_am_model as AM, hw64_model as M, hw64_pitch_model as PM
    from tests import test_gpu_hw64 as TF, test_gpu_hw64_am as TA, test_gpu_hw64_pitch as TP
    return SimpleNamespace(n=64, hop=160, M=M, PM=PM, AM=AM, TF=TF, TA=TA, TP=TP, g=M.load_golden(), front=sea.hw64_frontend_batch,
                           periph=sea.hw64_periphery_batch, gout=lambda b: sea.hw64_periphery_batch(b, gout=True),
                           corr=sea.hw64_correlogram_batch, pitch=sea.hw64_pitch_batch, am=sea.hw64_am_batch,
                           final=sea.hw64_finalseg_batch, ibm=sea.hw64_ibm_batch,
                           equal=lambda got, g, name, k: M.equals_golden(np.ascontiguousarray(got), g, name, k))


def hw_front(n, mode):
    """the fixture's 1770-sample (1210 at 8 kHz) inputs and its one-frame input; "group": the launch group, "two": the two calls"""
    def run(variant):
        b = _bank(n)
        keys = _pick("abcd", variant)
        batch = _fpack([b.g[f"x_{k}"] for k in keys])
        if mode == "group":
            res = b.front(batch, want_acf=True)
        else:
            hout, hev = b.periph(batch)[:2]
            res = b.corr(batch, hout, hev, want_acf=True)
        _torch().cuda.synchronize()
        for u, k in enumerate(keys):
            got = res.utterance(u)
            for name in b.TF.ARRAYS:
                assert b.equal(got[name], b.g, name, k), f"hw{n} {mode}, {k}: {name}"
    return run


def hw_pitch(n):
    def run(variant):
        b = _bank(n)
        g = b.PM.load_golden()
        keys = _pick(b.PM.AUDIO_CASES, variant)
        res = b.pitch(_fpack([g[f"x_{k}"] for k in keys]), stages=True)
        _torch().cuda.synchronize()
        for u, k in enumerate(keys):
            b.TP.assert_equal(res.utterance(u), b.TP._from_golden(g, k), f"hw{n}_pitch_batch, {k}")
    return run


def _check_am(b, g, got, k, what):
    tol = float(g["ratio_tol"])
    assert got["status"] == 0
    assert np.array_equal(got["amcrn"], g[f"amcrn_{k}"].astype(np.float32)), f"{what}, {k}: AmCrn"
    assert b.M.same_bits(np.ascontiguousarray(got["seng"]), g[f"seng_{k}"]), f"{what}, {k}: sEng"
    ref = g[f"ratio_{k}"]
    on = ref != 0
    assert np.array_equal(got["ratio"] != 0, on), f"{what}, {k}: the units where sinModel runs"
    assert (np.abs(got["ratio"][on].astype(np.float64) - ref[on]) / ref[on]).max() <= tol, f"{what}, {k}: ratio"
    for name in ("ampatt", "am"):
        b.TA._against_crcs(got[name], g, name, k)


def hw_am(n, grouped=False):
    """the periphery with gOut, then computeAM on the fixture's pitch; grouped: silent utterances behind the fixture's bring the
    padded extent to where the FFT runs in groups of channels"""
    def run(variant):
        torch = _torch()
        b = _bank(n)
        g = b.AM.load_golden()
        keys = _pick(b.AM.AUDIO_CASES, variant)
        utts = [g[f"x_{k}"] for k in keys]
        pitch = [g[f"pitch_{k}"] for k in keys]
        if grouped:
            quiet = 150000
            count = {25: 3, 64: 1}[n]
            utts += [np.zeros(quiet, np.float32)] * count
            pitch += [np.zeros(quiet // b.hop, np.int32)] * count
        batch = _fpack(utts)
        if grouped:
            lib = _sea().load()
            small = _fpack(utts[:len(keys)])
            fn = getattr(lib, f"sea_hw{n}_am_scratch_bytes")
            per = lambda bt: int(fn(int(bt.total), bt.n_utt)) / max(int(bt.total), 1)  # noqa: E731
            assert per(batch) < 0.5 * per(small), "the size rule did not select the channel groups"
        gout = b.gout(batch)[2]
        res = b.am(batch, gout, torch.from_numpy(np.concatenate(pitch).astype(np.int32)).to(DEV), want_details=True)
        torch.cuda.synchronize()
        blocks = b.TA._blocks(batch, gout)
        for u, k in enumerate(keys):
            b.TA._against_crcs(blocks[u][0], g, "gout", k)
            _check_am(b, g, res.utterance(u), k, f"hw{n}_am_batch")
    return run


def hw_finalseg(n):
    def run(variant):
        torch = _torch()
        b = _bank(n)
        g = b.AM.load_golden()
        keys = _pick(b.AM.AUDIO_CASES, variant)
        rows = np.array([g[f"grp_{k}"].shape[0] for k in keys], np.int64)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        inp = [dev(np.concatenate([g[f"{name}_{k}"].astype(np.float32) for k in keys])) for name in ("grp", "amcrn", "cross_ev", "pratio")]
        offs = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
        res = b.final(*inp, dev(rows * b.hop + 7), dev(offs), rows, stages=True)
        torch.cuda.synchronize()
        for u, k in enumerate(keys):
            got = res.utterance(u)
            assert got["status"] == 0
            for name in b.AM.FINAL_STAGES + ("grp_final", "mask"):
                assert np.array_equal(got[name], g[f"{name}_{k}"].astype(np.float32)), f"hw{n}_finalseg_batch, {k}: {name}"
    return run


def hw_ibm(n):
    def run(variant):
        b = _bank(n)
        g = b.AM.load_golden()
        keys = _pick(b.AM.AUDIO_CASES, variant)
        res = b.ibm(_fpack([g[f"x_{k}"] for k in keys]), stages=True)
        _torch().cuda.synchronize()
        for u, k in enumerate(keys):
            got = res.utterance(u)
            assert np.array_equal(got["mask"], g[f"mask_{k}"].astype(np.float32)), f"hw{n}_ibm_batch, {k}: the mask is not createIBM's"
            assert np.array_equal(got["pitch"], g[f"pitch_{k}"]) and got["status"] >> 16 == 0 and got["status"] > 0, k
            for name in b.AM.FINAL_STAGES:
                assert np.array_equal(got[name], g[f"{name}_{k}"].astype(np.float32)), f"hw{n}_ibm_batch, {k}: {name}"
    return run


def hw25_resynth(variant):
    from tests import hw25_am_model as AM, hw25_model as M, hw25_resynth_model as RM, test_gpu_hw25_resynth as TR
    g, xs = RM.load_golden(), AM.audio_inputs()
    keys = _pick(RM.AUDIO_CASES, variant)
    batch = TR._pack([xs[k] for k in keys])
    got, _ = TR.launch(batch, TR._gout(batch), [g[f"mask_a_{k}"].astype(np.float32) for k in keys])
    for u, k in enumerate(keys):
        assert M.same_bits(got[u], g[f"out_a_{k}"]), f"{k}: not the reference's resynthesis"


def hw25_enhance(variant):
    from tests import hw25_am_model as AM, hw25_model as M, hw25_resynth_model as RM, test_gpu_hw25_resynth as TR
    g, am, xs = RM.load_golden(), AM.load_golden(), AM.audio_inputs()
    keys = _pick(RM.AUDIO_CASES, variant)
    res = _sea().hw25_enhance_batch(TR._pack([xs[k] for k in keys]))
    _torch().cuda.synchronize()
    for u, k in enumerate(keys):
        got = res.utterance(u)
        assert np.array_equal(got["mask"], am[f"mask_{k}"].astype(np.float32)), f"{k}: the mask is not createIBM's"
        assert M.same_bits(got["audio"], g[f"out_a_{k}"]), f"{k}: audio in, enhanced audio out is not the reference's"
        assert got["status"] >> 16 == 0


RUNS = {
    "hw25_group": hw_front(25, "group"), "hw25_two": hw_front(25, "two"), "hw64_group": hw_front(64, "group"),
    "hw64_two": hw_front(64, "two"), "hw25_pitch": hw_pitch(25), "hw64_pitch": hw_pitch(64), "hw25_am": hw_am(25), "hw64_am": hw_am(64),
    "hw25_finalseg": hw_finalseg(25), "hw64_finalseg": hw_finalseg(64), "hw25_ibm": hw_ibm(25), "hw64_ibm": hw_ibm(64),
    "hw25_resynth": hw25_resynth, "hw25_enhance": hw25_enhance,
}
# the same calls at the size where am_launch takes its other path (no table row of their own)
EXTRA_RUNS = {"hw25_am_grouped": hw_am(25, grouped=True), "hw64_am_grouped": hw_am(64, grouped=True)}


# ---- the ETSI front end: NoiseSup, cepstra, the feature chain, both rates --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    return O.Oracle()


def ns_short(variant):
    """a ragged utterance, one shorter than a frame, an EMPTY one, an all-zero one and a whole one, against the oracle"""
    from tests import test_gpu_parity as TP
    TP.test_ns_batch_vs_oracle(_oracle(), utts=_pick(TP._mixed_corpus()[:5], variant))


def ns_chain(variant):
    from tests import test_gpu_golden as TG
    TG.test_golden_noisesup_batch_int16_float_stream_and_cepstra(names=_pick(TG.NAMES, variant))


def afe_chain(variant):
    from tests import test_gpu_golden as TG
    TG.test_golden_afe_feature_chain(names=_pick(TG.NAMES, variant))


def _golden(name):
    from tests import test_gpu_golden as TG
    import os
    return np.load(os.path.join(TG.GOLD, name))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rfft256(variant):
    torch = _torch()
    g = _golden("rfft_golden.npz")
    rows = _order(len(g["frames"]), variant)
    got = _sea().rfft_batch(torch.from_numpy(g["frames"][rows]).cuda()).cpu().numpy()
    assert np.array_equal(_u32(got), _u32(g["rfft"][rows]))


def rfft_any(variant):
    """rfft (x, 512, 8), the variant's transform, and a small and a large size: the schedule walker, in place"""
    torch = _torch()
    g = _golden("rfft_sizes_golden.npz")
    for n, m in ((512, 8), (16, 4), (4096, 12)):
        x, want = g[f"in_{n}_{m}"], g[f"out_{n}_{m}"]
        rows = _order(len(x), variant)
        got = _sea().rfft_any_batch(torch.from_numpy(x[rows]).cuda(), m).cpu().numpy()
        assert np.array_equal(_u32(got), _u32(want[rows])), f"sea_rfft_batch, rfft (x, {n}, {m})"


def compceps_frames(variant):
    torch = _torch()
    g = _golden("compceps_golden.npz")
    rows = _order(len(g["data201"]), variant)
    got = _sea().compceps_frames(torch.from_numpy(g["data201"][rows]).cuda()).cpu().numpy()
    assert float(np.abs(got - g["coef"][rows]).max()) <= 1e-3
    assert np.array_equal(_u32(got), _u32(g["coef"][rows]))


def wb_chain(variant):
    from tests import test_gpu_wb as W
    with np.load(W.GOLD) as z:
        g = {k: z[k] for k in z.files}
    ids = _pick(range(6), variant)
    res = W._run([g[f"x{i}"] for i in ids])
    st = W._Stats()
    for u, i in enumerate(ids):
        want = dict(out_i16=g[f"out{i}"], hp=g[f"hp{i}"], code=g[f"code{i}"], ceps=g[f"ceps{i}"],
                    first_out=int(g["first_out"][i]), onset=int(g["onset"][i]))
        if f"f32_{i}" in g:
            want["f32"] = g[f"f32_{i}"]
        W._compare(st, res[u], want, len(g[f"x{i}"]) // 160, f"fixture utterance {i}", f32=f"f32_{i}" in g)
    st.check()


def wb_afe_chain(variant):
    from tests import test_gpu_wb_afe as W
    g = W._fixture()
    ids = _pick(range(W.N_FIXTURE), variant)
    res = W._run([g[f"x{i}"] for i in ids])
    st = W._Stats()
    for u, i in enumerate(ids):
        want = dict(feat_cc=g[f"feat_cc{i}"], feat_pp=g[f"feat_pp{i}"], feat15=g[f"feat15_{i}"], flags=g[f"flags{i}"],
                    first_out=int(g["first_out"][i]), onset=int(g["onset"][i]))
        W._compare(st, res[u], want, len(g[f"x{i}"]) // 160, f"fixture utterance {i}")
    st.check()


def _negated(utts):
    """the slice drivers want the list longest first, so their decoy keeps the order: every sample negated"""
    return [(-np.clip(x.astype(np.int32), -32767, 32767)).astype(x.dtype) for x in utts]


def _slice_run(data, body):
    """data(variant) -> whatever body needs, computed OUTSIDE the recording (run.pre): the one launch is the yardstick"""
    cached = functools.lru_cache(maxsize=None)(data)

    def run(variant):
        body(*cached(variant))
    run.pre = lambda: [cached(v) for v in ("true", "decoy")]
    return run


def ceps_slices(wb):
    """the fixtures of the rate in four time slices, the denoiser's slice call and the cepstrum's per slice, all launches back
    to back: rows, counts and audio are the one launch's"""
    def data(variant):
        from tests import test_gpu_ceps_slices as C
        names, utts, want, _ = C._fixtures(wb)
        if variant == "decoy":
            utts = _negated(utts)
            want = C._one_launch(utts, wb)
        return C, names, utts, want

    def body(C, names, utts, want):
        got = C._in_slices(len(utts), C._cuts(utts, (0, 5, 22, 98, 400), C._hop(wb)), wb)
        for j, name in enumerate(names):
            C._assert_equal(got[j], want[j], name)
    return _slice_run(data, body)


def afe_slices(wb):
    def data(variant):
        if wb:
            from tests import test_gpu_wb_afe_slices as A
        else:
            from tests import test_gpu_afe_slices as A
        utts, want = A._fixture_one_launch()[-2:]
        if variant == "decoy":
            utts = _negated(utts)
            want = A._one_launch(utts)
        return A, utts, want

    def body(A, utts, want):
        got = A._in_slices(len(utts), A._cuts(utts, (0, 5, 16, 97, A.BOUNDS[-1])))
        for j in range(len(utts)):
            A._assert_features_equal(got[j], want[j], f"utterance {j}")
    return _slice_run(data, body)


def _push_cuts(x, push, check):
    """x [B, nfr, hop] in three pushes with the state carried on the device; check(per-key concatenated numpy arrays)"""
    torch = _torch()
    fr = torch.from_numpy(x).cuda()
    nfr = x.shape[1]
    cuts = (0, nfr // 4, nfr // 4 + 1, nfr)
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = push(fr[:, a:b].contiguous(), state)
        state = r.pop("state")
        parts.append(r)
    torch.cuda.synchronize()
    check({k: np.concatenate([p[k].cpu().numpy() for p in parts], axis=1) for k in parts[0]})


@functools.lru_cache(maxsize=None)
def _ns_streams():
    from speech_enhancement_amd import corpus
    xs = [corpus.synth_utterance(21 + k, 80 * 48) for k in range(3)]
    o = _oracle()
    return xs, [o.ns_trace(x, want_state=False)["den_f32"] for x in xs], [o.afe_trace(x)["flags"] for x in xs]


def ns_push(fd):
    def run(variant):
        sea = _sea()
        xs, den, flags = (_pick(a, variant) for a in _ns_streams())

        def push(frames, state):
            r = sea.ns_streams_push(frames, state=state, reset=None if state is None else False, want_flags=fd)
            return dict(zip(("out", "produced", "state", "flags", "counter"), r))

        def check(got):
            for b in range(len(xs)):
                assert np.array_equal(got["produced"][b], (np.arange(48) >= 4).astype(np.int32))
                assert np.array_equal(_u32(got["out"][b, 4:].reshape(-1)), _u32(den[b])), f"stream {b}: not the oracle's DoNoiseSup"
                if fd:
                    assert np.array_equal(got["flags"][b], flags[b][:, :4] @ np.array([1, 2, 4, 8])), f"stream {b}: flags"
                    assert np.array_equal(got["counter"][b], flags[b][:, 4]), f"stream {b}: frame counter"
        _push_cuts(np.stack(xs).astype(np.float32).reshape(len(xs), 48, 80), push, check)
    run.pre = _ns_streams
    return run


@functools.lru_cache(maxsize=None)
def _ns16k_streams():
    from tests import test_gpu_ns16k as N
    x = N._streams(60)
    return N, x, [_oracle().ns16k_new().push(x[b]) for b in range(len(x))]


def ns16k_push(variant):
    N, x, want = _ns16k_streams()
    rows = _order(len(x), variant)

    def push(frames, state):
        return dict(_sea().ns16k_streams_push(frames, state=state))

    def check(got):
        for b, i in enumerate(rows):
            N._compare({k: v[b] for k, v in got.items()}, want[i], 60, f"stream {i}")
    _push_cuts(np.ascontiguousarray(x[rows]).reshape(len(x), 60, 160), push, check)


ns16k_push.pre = _ns16k_streams


# ---- resynthesis, subbands, IRM, the training-set builder ------------------------------------------------------------------------
_RESTATED = {}


def _restated(kind, name, fn):
    """the oracle's restatement of one case, computed once"""
    if (kind, name) not in _RESTATED:
        _RESTATED[kind, name] = fn()
    return _RESTATED[kind, name]


def subband64(variant):
    from tests import resynth_model_cases as C
    sea = _sea()
    cases = _pick(C.subband_cases(), variant)
    batch = sea.PackedBatch.from_arrays([x for _, x, _ in cases])
    out = sea.subband_batch(batch)
    _torch().cuda.synchronize()
    host = out.cpu().numpy()
    for u, (name, x, _) in enumerate(cases):
        pitch = (len(x) + 7) // 8 * 8
        off = int(batch.host_offsets[u]) * 64
        blk = np.ascontiguousarray(host[off: off + 64 * pitch].reshape(64, pitch)[:, :len(x)])
        assert np.array_equal(blk, _restated("subband", name, lambda: _oracle().subband64(x))), f"{name}: differs from the restatement"


def resynth64(variant):
    from tests import resynth_model_cases as C
    sea = _sea()
    cases = _pick(C.resynth_cases(False), variant)
    batch = sea.PackedBatch.from_arrays([x for _, x, _, _ in cases])
    out, _ = sea.resynth_batch(batch, sea.MaskBatch.from_arrays([m for _, _, m, _ in cases]), binary=False)
    _torch().cuda.synchronize()
    for (name, x, mask, _), got in zip(cases, batch.split(out)):
        want = _restated("resynth", name, lambda: _oracle().resynth64(x, mask, binary=False, frames_l_over_160=False))
        assert np.array_equal(got, want), f"{name}: differs from the restatement"


@functools.lru_cache(maxsize=None)
def _irm_cases():
    from tests import irm_cases as C, irm_model as M
    mine = [c for c in C.cases(_oracle()) if c[3] == 1]
    return mine, {c[0]: M.irm(c[1], c[2], 1) for c in mine}


def irm(variant):
    from tests import test_gpu_irm as TI
    mine, models = _irm_cases()
    mine = _pick(mine, variant)
    rc, per_utt, _, _ = TI._launch(mine, 1)
    assert rc == 0
    for c, rows in zip(mine, per_utt):
        TI._check(c[0], rows, models[c[0]], {}, c[4])


irm.pre = _irm_cases


@functools.lru_cache(maxsize=None)
def _mix_setup(variant):
    from tests import addnoise_model as M
    recs, cs = M.recordings(), _pick(M.cases(), variant)
    src, base = M.noise_layout(recs)
    return dict(recs=recs, cases=cs, src=src, want=[M.addnoise(c["clean"], M.stretch(recs, c), c["db"]) for c in cs],
                start=np.array([base[c["rec"]] + c["off"] for c in cs], np.int64), db=np.array([c["db"] for c in cs], np.int32))


def addnoise(variant):
    from tests import test_gpu_trainset as TT
    sea = _sea()
    s = dict(_mix_setup(variant))
    s["batch"] = sea.PackedBatch.from_arrays([c["clean"] for c in s["cases"]])
    res = sea.addnoise_batch(s["batch"], s["src"], s["start"], s["db"])
    _torch().cuda.synchronize()
    TT._check_audio(s, res, "addnoise_batch")


def trainset(variant):
    from tests import test_gpu_trainset as TT
    sea = _sea()
    s = dict(_mix_setup(variant))
    s["batch"] = sea.PackedBatch.from_arrays([c["clean"] for c in s["cases"]])
    s["full"] = sea.trainset_batch(s["batch"], s["src"], s["start"], s["db"], window=1, noisy_subband=True)
    _torch().cuda.synchronize()
    TT._check_audio(s, s["full"], "trainset_batch")
    TT.test_trainset_batch_irm_vs_oracle(s, _oracle())


addnoise.pre = trainset.pre = lambda: [_mix_setup(v) for v in ("true", "decoy")]

RUNS.update({
    "ns_short": ns_short, "ns_chain": ns_chain, "afe_chain": afe_chain, "rfft256": rfft256, "rfft_any": rfft_any,
    "compceps_frames": compceps_frames, "wb_chain": wb_chain, "wb_afe_chain": wb_afe_chain, "ceps_slices_8k": ceps_slices(False),
    "ceps_slices_wb": ceps_slices(True), "afe_slices_8k": afe_slices(False), "afe_slices_wb": afe_slices(True),
    "ns_push": ns_push(False), "ns_push_fd": ns_push(True), "ns16k_push": ns16k_push, "subband64": subband64, "resynth64": resynth64,
    "irm": irm, "addnoise": addnoise, "trainset": trainset,
})

# sea_trainset_batch reads the lengths back before it launches (one stream synchronisation, stated in the header): the one
# entry point that waits for its stream and that a graph cannot capture
SYNCHRONISES = {"sea_trainset_batch"}


# ---- the tests --------------------------------------------------------------------------------------------------------------------
_DRIVEN = {}


def _prepared(run_name):
    run = {**RUNS, **EXTRA_RUNS}[run_name]
    if hasattr(run, "pre"):
        run.pre()
    return S.Case(run).prepare()


def _driven(run_name):
    """the run through the whole protocol, once per session: (the case, what it raised)"""
    if run_name not in _DRIVEN:
        case, err = None, None
        try:
            case = _prepared(run_name)
            case.enqueue()
            case.verify()
        except Exception as e:  # kept for every entry point that shares the run
            err = e
        _DRIVEN[run_name] = (case, err)
    case, err = _DRIVEN[run_name]
    if err is not None:
        raise err
    return case


def _control(on_side):
    """the protocol with a torch operation in the call's place -> (the stream was pending, the result equals the true one's)"""
    torch = _torch()
    S.calibrate()
    true = torch.arange(1 << 20, dtype=torch.float32, device=DEV)
    want = true + 1
    buf, out = torch.zeros_like(true), torch.zeros_like(true)
    torch.add(buf, 1, out=out)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        S.enqueue_delay(S.MIN_DELAY_MS)
        out.fill_(-7)
        buf.copy_(true)
        if on_side:
            torch.add(buf, 1, out=out)
    if not on_side:
        torch.add(buf, 1, out=out)  # on the default stream, while (a)-(c) are pending on s: it reads the stale input
    pending = not s.query()
    s.synchronize()
    torch.cuda.synchronize()
    return pending, bool(torch.equal(out, want))


def test_control_an_operation_on_the_default_stream_is_caught():
    pending, equal = _control(on_side=False)
    assert pending, "the delay was over before the operation was issued: the protocol's delay is too short"
    assert not equal, "an operation issued on the default stream came back equal: side streams here order against it"


def test_control_an_operation_on_the_side_stream_passes():
    pending, equal = _control(on_side=True)
    assert pending and equal


@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_entry_point_on_a_side_stream(name):
    case = _driven(S.TABLE[name].prepare)
    print(f"\n{name} [{S.TABLE[name].prepare}]: {case.report()}")
    assert name in case.true.names(), f"the run made no call of {name}: {sorted(set(case.true.names()))}"
    assert case.stale_rejected
    if name not in SYNCHRONISES:
        assert case.pending, "the stream was idle when the call returned: the call waited for it (or the delay is too short)"


@pytest.mark.parametrize("run_name", sorted(EXTRA_RUNS))
def test_am_launch_on_its_grouped_fft_path(run_name):
    case = _driven(run_name)
    print(f"\n{run_name}: {case.report()}")
    assert case.stale_rejected and case.pending


def test_two_streams_at_once():
    """sea_hw64_ibm_batch on one stream, sea_ns_denoise_batch + sea_compceps_batch on another, each behind its own delay with
    buffers of its own: no hidden device buffer is shared"""
    a, b = _prepared("hw64_ibm"), _prepared("ns_chain")
    assert "sea_hw64_ibm_batch" in a.true.names() and b.true.names() == ["sea_ns_denoise_batch", "sea_compceps_batch"]
    a.enqueue()
    b.enqueue()
    assert a.pending and b.pending and not a.stream.query()
    a.verify()
    b.verify()


# sea_wb_denoise_batch (a memset node before its kernels) is not among them: see DESIGN.md section 3
GRAPHS = {"sea_ns_denoise_batch": "ns_chain", "sea_afe_features_batch": "afe_chain",
          "sea_hw25_ibm_batch": "hw25_ibm", "sea_hw25_enhance_batch": "hw25_enhance", "sea_hw64_ibm_batch": "hw64_ibm",
          "sea_resynth64_batch": "resynth64"}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_capture_replays_on_two_inputs(name):
    """the chain captured once on a side stream over static buffers, replayed for A and for B (other data, other device-side
    lengths and offsets, the same n_utt and totals), outputs and scratch poisoned on the replay's stream before each"""
    torch = _torch()
    case = _prepared(GRAPHS[name])  # its warm run is the eager warm-up
    assert name in case.true.names()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        S.replay(case.true, torch.cuda.current_stream().cuda_stream)
    for variant in ("true", "decoy", "true"):
        with torch.cuda.stream(s):
            case.load(variant)
            graph.replay()
        s.synchronize()
        S.substitute(case.true, lambda: case.run(variant))


# ---- what the fixture-borne runs expect, on the CPU (tests/test_streams_cpu.py: the decoy's differs at every index) ---------------
def _per_key(path_or_g, keys, names, fmt="{name}_{key}"):
    g = np.load(path_or_g) if isinstance(path_or_g, str) else path_or_g
    return [{n: g[fmt.format(name=n, key=k)] for n in names} for k in keys]


def _hw_expected(n, what):
    if n == 25:
        from tests import hw25_am_model as AM, hw25_model as M, hw25_pitch_model as PM
        from tests.test_gpu_hw25 import ARRAYS
    else:
        from tests import hw64_am_model as AM, hw64_model as M, hw64_pitch_model as PM
        from tests.test_gpu_hw64 import ARRAYS
    if what == "front":  # the ACFs of the 64-band fixture lie in files of their own: the frame arrays stand for them
        return _per_key(M.load_golden(), "abcd", [a for a in ARRAYS if not a.startswith("acf")])
    if what == "pitch":
        return _per_key(PM.load_golden(), PM.AUDIO_CASES, ("pitch", "pratio", "grp") + PM.PITCH_STAGES + PM.GRP_STAGES)
    names = dict(am=("amcrn", "seng", "ratio"), finalseg=AM.FINAL_STAGES + ("grp_final", "mask"), ibm=AM.FINAL_STAGES + ("mask", "pitch"))
    return _per_key(AM.load_golden(), AM.AUDIO_CASES, names[what])


def _ns_expected(path, names):
    from tests import test_gpu_golden as TG
    import os
    g = np.load(os.path.join(TG.GOLD, path))
    return [{n: g[f"{name}/{n}"] for n in names} for name in TG.NAMES]


def _resynth25_expected():
    from tests import hw25_resynth_model as RM
    return _per_key(RM.load_golden(), RM.AUDIO_CASES, ("out_a", "mask_a"))


def _numbered(module, count, names):
    with np.load(module.GOLD) as z:
        return [{n: z[f"{n}{i}"] for n in names} for i in range(count)]


def _wb_expected():
    from tests import test_gpu_wb as W
    return _numbered(W, 6, ("out", "hp", "code", "ceps"))


def _wb_afe_expected():
    from tests import test_gpu_wb_afe as W
    return _numbered(W, W.N_FIXTURE, ("feat_cc", "feat_pp", "feat15_", "flags"))


def _rows_expected(path, key):
    return [{key: row} for row in _golden(path)[key]]


EXPECTED = {
    "hw25_group": lambda: _hw_expected(25, "front"), "hw25_two": lambda: _hw_expected(25, "front"),
    "hw64_group": lambda: _hw_expected(64, "front"), "hw64_two": lambda: _hw_expected(64, "front"),
    "hw25_pitch": lambda: _hw_expected(25, "pitch"), "hw64_pitch": lambda: _hw_expected(64, "pitch"),
    "hw25_am": lambda: _hw_expected(25, "am"), "hw64_am": lambda: _hw_expected(64, "am"),
    "hw25_finalseg": lambda: _hw_expected(25, "finalseg"), "hw64_finalseg": lambda: _hw_expected(64, "finalseg"),
    "hw25_ibm": lambda: _hw_expected(25, "ibm"), "hw64_ibm": lambda: _hw_expected(64, "ibm"),
    "hw25_resynth": _resynth25_expected, "hw25_enhance": _resynth25_expected,
    "ns_chain": lambda: _ns_expected("ns_golden.npz", ("etsi_denoise", "den_f32", "ceps")),
    "afe_chain": lambda: _ns_expected("afe_golden.npz", ("flags", "feat_cc", "feat_pp", "vad_out")),
    "wb_chain": _wb_expected, "wb_afe_chain": _wb_afe_expected,
    "rfft256": lambda: _rows_expected("rfft_golden.npz", "rfft"), "compceps_frames": lambda: _rows_expected("compceps_golden.npz", "coef"),
    "rfft_any": lambda: _rows_expected("rfft_sizes_golden.npz", "out_512_8"),
}


def test_zz_trainset_capture_is_refused_cleanly():
    """The stated exception: sea_trainset_batch reads the lengths back and synchronises its stream before
    it launches, which a capturing stream cannot do.  The call sees the capture and returns non-zero before it touches the
    stream: the capture stays valid and ends normally (empty), and the same call runs on a side stream afterwards."""
    torch = _torch()
    lib = _sea().load()
    case = _prepared("trainset")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        with pytest.raises(AssertionError, match="sea_trainset_batch returned"):
            S.replay(case.true, torch.cuda.current_stream().cuda_stream)
    said = lib.sea_last_error().decode(errors="replace")
    assert "cannot be captured" in said, said
    torch.cuda.synchronize()
    case.enqueue()
    case.verify()
