"""GPU tests of the 16 k-native NoiseSup variant (function/20141106_speech_enhancement/aurora_etsi/
NoiseSup.cpp:1140-1407 behind the etsi_denoise_mapping_* symbols), through the C ABI, bit for bit against
oracle/ns16k_oracle.c.  That oracle's transform / windows / IDCT / DoGamma are pinned against the reference's own
rfft.cpp + MelProc.cpp compiled here (tests/test_oracle.py); its frame loop is PARITY UNPINNED (NoiseSup.cpp needs the
absent aurora/aurora_include.h), so these tests show HIP == restatement, not HIP == reference, for the loop.
Run on an MI355X with ``pytest -m gpu``."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _streams(n_frames):
    """Six float streams of n_frames x 160: speech-like int16-valued signals as the reference's caller feeds them
    (aurora_etsi_test.cpp:52-55), leading zero frames, zero frames in the middle, a quiet one whose frames pass the gate
    only just (sum of squares around 1), a loud non-integer one, and amplitudes far outside int16."""
    from speech_enhancement_amd import corpus
    L = 160 * n_frames
    rng = np.random.default_rng(2024)
    s = [corpus.synth_utterance(21 + k, L).astype(np.float32) for k in range(6)]
    s[1] = corpus.synth_utterance(5, L).astype(np.float32)          # first 400 samples zero
    s[1][160 * 30:160 * 34] = 0.0
    s[2] = (rng.standard_normal(L) * 0.08).astype(np.float32)       # sum of squares per frame ~ 1.0: gate flips frame by frame
    s[3] = (s[3] * np.float32(3.7) + rng.standard_normal(L).astype(np.float32) * 300).astype(np.float32)
    s[4] = (s[4] * np.float32(1e6)).astype(np.float32)
    s[5] = (s[5] * np.float32(1e-3)).astype(np.float32)
    s[5][160 * 10:160 * 60] = 0.0                                    # long silence: state must not move
    return np.stack(s)


def _compare(got, want, n_frames, what):
    """got: dict of numpy arrays for one stream (GPU); want: Ns16k.push() result"""
    touched = want["counter"] != -7
    produced = want["out"].reshape(n_frames, 160)[:, 0] != -7.0
    produced |= np.any(want["out"].reshape(n_frames, 160) != -7.0, axis=1)
    assert np.array_equal(got["produced"].astype(bool), produced), f"{what}: produced"
    assert np.array_equal(got["counter"][touched], want["counter"][touched]), f"{what}: frame counter"
    assert np.all(got["counter"][~touched] == 0), f"{what}: counter where the first stage did not run"
    for bit, k in enumerate(("var", "spec", "mel", "vadns")):
        assert np.array_equal((got["flags"][touched] >> bit) & 1, want[k][touched]), f"{what}: {k}"
    go = got["out"].reshape(n_frames, 160)[produced]
    wo = want["out"].reshape(n_frames, 160)[produced]
    assert np.array_equal(_u32(go), _u32(wo)), f"{what}: {int(np.sum(_u32(go) != _u32(wo)))} of {go.size} output samples differ"
    gw = got["wiener"][produced]
    assert np.array_equal(_u32(gw), _u32(want["wiener"])), f"{what}: the 25 gains per second-stage frame"
    return int(produced.sum())


def test_ns16k_streams_vs_oracle_chunked(oracle):
    """sea_ns16k_streams_push on six streams in three pushes (the state blob carries the recursion), every output
    sample, flag, counter and gain row against the oracle's func_Wiener on the whole signal."""
    import speech_enhancement_amd as sea
    torch = _torch()
    nfr = 140
    x = _streams(nfr)
    want = [oracle.ns16k_new().push(x[b]) for b in range(len(x))]
    fr = torch.from_numpy(x.reshape(len(x), nfr, 160)).cuda()
    cuts = (0, 53, 54, nfr)
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = sea.ns16k_streams_push(fr[:, a:b].contiguous(), state=state)
        state = r["state"]
        parts.append({k: v.cpu().numpy() for k, v in r.items() if k != "state"})
    torch.cuda.synchronize()
    total = 0
    for b in range(len(x)):
        got = {k: np.concatenate([p[k][b] for p in parts]) for k in parts[0]}
        total += _compare(got, want[b], nfr, f"stream {b}")
    gated = [int(np.sum(w["counter"] == -7)) for w in want]
    print(f"ns16k: {total} output frames of {len(x) * nfr} bit-identical; frames without first-stage run per stream {gated}")
    assert gated[0] == 2 and gated[2] > 10 and gated[5] >= 50      # the gate cases really occur


def test_ns16k_state_blob_carries_the_stream_across_pushes(oracle):
    """The pipelined kernel (four waves per stream, two streams per workgroup: csrc/ns16k_pipe_kernel.hip) resumes from its
    state blob: a signal cut into two or more pushes, an ODD number of streams (the second stream slot of the last
    workgroup is padding), and pushes of one and two frames (shorter than the pipeline is deep) must all equal the oracle's
    func_Wiener on the whole signal."""
    import speech_enhancement_amd as sea
    torch = _torch()
    nfr = 90
    x = np.concatenate([_streams(nfr), _streams(nfr)[:1] * np.float32(0.5)])     # seven streams
    want = [oracle.ns16k_new().push(x[b]) for b in range(len(x))]
    fr = torch.from_numpy(x.reshape(len(x), nfr, 160)).cuda()
    for cuts in ((0, 41, nfr), (0, 1, 2, 4, 5, 40, nfr), (0, 3, 7, 8, 30, nfr)):
        state, parts = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            r = sea.ns16k_streams_push(fr[:, a:b].contiguous(), state=state)
            state = r["state"]
            parts.append({k: v.cpu().numpy() for k, v in r.items() if k != "state"})
        torch.cuda.synchronize()
        for b in range(len(x)):
            got = {k: np.concatenate([p[k][b] for p in parts]) for k in parts[0]}
            _compare(got, want[b], nfr, f"cuts {cuts} stream {b}")


def test_ns16k_device_pieces_vs_reference_fixture():
    """The pieces of the variant that the reference itself pins -- tests/golden/aurora_golden.npz = outputs of the reference's OWN
    aurora_etsi/rfft.cpp + MelProc.cpp compiled in the build container -- computed ON THE DEVICE by the functions the pipelined
    kernel's role waves call (sea_selftest_ns16k_pieces): rfft (x, 512, 8) from both of the transform wave's work areas,
    DoGamma, and rows 0..8 of DoGammaIDCT, bit for bit.  No oracle library in the loop; the twiddles are generated constants
    (csrc/ns16k_twiddles.inc), so the comparison does not depend on this box's libm."""
    import speech_enhancement_amd as sea
    _torch()
    lib = sea.load()
    g = np.load(os.path.join(GOLD, "aurora_golden.npz"))
    fr = np.ascontiguousarray(g["frames"], np.float32)
    gains = np.ascontiguousarray(g["gains"], np.float32)
    a, b = np.zeros_like(fr), np.zeros_like(fr)
    gam = np.zeros((len(gains), 25), np.float32)
    idct = np.zeros((len(gains), 9), np.float32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.sea_selftest_ns16k_pieces(P(fr), len(fr), P(a), P(b), P(gains), len(gains), P(gam), P(idct)) == 0, lib.sea_last_error()
    assert np.array_equal(_u32(a), _u32(g["rfft512_8"])) and np.array_equal(_u32(b), _u32(g["rfft512_8"])), "rfft (x, 512, 8)"
    assert np.array_equal(_u32(gam), _u32(g["do_gamma"])), "DoGamma"
    assert np.array_equal(_u32(idct), _u32(g["idct"][:, :9])), "DoGammaIDCT rows 0..8"


def test_ns16k_golden_no_oracle_in_the_loop():
    """The HIP path against the committed fixture tests/golden/ns16k_golden.npz (written by the restatement: a regression
    anchor, see oracle/gen_golden.py), no oracle library loaded.  Since round 4 the transform's twiddles are generated
    constants (csrc/ns16k_twiddles.inc), not the host libm's cosf / sinf at initialisation, so the product's output does not
    depend on the box: the comparison is unconditional (round 3 fell back to the live oracle and skipped on a differing libm)."""
    import speech_enhancement_amd as sea
    torch = _torch()
    g = np.load(os.path.join(GOLD, "ns16k_golden.npz"))
    for name in ("plain", "gated"):
        x = g[f"{name}/in"]
        n = len(x) // 160
        r = sea.ns16k_streams_push(torch.from_numpy(x[: n * 160].reshape(1, n, 160)).cuda())
        got = {k: v.cpu().numpy()[0] for k, v in r.items() if k != "state"}
        want = {k: g[f"{name}/{k}"] for k in ("out", "var", "spec", "mel", "vadns", "counter", "wiener")}
        _compare(got, want, n, name)

def test_etsi_denoise_mapping_symbols_16k_native(oracle, tmp_path):
    """The reference's batch plug-in symbols with sm_glb_res == NULL (what its caller passes,
    resyth_64sub_ori/cpp/aurora_etsi_test.cpp:20): the 16 k-native variant.  Two func_Wiener calls on one thread
    instance as that caller makes them (the state crosses the calls, :78, :128), output entries the reference leaves
    untouched stay untouched, and the FILE* receives the '%f ' lines of 25 gains (NoiseSup.cpp:1319-1328)."""
    import speech_enhancement_amd as sea
    _torch()
    lib = sea.load()
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]

    class In(ctypes.Structure):
        _fields_ = [("inData", ctypes.c_void_p), ("dataNum", ctypes.c_int)]

    class Out(ctypes.Structure):
        _fields_ = [("outData", ctypes.c_void_p), ("pSpeechFoundVar", ctypes.c_void_p), ("pSpeechFoundSpec", ctypes.c_void_p),
                    ("pSpeechFoundMel", ctypes.c_void_p), ("pSpeechFoundVADNS", ctypes.c_void_p), ("pFrameCounter", ctypes.c_void_p)]

    x = _streams(90)[1]
    nfr = len(x) // 160
    o = oracle.ns16k_new()
    cut = 37
    want = [o.push(x[:160 * cut]), o.push(x[160 * cut:])]
    glb, thd = ctypes.c_void_p(), ctypes.c_void_p()
    # a caller that passes a real DENOISEGlobalImpl {int SamplingFrequency} (NoiseSupExports.h:9-12) -- even one that says
    # 8000 -- gets what the reference gives it: the argument is ignored (aurora_etsi/NoiseSup.cpp:913-922)
    res = ctypes.c_int(8000)
    assert lib.etsi_denoise_mapping_global_init(ctypes.byref(glb), ctypes.byref(res)) == 1
    assert lib.etsi_denoise_mapping_thread_init(ctypes.byref(thd), glb) == 1
    out = np.full(nfr * 160, -7.0, np.float32)
    arrs = [np.full(nfr, -7, np.int32) for _ in range(5)]
    path = str(tmp_path / "x.wiener")
    fp = libc.fopen(path.encode(), b"w")
    assert fp
    for a, b in ((0, cut), (cut, nfr)):
        i = In(x[160 * a:].ctypes.data, 160 * (b - a) + (13 if b < nfr else 0))   # 13 samples beyond the last whole frame: ignored
        oo = Out(out[160 * a:].ctypes.data, *[v[a:].ctypes.data for v in arrs])
        assert lib.etsi_denoise_mapping_func_Wiener(glb, thd, ctypes.byref(i), ctypes.byref(oo), ctypes.c_void_p(fp)) == 0, lib.sea_last_error()
    libc.fclose(ctypes.c_void_p(fp))
    lib.etsi_denoise_mapping_thread_release(ctypes.byref(thd))
    lib.etsi_denoise_mapping_global_release(ctypes.byref(glb))
    assert not thd.value and not glb.value
    w_out = np.concatenate([w["out"] for w in want])
    assert np.array_equal(_u32(out), _u32(w_out)), "outData (untouched entries included)"
    for v, k in zip(arrs, ("var", "spec", "mel", "vadns", "counter")):
        assert np.array_equal(v, np.concatenate([w[k] for w in want])), k
    rows = np.concatenate([w["wiener"] for w in want])
    text = "".join("".join("%f " % v for v in row) + "\n" for row in rows)
    assert open(path).read() == text and len(rows) > 50
