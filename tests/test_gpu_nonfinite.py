"""GPU tests of the float-taking entry points on Inf, NaN and finite floats whose energy overflows (tests/nonfinite_cases.py),
through the C ABI, against the restatement under nonfinite_cases.same_words: finite words and infinities bit for bit, NaNs by
position, integers equal, no tolerance.  tests/test_nonfinite_cpu.py pins the restatement to the reference on the same inputs
(the 16 k-native variant's frame loop excepted: PARITY UNPINNED, so its test shows HIP == restatement only).

These are tests of VALUES.  Their precondition is the audit of DESIGN.md section 3: no integer index, loop bound or address
of the kernels behind these entry points derives from an input float except the logarithm's table index, which is 0..255 for
every bit pattern.  Output buffers start as sentinels and carry guard rows.  Run on an MI355X with ``pytest -m gpu``."""
import ctypes
import functools

import numpy as np
import pytest

from tests import nonfinite_cases as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_F32, SENT_INT = -7777.25, -77
GUARD = 3


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return torch


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _is_sent(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return bool((a.view(np.uint32) == np.float32(SENT_F32).view(np.uint32)).all())
    return bool((a.astype(np.int64) == (SENT_INT & 0xFF if a.dtype == np.uint8 else SENT_INT)).all())


def _full(shape, dtype):
    torch = _torch()
    if dtype == torch.float32:
        return torch.full(shape, SENT_F32, dtype=dtype, device=DEV)
    return torch.full(shape, SENT_INT & 0xFF if dtype == torch.uint8 else SENT_INT, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ the logarithm forms
def test_selftest_log_nonfinite():
    """The three logarithm forms as the float-intake kernels instantiate them, on +Inf, -Inf and NaN patterns of both signs
    and several payloads -- against the EXPECTED float (libm: log (+Inf) = +Inf, log (NaN) = NaN, log (-Inf) = NaN; the
    sites' expressions 0.5 + (L / ln 2) 16 and 20 L / 3 keep both), not against the slow form, which reads bit patterns
    too -- and on finite arguments, where they must be the plain forms bit for bit."""
    import speech_enhancement_amd as sea
    _torch()
    lib = sea.load()
    nonfin = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000],
                      np.uint32).view(np.float32)
    fin = np.array([64.0, 65.0, 1e5, 3e19, 3.4028234663852886e38, 2e-5, 1.0, 0.99999994, 1.4142135, 1.4142137], np.float32)
    x = np.concatenate([nonfin, fin])
    s1, s2, lg = (np.full(x.size, SENT_F32, np.float32) for _ in range(3))
    assert lib.sea_selftest_log_nonfinite(x.ctypes.data, s1.ctypes.data, s2.ctypes.data, lg.ctypes.data, x.size) == 0, lib.sea_last_error()
    for name, got in (("site 1", s1), ("site 2", s2), ("logf", lg)):
        assert got[0].view(np.uint32) == 0x7F800000, f"{name} (+Inf) = {got[0]}"
        assert np.isnan(got[1:len(nonfin)]).all(), f"{name} on -Inf and the NaN patterns: {got[1:len(nonfin)]}"
    p1, p2 = (np.zeros(fin.size, np.float32) for _ in range(2))
    assert lib.sea_selftest_log_sites(fin.ctypes.data, p1.ctypes.data, p2.ctypes.data, fin.size) == 0, lib.sea_last_error()
    ok1, ok2 = fin >= 64.0, fin.astype(np.float64) > 0.00001
    assert np.array_equal(s1[len(nonfin):][ok1].view(np.uint32), p1[ok1].view(np.uint32))
    assert np.array_equal(s2[len(nonfin):][ok2].view(np.uint32), p2[ok2].view(np.uint32))
    want = np.log(fin.astype(np.float64))
    assert np.all(np.abs(lg[len(nonfin):].astype(np.float64) - want) <= np.abs(want) * 2.0 ** -23 + 1e-45)   # (float) of a < 1 ulp double log


# ------------------------------------------------------------------------------------------------ 8 kHz streams
@functools.lru_cache(maxsize=None)
def _batch_8k():
    base, s = N.streams_8k()
    order = N.batch_order(sorted(s), 3)
    return base, s, order, np.stack([base if n is None else s[n] for n in order])


_WANT_8K = {}


def _want_8k(oracle):
    """per stream of the batch: (out [nout * 80], produced, flags, counter) from the restatement, computed once"""
    if not _WANT_8K:
        base, s, order, _ = _batch_8k()
        solo = {None: oracle.ns_stream_f32_fd(base)}
        for n in s:
            solo[n] = oracle.ns_stream_f32_fd(s[n])
            plain = oracle.ns_stream_f32(s[n])
            assert N.same_words(solo[n][0], plain[0]) and np.array_equal(solo[n][1], plain[1])
        _WANT_8K["solo"] = solo
        # preconditions: the overflow matters (another output than with 1e18 in the sample's place), and the batch is built
        # as case d asks: clean copies between poisoned streams
        for n in (k for k in s if k.startswith("a/")):
            assert not N.same_words(solo[n][0], oracle.ns_stream_f32(N.a_control(s[n], n))[0]), f"{n}: same output as with 1e18"
        assert order.count(None) == 3 and order[0] is not None and order[-1] is not None
    return _WANT_8K["solo"]


def _push_8k(x, fd, state=None, reset=True):
    """sea_ns_streams_push / _fd on x [B][n][80] into sentinel-filled buffers with guard rows -> numpy dict + the state tensor"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    B, n, _ = x.shape
    fr = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = _full((B + GUARD, n, 80), torch.float32)
    prod = _full((B + GUARD, n), torch.int32)
    flags = _full((B + GUARD, n), torch.uint8) if fd else None
    ctr = _full((B + GUARD, n), torch.int32) if fd else None
    if state is None:
        state = torch.zeros((B, lib.sea_ns_state_floats()), dtype=torch.float32, device=DEV)
    if fd:
        rc = lib.sea_ns_streams_push_fd(_p(fr), _p(out), _p(prod), _p(flags), _p(ctr), _p(state), B, n, int(reset), None)
    else:
        rc = lib.sea_ns_streams_push(_p(fr), _p(out), _p(prod), _p(state), B, n, int(reset), None)
    assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    r = dict(out=out.cpu().numpy(), produced=prod.cpu().numpy())
    if fd:
        r.update(flags=flags.cpu().numpy(), counter=ctr.cpu().numpy())
    for k, v in r.items():
        assert _is_sent(v[B:]), f"{k}: guard rows behind the last stream were written"
        r[k] = v[:B]
    assert np.array_equal(fr.cpu().numpy().view(np.uint32), np.ascontiguousarray(x).view(np.uint32)), "the input was modified"
    return r, state


def _check_8k(parts, want, order, fd, what):
    """parts: the results of consecutive pushes of the whole batch; every word of every stream against its solo expectation"""
    got = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
    bad, words = 0, 0
    for b, name in enumerate(order):
        wo, wp, wf, wc = want[name]
        label = f"{what}, stream {b} ({name or 'clean copy'})"
        assert np.array_equal(got["produced"][b], wp), f"{label}: produced"
        rows = got["out"][b][wp != 0].reshape(-1)
        assert _is_sent(got["out"][b][wp == 0]), f"{label}: output rows of frames that produced nothing were written"
        d = N.differing_words(rows, wo)
        bad, words = bad + d, words + wo.size
        assert d == 0, f"{label}: {d} of {wo.size} output words differ from the restatement"
        if fd:
            assert np.array_equal(got["flags"][b].astype(np.int32), wf), f"{label}: flags at {np.flatnonzero(got['flags'][b] != wf)[:6]}"
            assert np.array_equal(got["counter"][b], wc), f"{label}: frame counter"
    print(f"\n{what}: {words} output words of {len(order)} streams, {bad} differ")


@pytest.mark.parametrize("fd", [False, True], ids=["sea_ns_streams_push", "sea_ns_streams_push_fd"])
def test_streams_8k_vs_restatement(oracle, fd):
    """cases a, b, c, d in one batch and one push: every output word (flags and frame counter too) of every stream equals its
    solo restatement result -- the clean copies between the poisoned streams included"""
    base, s, order, x = _batch_8k()
    want = _want_8k(oracle)
    r, _ = _push_8k(x, fd)
    _check_8k([r], want, order, fd, "one push")


@pytest.mark.parametrize("fd", [False, True], ids=["sea_ns_streams_push", "sea_ns_streams_push_fd"])
def test_streams_8k_carried_state_and_reset(oracle, fd):
    """case e: the batch in two pushes, cut right after frame 2 (the overflowing sample at [2][40]) and right after frame 3
    (NaN at [3][5]), the state blob passed back in: the one-push result.  case f: after the poisoned batch, the base stream
    pushed on the same state with reset: a fresh push."""
    base, s, order, x = _batch_8k()
    want = _want_8k(oracle)
    state = None
    for cut in N.CARRY_CUTS:
        r1, state = _push_8k(x[:, :cut], fd)
        r2, state = _push_8k(x[:, cut:], fd, state=state, reset=False)
        _check_8k([r1, r2], want, order, fd, f"two pushes cut at {cut}")
    clean = np.stack([base] * len(order))
    r, _ = _push_8k(clean, fd, state=state, reset=True)
    _check_8k([r], want, [None] * len(order), fd, "reset on a poisoned state")


# ------------------------------------------------------------------------------------------------ 16 kHz streams
_WANT_16K = {}


def _batch_16k(oracle):
    if not _WANT_16K:
        base, s = N.streams_16k()
        g = N.ns16k_streams_per_group()
        order = N.batch_order(sorted(s), 0, group=g)
        for k in range(0, len(order), g):   # every poisoned stream shares its workgroup with clean ones only
            assert order[k] is not None and all(o is None for o in order[k + 1:k + g])
        want = {None: oracle.ns16k_new().push(base.reshape(-1))}
        for n in s:
            want[n] = oracle.ns16k_new().push(s[n].reshape(-1))
        for n in (k for k in s if k.startswith("a/")):
            ctl = oracle.ns16k_new().push(N.a_control(s[n], n).reshape(-1))
            assert not N.same_words(want[n]["out"], ctl["out"]), f"{n}: same output as with 1e18"
        _WANT_16K.update(order=order, want=want, x=np.stack([base if n is None else s[n] for n in order]))
    return _WANT_16K["order"], _WANT_16K["want"], _WANT_16K["x"]


def _push_16k(x, state=None, reset=True):
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    B, n, _ = x.shape
    fr = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    bufs = dict(out=_full((B + GUARD, n, 160), torch.float32), produced=_full((B + GUARD, n), torch.int32),
                flags=_full((B + GUARD, n), torch.uint8), counter=_full((B + GUARD, n), torch.int32),
                wiener=_full((B + GUARD, n, 25), torch.float32))
    if state is None:
        state = torch.zeros((B, lib.sea_ns16k_state_floats()), dtype=torch.float32, device=DEV)
    rc = lib.sea_ns16k_streams_push(_p(fr), _p(bufs["out"]), _p(bufs["produced"]), _p(bufs["flags"]), _p(bufs["counter"]),
                                    _p(bufs["wiener"]), _p(state), B, n, int(reset), None)
    assert rc == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in r.items():
        assert _is_sent(v[B:]), f"{k}: guard rows behind the last stream were written"
        r[k] = v[:B]
    return r, state


def _check_16k(parts, want, order, what):
    got = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
    nfr = got["produced"].shape[1]
    bad, words = 0, 0
    for b, name in enumerate(order):
        w = want[name]
        label = f"{what}, stream {b} ({name or 'clean copy'})"
        wout = w["out"].reshape(nfr, 160)
        touched = w["counter"] != -7
        produced = (wout.view(np.uint32) != np.float32(-7.0).view(np.uint32)).any(axis=1)
        assert np.array_equal(got["produced"][b].astype(bool), produced), f"{label}: produced"
        assert np.array_equal(got["counter"][b][touched], w["counter"][touched]), f"{label}: frame counter"
        assert np.all(got["counter"][b][~touched] == 0), f"{label}: counter where the first stage did not run"
        for bit, k in enumerate(("var", "spec", "mel", "vadns")):
            assert np.array_equal((got["flags"][b][touched] >> bit) & 1, w[k][touched]), f"{label}: {k}"
        assert _is_sent(got["out"][b][~produced]) and _is_sent(got["wiener"][b][~produced]), f"{label}: rows of frames without output"
        d = N.differing_words(got["out"][b][produced], wout[produced]) + N.differing_words(got["wiener"][b][produced], w["wiener"])
        bad, words = bad + d, words + int(produced.sum()) * 185
        assert d == 0, f"{label}: {d} output / gain words differ from the restatement"
    print(f"\n{what}: {words} output and gain words of {len(order)} streams, {bad} differ")


def test_streams_16k_vs_restatement(oracle):
    """sea_ns16k_streams_push on cases a and c, every poisoned stream sharing its workgroup with clean copies (case d), in
    one push and (case e) in two pushes cut after frame 2 and after frame 3: out, produced, flags, counter, wiener"""
    order, want, x = _batch_16k(oracle)
    r, _ = _push_16k(x)
    _check_16k([r], want, order, "16 kHz, one push")
    for cut in N.CARRY_CUTS:
        r1, state = _push_16k(x[:, :cut])
        r2, _ = _push_16k(x[:, cut:], state=state, reset=False)
        _check_16k([r1, r2], want, order, f"16 kHz, two pushes cut at {cut}")


# ------------------------------------------------------------------------------------------------ CompCeps, rfft
def test_compceps_frames_vs_restatement(oracle):
    """sea_compceps_frames on 35 frames (three tiles, each with poisoned and clean frames), and the host form
    sea_compceps_frame on three of them"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    cc = N.compceps_frames()
    want = np.stack([oracle.compceps_frame(v) for v in cc])
    assert np.isnan(want).any() and np.isinf(want).any()                                   # the expectations hold NaN and Inf
    assert all(not np.isfinite(want[i]).all() for i in N.CC_TABLE_ROWS)
    assert all(np.isfinite(want[i]).all() for i in range(len(cc)) if i not in N.CC_POISONED)
    n = len(cc)
    x = torch.from_numpy(cc).to(DEV)
    out = _full((n + GUARD, 14), torch.float32)
    assert lib.sea_compceps_frames(_p(x), _p(out), n, None) == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _is_sent(got[n:]), "guard rows behind the last frame were written"
    per = [N.differing_words(got[i], want[i]) for i in range(n)]
    print(f"\nsea_compceps_frames: {sum(per)} of {n * 14} words differ; per poisoned frame "
          f"{ {N.CC_POISONED[i]: per[i] for i in sorted(N.CC_POISONED)} }")
    assert sum(per) == 0, f"frames {[i for i in range(n) if per[i]]} differ: got {got[[i for i in range(n) if per[i]][0]]}"
    # clean frames alone give the same rows: nothing leaks from a poisoned neighbour in the tile
    clean = [i for i in range(n) if i not in N.CC_POISONED]
    solo = sea.compceps_frames(torch.from_numpy(cc[clean]).to(DEV)).cpu().numpy()
    assert np.array_equal(solo.view(np.uint32), got[clean].view(np.uint32))
    for i in (3, 5, 20):   # +Inf, NaN, a clean one
        assert N.same_words(sea.DoCompCeps(cc[i]), want[i]), f"sea_compceps_frame on frame {i}"


def test_rfft_vs_restatement(oracle):
    """sea_rfft256_batch, sea_rfft_batch (512, 8) and the host symbol rfft on frames with NaN, +-Inf and +-FLT_MAX"""
    import speech_enhancement_amd as sea
    torch = _torch()
    lib = sea.load()
    a, b = N.rfft_frames()
    wa, wb = np.stack([oracle.rfft(v) for v in a]), np.stack([oracle.rfft(v, 8) for v in b])
    assert np.isnan(wa).any() and np.isnan(wb).any()
    clean = [i for i in range(len(a)) if i not in N.RFFT256_POISONED]
    assert np.isfinite(wa[clean]).all()
    out = _full((len(a) + GUARD, 256), torch.float32)
    assert lib.sea_rfft256_batch(_p(torch.from_numpy(a).to(DEV)), _p(out), len(a), None) == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _is_sent(got[len(a):]), "guard rows behind the last frame were written"
    d = N.differing_words(got[:len(a)], wa)
    print(f"\nsea_rfft256_batch: {d} of {wa.size} words differ")
    assert d == 0
    buf = _full((len(b) + GUARD, 512), torch.float32)
    buf[:len(b)] = torch.from_numpy(b).to(DEV)
    assert lib.sea_rfft_batch(_p(buf), 512, 8, len(b), None) == 0, lib.sea_last_error()
    torch.cuda.synchronize()
    gb = buf.cpu().numpy()
    assert _is_sent(gb[len(b):]), "guard rows behind the last frame were written"
    assert N.same_words(gb[:len(b)], wb), f"sea_rfft_batch (512, 8): {N.differing_words(gb[:len(b)], wb)} words differ"
    assert N.same_words(sea.rfft(a[1]), wa[1]), "rfft on the frame with NaN at index 0"
