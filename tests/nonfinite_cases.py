"""Test infrastructure: seeded inputs of the float-taking entry points that hold Inf, NaN or finite floats whose energy
overflows, and the rule under which results on them are compared.

The reference takes its logarithms from libm, where log (Inf) = Inf and log (NaN) = NaN; those values then steer branches
(the VAD's mean energy, the noise update it gates, the cepstral floors).  A FINITE float is enough to get there: 1.9e19 is the
smallest sample used here whose square is above FLT_MAX, so `64 + sum x^2` (NoiseSup.c:386-391) is +Inf.  Used by
tests/test_nonfinite_cpu.py (restatement against reference, and against a mutant whose logarithm reads bit patterns) and
tests/test_gpu_nonfinite.py (the kernels against the restatement).

The comparison rule, `same_words`: a word that is finite in `want` must be bit-equal (-0.0 included), an infinity must be
bit-equal (so its sign counts), a NaN must sit where a NaN sits -- payload and sign are free, because an x86 generates the
negative quiet NaN 0xFFC00000 and gfx950 the positive 0x7FC00000 for the same invalid operation.  Integers must be equal.
No tolerance, no share of words left out.  (tests/test_gpu_hw25.py compares "NaNs by position" in the same way.)"""
import hashlib
import os
import re

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
OVERFLOWING = (1.9e19, 3e19, 3e38)          # finite floats whose square is +Inf in float32
A_FRAMES = (2, 6, 12, 30)                   # the frame of the a-cases' offending sample [f][HOP / 2]
NFR_8K, NFR_16K = 120, 48
STREAM_SEED = 12
CONTROL = np.float32(1e18)                  # the largest scale the amplitude test reaches: its square is finite


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differing_words(got, want):
    """how many words of `got` break the rule of the module docstring against `want` (float32 arrays of one shape, or integer
    arrays, which must be equal)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"shape {got.shape} vs {want.shape}"
    if want.dtype.kind in "iub":
        return int(np.count_nonzero(got.astype(np.int64) != want.astype(np.int64)))
    assert got.dtype == np.float32 and want.dtype == np.float32, f"{got.dtype} vs {want.dtype}"
    wn = np.isnan(want)
    bad = np.where(wn, ~np.isnan(got), _u32(got) != _u32(want))
    return int(np.count_nonzero(bad))


def same_words(got, want):
    return differing_words(got, want) == 0


def canonical(a):
    """the array with every NaN replaced by the positive quiet NaN 0x7FC00000 (what digests are taken of)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = 0x7FC00000
    return w.view(np.float32)


def digest(a):
    """dtype, shape and sha256 of the bytes of an array after canonical()"""
    a = canonical(a)
    return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


# ---------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------
def float_stream_case(seed, nfr=60, hop=80):
    """hop 80: _float_stream_case of tests/test_gpu_parity.py, value for value (tests/test_nonfinite_cpu.py checks that);
    hop 160: the same signal laid out in frames of 160 with the tone at the same digital frequency per frame"""
    rng = np.random.default_rng(seed)
    t = np.arange(nfr * hop)
    x = rng.standard_normal(nfr * hop) * 800 + 2000 * np.sin(t * (8.0 / hop)) * ((t // (20 * hop)) % 2)
    return x.astype(np.float32).reshape(nfr, hop)


def _streams(hop, nfr, with_b):
    base = float_stream_case(STREAM_SEED, nfr, hop)
    mid, five = hop // 2, 5
    s = {}
    for f in A_FRAMES:                                       # a: one finite sample whose square overflows
        for v in OVERFLOWING:
            x = base.copy()
            x[f, mid] = np.float32(v)
            s[f"a/{f}/{v:g}"] = x
    if with_b:                                               # b: bursts and whole streams whose energy overflows
        for lo, hi in ((3, 6), (30, 33)):
            x = base.copy()
            x[lo:hi] *= np.float32(1e20)
            s[f"b/burst{lo}-{hi - 1}"] = x
        for sc in (1e25, 3e30):
            s[f"b/x{sc:g}"] = base * np.float32(sc)
    for name, v in (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan)):   # c: the non-finite values themselves
        for f, i in ((3, five), (30, five), (0, 0)):
            x = base.copy()
            x[f, i] = np.float32(v)
            s[f"c/{name}/{f}.{i}"] = x
    x = base.copy()
    x[8] = np.float32(np.nan)
    s["c/nanframe"] = x
    x = base.copy()
    x[8] = FLT_MAX * np.where(np.arange(hop) % 2 == 0, 1, -1).astype(np.float32)
    s["c/fltmaxframe"] = x
    with np.errstate(over="ignore"):
        assert all(np.isinf(np.float32(v) * np.float32(v)) for v in OVERFLOWING) and np.isfinite(CONTROL * CONTROL)
    return base, s


def streams_8k():
    """(base [120][80], {name: poisoned stream}) -- cases a, b, c of the 8 kHz entry points"""
    return _streams(80, NFR_8K, True)


def streams_16k():
    """(base [48][160], {name: poisoned stream}) -- cases a and c for the 16 k-native variant (oracle/ns16k_oracle.c, whose
    frame loop is PARITY UNPINNED: no reference build of it exists, so these show HIP == restatement only)"""
    return _streams(160, NFR_16K, False)


def a_control(x, name):
    """the a-case stream `name` with its offending sample replaced by 1e18 (finite square)"""
    f = int(name.split("/")[1])
    y = x.copy()
    y[f, x.shape[1] // 2] = CONTROL
    return y


def batch_order(names, n_clean, group=1):
    """The order of a batch: `names` (poisoned streams) with `n_clean` copies of the base, marked None, spread evenly between
    them (case d).  group > 1: the entry point packs `group` consecutive streams into one workgroup; then every poisoned
    stream gets clean workgroup mates instead -- (poisoned, None, ..) per workgroup -- and n_clean is ignored."""
    names = list(names)
    if group > 1:
        out = []
        for n in names:
            out += [n] + [None] * (group - 1)
        return out
    out, step = [], max(len(names) // (n_clean + 1), 1)
    for i, n in enumerate(names):
        if i and i % step == 0 and out.count(None) < n_clean:
            out.append(None)
        out.append(n)
    while out.count(None) < n_clean:
        out.insert(len(out) - 1, None)
    return out


CARRY_CUTS = (3, 4)   # case e: two pushes cut right after frame 2 (the a-cases at [2][..]) and after frame 3 (NaN at [3][5])


def ns16k_streams_per_group():
    """G of sea_ns16k_streams_push's launch (capi.hip: `constexpr int G = sea::kNs16PipeStreamsPerGroup`), read from the
    sources the way tests/launch_caps.py reads its constants"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech_enhancement_amd", "csrc")
    with open(os.path.join(csrc, "capi.hip")) as f:
        capi = f.read()
    use = re.findall(r"constexpr int G = sea::(\w+);\s*\n\s*hipLaunchKernelGGL\(sea::ns16k_pipe_kernel, dim3\(\(n_streams \+ G - 1\) / G\)", capi)
    if len(use) != 1:
        raise LookupError("the launch of ns16k_pipe_kernel in capi.hip is not where it was")
    with open(os.path.join(csrc, "sea_kernels.h")) as f:
        val = re.findall(r"constexpr int %s = (\d+);" % use[0], f.read())
    if len(val) != 1:
        raise LookupError(f"{use[0]} is not defined once in sea_kernels.h")
    return int(val[0])


# ---------------------------------------------------------------------------------------------------------------
# CompCeps frames [35][201] (word 0 = Data[-1]) and rfft frames
# ---------------------------------------------------------------------------------------------------------------
CC_POISONED = {1: "3e19", 3: "+inf", 5: "nan", 17: "x1e17", 19: "nan_at_data[-1]", 21: "zero", 32: "-inf", 34: "fltmax"}
CC_TABLE_ROWS = (1, 3, 5, 17)   # one 3e19 sample, one +Inf, one NaN, frame x 1e17: the reference gives NaN / Inf there


def compceps_frames():
    """35 frames of sigma 900, three tiles of 16 each holding poisoned and clean frames; CC_POISONED says which are which"""
    rng = np.random.default_rng(4242)
    d = (rng.standard_normal((35, 201)) * 900).astype(np.float32)
    d[1, 101] = np.float32(3e19)
    d[3, 101] = np.float32(np.inf)
    d[5, 101] = np.float32(np.nan)
    d[17] *= np.float32(1e17)
    d[19, 0] = np.float32(np.nan)
    d[21] = 0.0
    d[32, 57] = np.float32(-np.inf)
    d[34] = FLT_MAX * np.where(np.arange(201) % 2 == 0, 1, -1).astype(np.float32)
    return d


RFFT256_POISONED = {1: "nan@0", 3: "nan@1", 5: "nan@128", 7: "nan@255", 9: "+inf,-inf", 11: "fltmax"}


def rfft_frames():
    """(frames [13][256] for (256, 8), frames [2][512] for (512, 8)): NaN at index 0, 1, 128, 255, +Inf with -Inf, +-FLT_MAX
    everywhere (the butterflies overflow, then Inf - Inf), clean frames between"""
    rng = np.random.default_rng(777)
    a = (rng.standard_normal((13, 256)) * 3000).astype(np.float32)
    for row, i in ((1, 0), (3, 1), (5, 128), (7, 255)):
        a[row, i] = np.float32(np.nan)
    a[9, 17], a[9, 200] = np.float32(np.inf), np.float32(-np.inf)
    a[11] = FLT_MAX * np.where(np.arange(256) % 2 == 0, 1, -1).astype(np.float32)
    b = (rng.standard_normal((2, 512)) * 3000).astype(np.float32)
    b[0] = FLT_MAX * np.where(np.arange(512) % 3 == 0, 1, -1).astype(np.float32)
    b[1, 300] = np.float32(np.nan)
    return a, b


# ---------------------------------------------------------------------------------------------------------------
# digests of what a library (the reference build, or the restatement: same entry points) makes of the 8 kHz inputs
# ---------------------------------------------------------------------------------------------------------------
def live_nonfinite_digests(lib):
    base, s = streams_8k()
    d = {}
    for name, x in [("base", base)] + sorted(s.items()):
        out, prod = lib.ns_stream_f32(x)
        d[f"nonfinite/stream/{name}/in"], d[f"nonfinite/stream/{name}/out"] = digest(x), digest(out)
        d[f"nonfinite/stream/{name}/produced"] = digest(prod)
    cc = compceps_frames()
    d["nonfinite/cc/in"] = digest(cc)
    d["nonfinite/cc/out"] = digest(np.stack([lib.compceps_frame(v) for v in cc]))
    a, b = rfft_frames()
    d["nonfinite/rfft256/in"], d["nonfinite/rfft256/out"] = digest(a), digest(np.stack([lib.rfft(v) for v in a]))
    d["nonfinite/rfft512_8/in"], d["nonfinite/rfft512_8/out"] = digest(b), digest(np.stack([lib.rfft(v, 8) for v in b]))
    return d
