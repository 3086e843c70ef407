"""Test infrastructure: the model of the objective scores.

Two statements of the contract that must agree bit for bit (tests/test_scores_cpu.py): the plain-C program
tests/score_model_driver.c, which states the loops literally, and `scores` / `mask_counts` below, numpy on int64 prefix sums
with sea_lnf taken from the C header through tests/dnn_model.lnf.  The GPU results must equal them bit for bit.

Also here: the inputs of the GPU tests, so that the CPU suite can assert their conditions (at most 10 % of the frames of a
random case clamped or skipped; each of the four mask counts at least 10 % of the units) without a device.
"""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import dnn_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_enhancement_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "score_model_driver.c")
C_DB = np.float32(float.fromhex("0x1.15f2cep+2"))  # the float nearest 10 / ln 10
SKIPPED = np.uint32(0x7FC00000)
WAVE_FRAMES, TILE_FRAMES = 63, 252  # frames per wave tile and per workgroup of score_frames_kernel
MASK_TILE_ROWS = 64

_built = {}


def build_driver(sanitize=False):
    """the driver's path; built once per process (sanitize: with -fsanitize=address,undefined at -O1)"""
    if sanitize not in _built:
        cc = shutil.which("gcc")
        assert cc, "gcc is needed to build tests/score_model_driver.c"
        d = tempfile.mkdtemp(prefix="score_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "score_model_driver")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", CSRC, SOURCE, "-o", exe, "-lm"])
        _built[sanitize] = (exe, d)
    return _built[sanitize]


def _run(args, sanitize=False, timeout=600):
    exe, _ = build_driver(sanitize)
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0 and not run.stderr, f"score_model_driver exited with {run.returncode}:\n{run.stderr[-2000:]}"
    return run.stdout


def lnf_sweep():
    """every float of (2^39, 2^41] -> dict n, max_ulp, at"""
    n, ulp, at = (tok.split("=")[1] for tok in _run(["lnf_sweep"]).split())
    return dict(n=int(n), max_ulp=float(ulp), at=at)


def frames_of(length, hop):
    return (length - 2 * hop) // hop + 1 if length >= 2 * hop else 0


def _i16(xs):
    return [np.ascontiguousarray(x, np.int16).reshape(-1) for x in xs]


def driver_scores(refs, ests, hop, sanitize=False):
    """the C model -> list of dicts: sums (int64 [3]), seg_sum (float64), seg_frames (int), frame_db (float32 [F])"""
    refs, ests = _i16(refs), _i16(ests)
    _, d = build_driver(sanitize)
    src, dst = os.path.join(d, "score_in.bin"), os.path.join(d, "score_out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([hop, len(refs)], np.int32).tobytes())
        f.write(np.asarray([r.size for r in refs], np.int64).tobytes())
        for r, e in zip(refs, ests):
            assert r.size == e.size
            f.write(r.tobytes() + e.tobytes())
    _run(["score", src, dst], sanitize)
    raw = open(dst, "rb").read()
    out, at = [], 0
    for r in refs:
        F = frames_of(r.size, hop)
        sums = np.frombuffer(raw, np.int64, 3, at)
        seg = np.frombuffer(raw, np.float64, 1, at + 24)[0]
        used = int(np.frombuffer(raw, np.int64, 1, at + 32)[0])
        db = np.frombuffer(raw, np.float32, F, at + 40).copy()
        out.append(dict(sums=sums.copy(), seg_sum=seg, seg_frames=used, frame_db=db))
        at += 40 + 4 * F
    assert at == len(raw)
    return out


def frame_energies(ref, est, hop):
    """int64 [F] each: srr, see, sre of every frame, and n = srr - 2 sre + see, from prefix sums"""
    r, e = np.asarray(ref).astype(np.int64), np.asarray(est).astype(np.int64)
    F = frames_of(r.size, hop)
    starts = hop * np.arange(F)
    out = []
    for prod in (r * r, e * e, r * e):
        c = np.concatenate([np.zeros(1, np.int64), np.cumsum(prod)])
        out.append(c[starts + 2 * hop] - c[starts])
    srr, see, sre = out
    return srr, see, sre, srr - 2 * sre + see


def scores(refs, ests, hop):
    """the numpy model, in the driver's output form"""
    out = []
    for ref, est in zip(_i16(refs), _i16(ests)):
        r, e = ref.astype(np.int64), est.astype(np.int64)
        sums = np.array([(r * r).sum(), (e * e).sum(), (r * e).sum()], np.int64)
        srr, see, sre, n = frame_energies(ref, est, hop)
        F = srr.size
        used = srr != 0
        db = np.zeros(F, np.float32)
        if F:
            # numpy converts int64 to float32 by round-to-nearest-even, as C does; float32 arrays subtract and multiply in float32
            a = DM.lnf((np.where(used, srr, 0) + 1).astype(np.float32))
            b = DM.lnf((np.where(used, n, 0) + 1).astype(np.float32))
            db = np.clip(((a - b).astype(np.float32) * C_DB).astype(np.float32), np.float32(-10), np.float32(35)).astype(np.float32)
            db.view(np.uint32)[~used] = SKIPPED
        seg = 0.0
        for l in range(64):  # np.cumsum adds in order (np.sum does not)
            lane = db[l::64][used[l::64]].astype(np.float64)
            seg += float(np.cumsum(lane)[-1]) if lane.size else 0.0
        out.append(dict(sums=sums, seg_sum=np.float64(seg), seg_frames=int(used.sum()), frame_db=db))
    return out


def same_scores(a, b):
    """bit for bit: the integers, the double's bits, the floats' bits"""
    return (np.array_equal(a["sums"], b["sums"]) and np.float64(a["seg_sum"]).tobytes() == np.float64(b["seg_sum"]).tobytes()
            and a["seg_frames"] == b["seg_frames"] and a["frame_db"].dtype == b["frame_db"].dtype == np.float32
            and a["frame_db"].tobytes() == b["frame_db"].tobytes())


def _masks(ms):
    return [np.ascontiguousarray(m, np.float32).reshape(-1, 64) for m in ms]


def driver_mask_counts(est, ideal, t_est, t_ideal, sanitize=False):
    est, ideal = _masks(est), _masks(ideal)
    _, d = build_driver(sanitize)
    src, dst = os.path.join(d, "mask_in.bin"), os.path.join(d, "mask_out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([len(est), 0], np.int32).tobytes() + np.asarray([t_est, t_ideal], np.float32).tobytes())
        f.write(np.asarray([m.shape[0] for m in est], np.int32).tobytes())
        for a, b in zip(est, ideal):
            assert a.shape == b.shape
            f.write(a.tobytes() + b.tobytes())
    _run(["mask", src, dst], sanitize)
    return np.fromfile(dst, np.int64).reshape(len(est), 4)


def mask_counts(est, ideal, t_est, t_ideal):
    """the numpy model: int64 [n][4], n11, n10, n01, n00 (a comparison with a NaN is false: off)"""
    out = np.zeros((len(est), 4), np.int64)
    with np.errstate(invalid="ignore"):
        for u, (a, b) in enumerate(zip(_masks(est), _masks(ideal))):
            on_e, on_i = a > np.float32(t_est), b > np.float32(t_ideal)
            out[u] = [(on_e & on_i).sum(), (on_e & ~on_i).sum(), (~on_e & on_i).sum(), (~on_e & ~on_i).sum()]
    return out


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------
def random_pair(seed, length, hop):
    """speech-like clean audio and an estimate whose error level drifts, so that the frames' d spread over about -6 .. 32 dB:
    the logarithm path, not the clamp, decides nearly every frame"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(-9000, 9001, length).astype(np.int16)
    knots = np.arange(0, length + 4 * hop, 4 * hop)
    snr = np.interp(np.arange(length), knots, rng.uniform(-6.0, 32.0, knots.size))
    err = rng.integers(-9000, 9001, length) * 10.0 ** (-snr / 20.0)
    est = np.clip(np.rint(ref + err), -32768, 32767).astype(np.int16)
    return ref, est


def edge_lengths(hop):
    """the lengths the issue lists: around one frame, and F at the edges of a 63-frame wave tile (62, 63, 64, 126, 127) and of a
    252-frame workgroup (252, 253, 505) with r = 0, 1, hop - 1 samples of tail"""
    ls = [0, 1, hop - 1, 2 * hop - 1, 2 * hop, 2 * hop + 1, 3 * hop]
    ls += [hop * (F + 1) + r for F in (62, 63, 64, 126, 127, 252, 253, 505) for r in (0, 1, hop - 1)]
    return ls


def length_cases(hop):
    ls = edge_lengths(hop)
    pairs = [random_pair(1000 + hop + i, L, hop) for i, L in enumerate(ls)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def placement_lists(hop):
    """lists of 1, 2 and 67 utterances of mixed lengths, one of them empty in the middle"""
    rng = np.random.default_rng(77 + hop)
    out = []
    for n in (1, 2, 67):
        ls = [int(v) for v in rng.integers(1, 9 * hop * 63, n)]
        if n > 2:
            ls[n // 2] = 0
            ls[5] = hop * 253 + 3  # one that needs two workgroups
        pairs = [random_pair(2000 + hop + 100 * n + i, L, hop) for i, L in enumerate(ls)]
        out.append(([p[0] for p in pairs], [p[1] for p in pairs]))
    return out


def special_cases(hop):
    """name -> (ref, est), 70 frames each (two wave tiles)"""
    L = hop * 71 + 5
    rng = np.random.default_rng(5 + hop)
    loud = rng.integers(-9000, 9001, L).astype(np.int16)
    noise = rng.integers(-9000, 9001, L).astype(np.int16)
    gaps = loud.copy()
    for f0 in (0, 9, 10, 30, 62, 63, 69):  # silent frames (2 hop samples from hop f0) between loud ones
        gaps[hop * f0:hop * f0 + 2 * hop] = 0
    return {
        "silent reference": (np.zeros(L, np.int16), noise),
        "silent frames between loud ones": (gaps, np.clip(gaps.astype(np.int32) + noise // 16, -32768, 32767).astype(np.int16)),
        "all clamped low": ((loud // 64).astype(np.int16), noise),
        "all clamped high": (loud, np.clip(loud.astype(np.int32) + (np.arange(L) % 97 == 0), -32768, 32767).astype(np.int16)),
        "identical": (loud, loud.copy()),
        "extremes": (np.full(L, -32768, np.int16), np.full(L, 32767, np.int16)),
        "extremes, same sign": (np.full(L, -32768, np.int16), np.full(L, -32768, np.int16)),
    }


def chunk_list(hop=160):
    """eight utterances of 100 000 samples: 4 B per padded sample of staged audio and 4 B per frame and a few partials make about
    410 KB each, so a budget of 1 MB holds two and not three: four chunks"""
    pairs = [random_pair(3000 + i, 100000, hop) for i in range(8)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


MASK_ROWS = (0, 1, 63, 64, 65, 300)
MASK_THRESHOLDS = (0.0, 0.5, float(np.float32(2 ** -0.5)))


def mask_cases(t_est, t_ideal):
    """masks of MASK_ROWS rows: uniform values around the thresholds, and in every utterance with rows the special values --
    the threshold itself, +-0, +-Inf, NaN -- in both masks against each other"""
    rng = np.random.default_rng(11)
    special = np.float32([t_est, t_ideal, 0.0, -0.0, np.inf, -np.inf, np.nan, np.nextafter(np.float32(t_est), np.float32(2)),
                          np.nextafter(np.float32(t_ideal), np.float32(2))])
    est, ideal = [], []
    for rows in MASK_ROWS:
        a = (np.float32(t_est) + rng.uniform(-0.5, 0.5, (rows, 64))).astype(np.float32)
        b = (np.float32(t_ideal) + rng.uniform(-0.5, 0.5, (rows, 64))).astype(np.float32)
        if rows:
            k = min(len(special), 32)
            a[-1, :k], b[-1, 32:32 + k] = special[:k], special[:k]
            if rows > 1:  # every special value of one mask against every one of the other
                g = np.array(np.meshgrid(special, special)).reshape(2, -1)
                a[0, :], b[0, :] = g[0, :64], g[1, :64]
        est.append(a), ideal.append(b)
    return est, ideal
