"""Long recordings: the chunking of the reference's batch tool (BufferDenoise, aurora_speech_enhancement.cpp:25-80) over
libsea_mi355x.so.  The plan (sea_recording_plan, sea_recording_stitch_map; csrc/recording_plan.h) is host arithmetic;
buffer_denoise runs the chunks of all recordings as the utterances of ONE sea_denoise_utterances call -- they are independent
NoiseSup chains, each from a fresh state -- and stitches their outputs on the host.  The contract is DESIGN.md section 5.20:
the result differs from etsi_denoise on the whole recording, as the reference's does.  The tool's level and band-pass steps
are not here yet (Status)."""
import ctypes

import numpy as np

from . import _lib

CHUNK = 1_440_000  # the tool's batch_length: 3 minutes at 8 kHz
OVERLAP = 320      # etsi_offset_points


def recording_plan(samples, chunk=CHUNK):
    """dict(src, len, off: int64 [n_chunks], layout: samples of the chunk layout); n_chunks = 0 below 320 samples"""
    lib = _lib.load()
    n = lib.sea_recording_plan(int(samples), int(chunk), None, None, None, 0)
    if n < 0:
        _lib.check(1, "sea_recording_plan")
    src, ln, off = (np.zeros(n, np.int64) for _ in range(3))
    if n:
        lib.sea_recording_plan(int(samples), int(chunk), src.ctypes.data, ln.ctypes.data, off.ctypes.data, n)
    return dict(src=src, len=ln, off=off, layout=int(lib.sea_recording_layout_samples(int(samples), int(chunk))))


def recording_stitch_map(samples, chunk=CHUNK, first=0, count=None):
    """int64 [count]: where des[first + k] lies in the chunks' outputs laid out by recording_plan, -1 where it is 0"""
    count = int(samples) - int(first) if count is None else int(count)
    index = np.zeros(max(count, 0), np.int64)
    rc = _lib.load().sea_recording_stitch_map(int(samples), int(chunk), int(first), count, index.ctypes.data)
    _lib.check(rc, "sea_recording_stitch_map")
    return index


def buffer_denoise_recordings(xs, chunk=CHUNK):
    """BufferDenoise of every int16 recording of xs, all chunks in one sea_denoise_utterances call.  Returns dict(audio = list
    of int16 arrays of the recordings' lengths, status = int32 [n]: 1 for a recording shorter than 320 samples, which the tool
    skips -- its audio is zero).  The trailing len % 80 samples of a chunk, which etsi_denoise never writes, count as 0."""
    lib = _lib.load()
    xs = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in xs]
    plans = [recording_plan(x.size, chunk) for x in xs]
    works = [np.zeros(p["layout"], np.int16) for p in plans]
    ins, outs, lens = [], [], []
    for x, p, w in zip(xs, plans, works):
        for s, n, o in zip(p["src"], p["len"], p["off"]):
            ins.append(x.ctypes.data + 2 * int(s))   # the chunks alias overlapping ranges of the recording
            outs.append(w.ctypes.data + 2 * int(o))
            lens.append(int(n))
    if lens:
        m = len(lens)
        rc = lib.sea_denoise_utterances((ctypes.c_void_p * m)(*ins), (ctypes.c_void_p * m)(*outs), (ctypes.c_long * m)(*lens), m)
        _lib.check(rc, "sea_denoise_utterances")
    audio = []
    for x, p, w in zip(xs, plans, works):
        if not len(p["src"]):
            audio.append(np.zeros(x.size, np.int16))
            continue
        idx = recording_stitch_map(x.size, chunk)
        audio.append(np.where(idx >= 0, w[np.maximum(idx, 0)], 0).astype(np.int16))
    return dict(audio=audio, status=np.array([0 if len(p["src"]) else 1 for p in plans], np.int32))


def buffer_denoise(x, chunk=CHUNK):
    """BufferDenoise of one recording (see buffer_denoise_recordings)"""
    return buffer_denoise_recordings([x], chunk)["audio"][0]
