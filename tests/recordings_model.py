"""Test infrastructure: the numpy model of the long-recording denoiser's contract (the reference's
aurora_speech_enhancement.cpp: WaveConvert :82-230, BufferDenoise :25-80).

  level           float64, the sum of squares an exact integer converted once, the cast an x86-64 build's
  buffer_denoise  composed from the oracle's etsi_denoise per chunk, the work buffer zeroed per chunk
  fir             float32, k ascending, multiply and add separate (ours: the tool's IPP call and its taps are not in the reference)
"""
import numpy as np

OVERLAP = 320


def x86_short(p):
    """(short) of a float32 / float64 array as cvttss2si / cvttsd2si + low half give it: NaN and |p| >= 2^31 give 0"""
    p = np.asarray(p)
    with np.errstate(invalid="ignore"):
        ok = np.abs(p) < 2147483648.0
    v = np.trunc(np.where(ok, p, 0)).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16)


def level_factor(x, level):
    x = np.asarray(x, dtype=np.int16)
    e = float(int((x.astype(np.int64) ** 2).sum()))  # exact integer, one correctly rounded conversion
    with np.errstate(divide="ignore"):
        e = np.sqrt(np.float64(e) / np.float64(x.size))
        return np.float64(np.float32(level)) / e


def level_apply(x, factor):
    x = np.asarray(x, dtype=np.int16)
    with np.errstate(invalid="ignore", over="ignore"):
        return x86_short(x.astype(np.float32).astype(np.float64) * np.float64(factor))


def chunks(S, B):
    """(first sample, length) of every chunk of a recording of S >= 320 samples"""
    T, R = divmod(S, B)
    if T == 0:
        return [(0, S)]
    return [(0, B)] + [(i * B - OVERLAP, B + OVERLAP) for i in range(1, T)] + [(T * B - OVERLAP, R + OVERLAP)]


def buffer_denoise(x, B, denoise):
    """denoise (chunk) -> int16 array of the chunk's length with 0 where etsi_denoise writes nothing"""
    x = np.asarray(x, dtype=np.int16)
    S = x.size
    des = np.zeros(S, np.int16)
    T, R = divmod(S, B)
    if T == 0:
        work = denoise(x)
        des[:S - OVERLAP] = work[OVERLAP:S]
        return des
    work = denoise(x[:B])
    des[:B - OVERLAP] = work[OVERLAP:B]
    for i in range(1, T):
        work = denoise(x[i * B - OVERLAP:i * B + B])
        des[i * B - OVERLAP:i * B + B - OVERLAP] = work[OVERLAP:B + OVERLAP]
    work = denoise(x[T * B - OVERLAP:T * B + R])
    des[T * B - OVERLAP:S - OVERLAP] = work[OVERLAP:OVERLAP + R]
    des[S - OVERLAP:] = 0
    return des


def fir(des, taps):
    des = np.asarray(des, dtype=np.int16).astype(np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    acc = np.zeros(des.size, np.float32)
    for k in range(min(taps.size, des.size)):
        acc[k:] = acc[k:] + taps[k] * des[:des.size - k]
    return x86_short(acc)


def denoise_recording(x, B, level, taps, denoise):
    """one recording -> (audio, factor, status)"""
    x = np.asarray(x, dtype=np.int16)
    if x.size < OVERLAP:
        return np.zeros(x.size, np.int16), 0.0, 1
    factor = 1.0
    if level > 0:
        factor = level_factor(x, level)
        x = level_apply(x, factor)
    des = buffer_denoise(x, B, denoise)
    if taps is not None and len(taps):
        des = fir(des, taps)
    return des, float(factor), 0


def oracle_denoise(ora):
    return lambda chunk: ora.etsi_denoise(np.ascontiguousarray(chunk), fill=0)
