"""Test infrastructure: STOI (Taal, Hendriks, Heusdens, Jensen 2011) in numpy float64, written from the paper's definition with
the conventions of DESIGN.md section 5.24 (frame count, zero rules, taps not renormalised).  It shares no code, table or loop
structure with tests/stoi_model_driver.c: the tables come from numpy's own hanning, kaiser and sinc, the resampler is a dense
upsample-and-convolve, the transform is numpy.fft.rfft.  It is the yardstick the float32 contract is measured against
(tests/test_stoi_cpu.py)."""
import numpy as np

FS, NFRAME, HOP, NFFT, NBAND, NSEG, BETA_DB, RANGE_DB = 10000, 256, 128, 512, 15, 30, -15.0, 40.0


def third_octave_matrix():
    """[15][257] of 0 / 1: the bins of each band, from the band centres 150 * 2^(j / 3) Hz"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    cf = 150.0 * 2.0 ** (np.arange(NBAND) / 3.0)
    A = np.zeros((NBAND, f.size))
    for j in range(NBAND):
        lo = int(np.argmin((f - cf[j] * 2.0 ** (-1 / 6)) ** 2))
        hi = int(np.argmin((f - cf[j] * 2.0 ** (1 / 6)) ** 2))
        A[j, lo:hi] = 1.0
    return A


def resample_to_10k(x, rate):
    p, q = {16000: (5, 8), 8000: (5, 4)}[rate]
    big = max(p, q)
    half = 10 * big
    t = np.arange(-half, half + 1)
    h = p * np.sinc(t / big) / big * np.kaiser(2 * half + 1, 5.0)
    x = np.asarray(x, np.float64)
    n_out = -(-p * x.size // q)
    if x.size == 0:
        return np.zeros(0)
    up = np.zeros(x.size * p)
    up[::p] = x
    return np.convolve(up, h)[half::q][:n_out]


def _frames(x, n):
    return np.stack([x[HOP * f:HOP * f + NFRAME] for f in range(n)]) if n else np.zeros((0, NFRAME))


def stoi(ref, est, rate):
    """dict: stoi, d [S][15], frames, kept, ratio (10^4 e / emax of every frame: how near the 40 dB decision was), clipped (the
    share of terms that took the clipped branch), den_min"""
    x, y = resample_to_10k(ref, rate), resample_to_10k(est, rate)
    w = np.hanning(NFRAME + 2)[1:-1]
    F = (x.size - NFRAME) // HOP + 1 if x.size >= NFRAME else 0
    fx, fy = _frames(x, F) * w, _frames(y, F) * w
    e = (fx ** 2).sum(axis=1)
    emax = e.max() if F else 0.0
    ratio = 10.0 ** (RANGE_DB / 10) * e / emax if emax > 0 else np.zeros(F)
    on = ratio > 1.0
    M = int(on.sum())
    out = dict(frames=F, kept=M, ratio=ratio, stoi=np.nan, d=np.zeros((0, NBAND)), clipped=0.0, den_min=np.inf)
    if M < NSEG:
        return out
    zx, zy = np.zeros(HOP * (M + 1)), np.zeros(HOP * (M + 1))
    for j, (a, b) in enumerate(zip(fx[on], fy[on])):
        zx[HOP * j:HOP * j + NFRAME] += a
        zy[HOP * j:HOP * j + NFRAME] += b
    A = third_octave_matrix()
    X = np.sqrt(np.abs(np.fft.rfft(_frames(zx, M) * w, NFFT)) ** 2 @ A.T)  # [M][15]
    Y = np.sqrt(np.abs(np.fft.rfft(_frames(zy, M) * w, NFFT)) ** 2 @ A.T)
    S = M - NSEG + 1
    d = np.zeros((S, NBAND))
    c = 1.0 + 10.0 ** (-BETA_DB / 20)
    clipped = 0
    den_min = np.inf
    for s in range(S):
        xs, ys = X[s:s + NSEG], Y[s:s + NSEG]
        ey = (ys ** 2).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.sqrt((xs ** 2).sum(axis=0) / ey)
            scaled = alpha * ys
        yc = np.minimum(np.where(ey > 0, scaled, 0.0), c * xs)
        clipped += int(np.count_nonzero((scaled >= c * xs) & (ey > 0)))
        xm, ym = xs - xs.mean(axis=0), yc - yc.mean(axis=0)
        den = np.sqrt((xm ** 2).sum(axis=0)) * np.sqrt((ym ** 2).sum(axis=0))
        den_min = min(den_min, float(np.where(ey > 0, den, np.inf).min()))
        with np.errstate(divide="ignore", invalid="ignore"):
            d[s] = np.where((ey > 0) & (den > 0), (xm * ym).sum(axis=0) / den, 0.0)
    out.update(stoi=float(d.mean()), d=d, clipped=clipped / (S * NBAND * NSEG), den_min=den_min)
    return out
