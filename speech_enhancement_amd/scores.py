"""Objective scores over libsea_mi355x.so (csrc/score_kernel.hip, csrc/score_capi.hip): whether an
enhancement made the audio better, and how close an estimated mask is to the ideal one.

  score_utterances       clean and enhanced int16 audio -> the exact energies Srr, See, Sre, and SNR, SI-SDR, segmental SNR
  mask_scores            estimated and ideal masks [F][64] -> the 2 x 2 counts, HIT, FA and HIT - FA, per utterance and pooled
  dnn_score_utterances   dnn_enhance_utterances followed by the scores of its output and of its input against the clean audio
  stoi_utterances        clean and enhanced int16 audio -> STOI, the short-time objective intelligibility measure (section 5.24)

The library returns exact integers (and the segmental sum as a double formed in a stated order); the derived figures are host
arithmetic here, in float64 from exact Python ints.  Where a denominator is zero:

  snr_db      N = Srr - 2 Sre + See:  Srr > 0, N = 0 -> +inf;  Srr = 0, N > 0 -> -inf;  both 0 -> nan
  si_sdr_db   T = Sre^2, D = Srr See - T (>= 0 by Cauchy-Schwarz):  T > 0, D = 0 -> +inf;  T = 0, D > 0 -> -inf;  both 0 -> nan
  segsnr_db   no frame used -> nan
  stoi        no term (fewer than 30 kept frames) -> nan
  hit, fa     no ideal unit on (off) -> nan; hit_fa is nan if either is

All arguments are host arrays; there is no CPU fallback.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .dnn import _i16_list, _ptr_array, dnn_enhance_utterances
from .engine import _np_ptr

NCHAN = 64
SKIPPED_BITS = 0x7FC00000  # frame_db of a frame whose reference is silent


def score_frames(length, hop=160):
    """frames of 2 hop samples every hop in an utterance of `length` samples (at hop 160: dnn_rows)"""
    return (int(length) - 2 * hop) // hop + 1 if length >= 2 * hop else 0


def ratio_db(num, den):
    """10 log10 (num / den) of two exact non-negative ints: the quotient rounded once, its logarithm, times 10"""
    num, den = int(num), int(den)
    if den == 0:
        return math.inf if num > 0 else math.nan
    if num == 0:
        return -math.inf
    return 10.0 * math.log10(num / den)


def snr_db(srr, see, sre):
    srr, see, sre = int(srr), int(see), int(sre)
    return ratio_db(srr, srr - 2 * sre + see)


def si_sdr_db(srr, see, sre):
    srr, see, sre = int(srr), int(see), int(sre)
    return ratio_db(sre * sre, srr * see - sre * sre)


def _div(a, b):
    return a / b if b else math.nan


def score_utterances(refs, ests, hop=160, frames=False):
    """Clean (refs) and enhanced (ests) int16 utterances of equal lengths -> dict of arrays over the list: srr, see, sre (int64,
    exact, over all samples), snr_db, si_sdr_db, segsnr_db (float64), seg_sum (float64), seg_frames (int32); frames=True adds
    frame_db, the list of float32 [F_u] arrays (nan where the reference frame is silent)."""
    lib = _lib.load()
    refs, lens = _i16_list(refs)
    ests, elens = _i16_list(ests)
    if len(refs) != len(ests) or any(r.size != e.size for r, e in zip(refs, ests)):
        raise ValueError("score_utterances: one estimate per reference, of the same length")
    n = len(refs)
    sums = np.zeros((n, 3), np.int64)
    seg_sum, seg_frames = np.zeros(n, np.float64), np.zeros(n, np.int32)
    db = [np.zeros(score_frames(r.size, hop), np.float32) for r in refs] if frames else None
    rc = lib.sea_score_utterances(_ptr_array(refs), _ptr_array(ests), lens, n, int(hop), _np_ptr(sums), _np_ptr(seg_sum),
                                  _np_ptr(seg_frames), _ptr_array(db) if frames else None)
    _lib.check(rc, "sea_score_utterances")
    out = dict(srr=sums[:, 0].copy(), see=sums[:, 1].copy(), sre=sums[:, 2].copy(), seg_sum=seg_sum, seg_frames=seg_frames,
               snr_db=np.array([snr_db(*s) for s in sums.tolist()], np.float64),
               si_sdr_db=np.array([si_sdr_db(*s) for s in sums.tolist()], np.float64),
               segsnr_db=np.array([_div(float(s), int(k)) for s, k in zip(seg_sum, seg_frames)], np.float64))
    if frames:
        out["frame_db"] = db
    return out


def hit_fa(n11, n10, n01, n00):
    """(hit, fa, hit - fa) from the counts est on / ideal on, est on / ideal off, est off / ideal on, both off"""
    hit, fa = _div(int(n11), int(n11) + int(n01)), _div(int(n10), int(n10) + int(n00))
    return hit, fa, hit - fa


def mask_scores(est, ideal, t_est=0.5, t_ideal=0.5):
    """Lists of estimated and ideal masks [F_u][64] -> dict: counts (int64 [n][4]: n11, n10, n01, n00), hit, fa, hit_fa (float64
    [n]) and `pooled`, the same four entries over all units of the list.  A unit is on iff value > threshold."""
    lib = _lib.load()
    est = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, NCHAN) for m in est]
    ideal = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, NCHAN) for m in ideal]
    if len(est) != len(ideal) or any(a.shape != b.shape for a, b in zip(est, ideal)):
        raise ValueError("mask_scores: one ideal mask per estimated mask, of the same shape")
    n = len(est)
    n_rows = (ctypes.c_int * max(n, 1))(*[m.shape[0] for m in est])
    counts = np.zeros((n, 4), np.int64)
    rc = lib.sea_mask_score_utterances(_ptr_array(est), _ptr_array(ideal), n_rows, n, float(t_est), float(t_ideal), _np_ptr(counts))
    _lib.check(rc, "sea_mask_score_utterances")
    rates = np.array([hit_fa(*c) for c in counts.tolist()], np.float64).reshape(n, 3)
    total = counts.sum(axis=0)
    ph, pf, phf = hit_fa(*total.tolist())
    return dict(counts=counts, hit=rates[:, 0], fa=rates[:, 1], hit_fa=rates[:, 2],
                pooled=dict(counts=total, hit=ph, fa=pf, hit_fa=phf))


def dnn_score_utterances(model, noisy, clean):
    """dnn_enhance_utterances (model, noisy) scored against `clean`, beside the noisy input's own scores:
    {'enhanced': score_utterances (clean, enhanced), 'noisy': score_utterances (clean, noisy), 'gain_db': their differences in
    snr_db, si_sdr_db and segsnr_db}."""
    enhanced = score_utterances(clean, dnn_enhance_utterances(model, noisy))
    before = score_utterances(clean, noisy)
    return dict(enhanced=enhanced, noisy=before,
                gain_db={k: enhanced[k] - before[k] for k in ("snr_db", "si_sdr_db", "segsnr_db")})


def stoi_frames(length, rate=16000):
    """frames of 256 samples every 128 in an utterance of `length` samples once it is resampled to 10 kHz"""
    q = {16000: 8, 8000: 4}[int(rate)]
    l10 = (5 * int(length) + q - 1) // q
    return (l10 - 256) // 128 + 1 if l10 >= 256 else 0


def stoi_utterances(refs, ests, rate=16000, terms=False):
    """Clean (refs) and enhanced (ests) int16 utterances of equal lengths at 16000 or 8000 Hz -> dict of arrays over the list:
    stoi (float64; stoi_sum / stoi_terms, nan without a term), stoi_sum (float64), stoi_terms (int64), frames and kept (int32:
    the frames at 10 kHz, and those within 40 dB of the reference's loudest); terms=True adds d, the list of float32 [S_u][15]
    arrays of the intermediate measure per 30-frame segment and third-octave band."""
    lib = _lib.load()
    refs, lens = _i16_list(refs)
    ests, elens = _i16_list(ests)
    if len(refs) != len(ests) or any(r.size != e.size for r, e in zip(refs, ests)):
        raise ValueError("stoi_utterances: one estimate per reference, of the same length")
    n = len(refs)
    stoi_sum, stoi_terms, fk = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
    d = [np.zeros((max(stoi_frames(r.size, rate) - 29, 0), 15), np.float32) for r in refs] if terms else None
    rc = lib.sea_stoi_utterances(_ptr_array(refs), _ptr_array(ests), lens, n, int(rate), _np_ptr(stoi_sum), _np_ptr(stoi_terms),
                                 _np_ptr(fk), _ptr_array(d) if terms else None)
    _lib.check(rc, "sea_stoi_utterances")
    out = dict(stoi=np.array([_div(float(s), int(k)) for s, k in zip(stoi_sum, stoi_terms)], np.float64), stoi_sum=stoi_sum,
               stoi_terms=stoi_terms, frames=fk[:, 0].copy(), kept=fk[:, 1].copy())
    if terms:
        out["d"] = [a[:int(k) // 15] for a, k in zip(d, stoi_terms)]
    return out


def stoi_last_chunks():
    """How many chunks the last stoi_utterances call of this thread was cut into (SEA_SCORE_SCRATCH_MB sets the budget)."""
    return int(_lib.load().sea_stoi_last_chunks())


def score_last_chunks():
    """How many chunks the last list call of this thread was cut into (SEA_SCORE_SCRATCH_MB sets the budget)."""
    return int(_lib.load().sea_score_last_chunks())
