"""The front half of the Hu-Wang mask estimator createIBM() at 16 kHz on the 64-channel gammatone bank (HuWang.cpp:41-76 at the
constants of resyth_64sub_IBM/cpp/HuWang.h; csrc/hw64_kernel.hip), over libsea_mi355x.so: AudiPeriph, lowPass, computeACF,
crossCorr, globalPitch, timeCrn and the initial labelling.  The functions have the shapes and the result class of their
hw25_* namesakes at 64 channels, 201 delays and a hop of 160 samples, and share their bodies (hw25.py).

Then createIBM():79-87, initGroup and pitchDtm (csrc/hw64_pitch_kernel.hip): the pitch contour of the dominant voiced source and
the units grouped with it or against it, hw64_pitch_batch / hw64_pitch.  The reference's leftDevelope and rightDevelope bound
two loops by the literal 40; on this bank that keeps channels 40..63 out of their votes (the 25-band bank reads the cross
array there instead, which is why only its call takes one).

Then createIBM():89-106, computeAM, finalSeg and the binarisation (csrc/hw64_am_kernel.hip): hw64_am_batch, hw64_finalseg_batch
and the whole estimator, hw64_ibm_batch / hw64_ibm, the binary mask [frames][64] from 16 kHz audio.

Then resynthesis() (HuWang.cpp:1498-1549; csrc/hw64_resynth_kernel.hip), which closes the chain at this bank: hw64_resynth and
hw64_enhance for one utterance from host memory, hw64_resynth_utterances and hw64_enhance_utterances for lists of utterances,
cut into chunks that fit HBM (hw64_enhance_plan shows the cut).  These take host arrays only: the forms on a PackedBatch
(hw64_resynth_batch, hw64_enhance_batch) wait for the exported device-pointer calls they would bind.

torch is used for device memory and streams only (plumbing); all compute is in the HIP library.
"""
import ctypes
from types import SimpleNamespace

import numpy as np

from . import _lib
from .engine import _np_ptr
from .hw25 import (Hw25AmResult, Hw25MaskResult, Hw25PitchResult, Hw25Result, _bank_am, _bank_finalseg, _bank_front,
                   _bank_frontend_host, _bank_ibm, _bank_periphery, _bank_pitch, _bank_split, _bank_tables, _hw25_host)

HW64_NCHAN, HW64_DELAYS, HW64_HOP = 64, 201, 160
HW64_STAGE_WORDS = 5 + 2 * HW64_NCHAN
_BANK64 = SimpleNamespace(name="hw64", nchan=HW64_NCHAN, delays=HW64_DELAYS, hop=HW64_HOP, taps=181, gout_fn=None, scratch_fn=None,
                          pitch_reads_cross=False)


class Hw64Result(Hw25Result):
    """What hw64_frontend_batch() computed: Hw25Result's tensors at 64 channels -- hout, hev (64x the packed size), cross_hc,
    cross_ev, pratio, mark [rows][64], pitch int32 [rows] (32..200, in samples at 16 kHz), acf_hc, acf_ev [rows][64][201] or
    None; utterance u has length // 160 rows."""
    NCHAN = HW64_NCHAN


def hw64_tables():
    """The bank's host tables: cf, bw, midEarCoeff, gain, f1, f2 [64], winsize int32 [64], lp [181] (lowPass's Kaiser taps) and
    hair [10] = ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0."""
    return _bank_tables(_BANK64)


def hw64_periphery_batch(batch, use_order=True, gout=False):
    """AudiPeriph + lowPass for every utterance of the batch: (hOut, hEv), with gout (hOut, hEv, gOut): float32 tensors of 64x
    the packed size; utterance u's [64][pitch] block starts at offsets[u]*64, pitch = length rounded up to 8 (hw64_split cuts
    them).  gOut is the gammatone filters' output before the hair cell."""
    return _bank_periphery(_BANK64, batch, use_order, gout)


def hw64_split(batch, tensor):
    """A hw64_periphery_batch() tensor -> per-utterance numpy arrays [64][L]."""
    return _bank_split(_BANK64, batch, tensor)


def hw64_correlogram_batch(batch, hout, hev, want_acf=False, use_order=True):
    """computeACF, crossCorr, globalPitch, timeCrn and the initial labelling from hw64_periphery_batch()'s tensors."""
    return _bank_front(_BANK64, Hw64Result, batch, want_acf, use_order, hout, hev)


def hw64_frontend_batch(batch, want_acf=False, use_order=True):
    """The front half of createIBM() at 16 kHz for every utterance of the batch, one launch group on the current stream ->
    Hw64Result.  The ACFs are [rows][64][201] floats per stream (about 41 MB per 4 s utterance): computed always, written only
    on request."""
    return _bank_front(_BANK64, Hw64Result, batch, want_acf, use_order)


def hw64_frontend(x, want_acf=True):
    """One utterance from host memory (float32 or int16 samples on the int16 scale) -> dict under the reference's names:
    hOut, hEv [64][L]; acf_hc, acf_ev [F][64][201] (None without want_acf); cross_hc, cross_ev, pRatio, mark [F][64]; pitch [F]."""
    return _bank_frontend_host(_BANK64, x, want_acf)


def hw64_workgroups_per_utterance(n_utt):
    """How many workgroups the correlogram launch gives every utterance of a batch of n_utt on the current device."""
    return int(_lib.load().sea_hw64_workgroups_per_utterance(int(n_utt)))


class Hw64PitchResult(Hw25PitchResult):
    """What hw64_pitch_batch() computed: Hw25PitchResult's tensors at 64 channels -- pitch int32 [rows] (0 = unvoiced, else the
    delay 32..200 in samples at 16 kHz), grp [rows][64] in {-1, 0, +1}, pratio [rows][64], status int32 [n_utt] (bits 0..15 the
    segment count, HW25_TOO_MANY_SEGMENTS, HW25_CHANMARK_UNSET), stages (HW64_STAGE_WORDS int32 words per row, or None) and
    front, the Hw64Result they were computed from.  utterance(u): numpy arrays, the stage arrays under HW25_PITCH_STAGES /
    HW25_GRP_STAGES when they were asked for."""
    NCHAN = HW64_NCHAN
    STAGE_WORDS = HW64_STAGE_WORDS


def hw64_pitch_batch(batch, stages=False, use_order=True):
    """createIBM():41-87 at 16 kHz for every utterance of the batch: the front half with its ACF output (51 456 B per row), then
    initGroup and pitchDtm, one launch group on the current stream -> Hw64PitchResult.  stages: also keep Pitch / Grp after
    every step of pitchDtm."""
    return _bank_pitch(_BANK64, Hw64Result, Hw64PitchResult, batch, stages, use_order)


def hw64_pitch(x):
    """One utterance from host memory (float32 or int16 samples on the int16 scale, 16 kHz) -> dict: pitch int32 [F], grp and
    pratio [F][64], status; F = len(x) // 160."""
    return _hw25_host("sea_hw64_pitch", x, ("pitch", "grp", "pratio"), bank=_BANK64)


def hw64_pitch_waves_per_utterance(n_utt):
    """How many waves the pitch stage's two frame-walking kernels give every utterance of a batch of n_utt on the current device."""
    return int(_lib.load().sea_hw64_pitch_waves_per_utterance(int(n_utt)))


class Hw64AmResult(Hw25AmResult):
    """What hw64_am_batch() computed: Hw25AmResult's tensors at 64 channels -- amcrn [rows][64] 0 / 1, status int32 [n_utt]
    (HW25_AM_TOO_LONG, HW25_AM_BAD_PITCH) and, when asked for, ratio and seng [rows][64], ampatt and am (gOut's layout)."""
    NCHAN = HW64_NCHAN


class Hw64MaskResult(Hw25MaskResult):
    """What hw64_finalseg_batch() / hw64_ibm_batch() computed: Hw25MaskResult's tensors at 64 channels -- mask [rows][64] 0 / 1,
    status int32 [n_utt], grp_final [rows][64] or None, pitch int32 [rows] or None, stages (floats, [5][rows_u][64] per
    utterance, or None).  utterance(u): numpy arrays, the stage arrays under HW25_FINAL_STAGES when they were asked for."""
    NCHAN = HW64_NCHAN


def hw64_am_batch(batch, gout, pitch, row_offsets=None, want_details=False, use_order=True):
    """computeAM at 16 kHz for every utterance of the batch from hw64_periphery_batch(gout=True)'s gOut and hw64_pitch_batch()'s
    pitch (int32 [rows] on the device, 0 or 32..200; row_offsets: the int64 device tensor that goes with it) -> Hw64AmResult.
    want_details: also ratio, seng, ampatt and am."""
    return _bank_am(_BANK64, Hw64AmResult, batch, gout, pitch, row_offsets, want_details, use_order)


def hw64_finalseg_batch(grp, amcrn, cross_ev, pratio, lengths, row_offsets, host_rows, stages=False, use_order=None):
    """finalSeg and the binarisation on device tensors [rows][64] (hw64_pitch_batch()'s grp and pratio, hw64_am_batch()'s amcrn,
    the front half's cross_ev), lengths / row_offsets int64 [n_utt] on the device, host_rows the row counts -> Hw64MaskResult.
    use_order: an int32 device tensor (launch order) or None."""
    return _bank_finalseg(_BANK64, Hw64MaskResult, grp, amcrn, cross_ev, pratio, lengths, row_offsets, host_rows, stages, use_order)


def hw64_ibm_batch(batch, stages=False, use_order=True):
    """createIBM() at 16 kHz for every utterance of the batch, one launch group on the current stream -> Hw64MaskResult with the
    binary mask [rows][64], pitchDtm's pitch [rows] and the status (hw64_pitch_batch()'s with HW25_FINAL_TOO_MANY_SEGMENTS,
    HW25_AM_TOO_LONG).  stages: also keep Grp after each of finalSeg's five steps."""
    return _bank_ibm(_BANK64, Hw64MaskResult, batch, stages, use_order)


def hw64_ibm(x):
    """createIBM (x) for one utterance from host memory (float32 or int16 samples on the int16 scale, 16 kHz) -> dict: mask
    [F][64] floats 0 / 1, pitch int32 [F], status; F = len(x) // 160."""
    return _hw25_host("sea_hw64_ibm", x, ("mask", "pitch"), bank=_BANK64)


# ------------------------------------------------------------------------------------------------
# the estimator's resynthesis at 16 kHz (HuWang.cpp:1498-1549; csrc/hw64_resynth_kernel.hip): the mask applied, audio out
# ------------------------------------------------------------------------------------------------
def hw64_resynth_tables():
    """The overlap-add tables of resynthesis() at WINDOW = 320 = 2 x 160: up float64 [160], down float64 [160] and w float32
    [160][4], the weight at position o of a hop for the four states (bit 0 / 1: frame k / k + 1 exists and is set)."""
    lib = _lib.load()
    w, up, down = np.zeros((160, 4), np.float32), np.zeros(160, np.float64), np.zeros(160, np.float64)
    _lib.check(lib.sea_hw64_resynth_tables_host(_np_ptr(w), _np_ptr(up), _np_ptr(down)), "sea_hw64_resynth_tables_host")
    return dict(w=w, up=up, down=down)


def hw64_resynth(x, mask, threshold=0.0):
    """One utterance from host memory (float32 or int16 samples on the int16 scale, 16 kHz) and its mask [len(x) // 160][64]
    (a unit is set where mask > threshold) -> the resynthesised float32 audio [len(x)]."""
    mask = np.ascontiguousarray(mask, dtype=np.float32).reshape(-1, HW64_NCHAN)
    return _hw25_host("sea_hw64_resynth", x, ("audio",), _np_ptr(mask), mask.shape[0], float(threshold), status=False,
                      bank=_BANK64)["audio"]


def hw64_enhance(x):
    """One utterance from host memory (float32 or int16 samples on the int16 scale, 16 kHz) -> dict: audio float32 [L], the
    enhanced signal; mask [F][64] floats 0 / 1, pitch int32 [F], status, as hw64_ibm() gives them; F = len(x) // 160."""
    return _hw25_host("sea_hw64_enhance", x, ("audio", "mask", "pitch"), bank=_BANK64)


def _ptr_array(arrays):
    return (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays]) if arrays is not None else None


def _host_list(xs):
    xs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in xs]
    return xs, (ctypes.c_long * max(len(xs), 1))(*[x.size for x in xs])


def hw64_resynth_utterances(xs, masks, threshold=0.0, int16=False):
    """resynthesis() for a list of utterances in host memory (float32 or int16 samples on the int16 scale, 16 kHz) with their
    masks [len(x) // 160][64] -> dict: audio, the list of float32 arrays; int16=True: also shorts, their int16 conversion as
    the x86-64 build performs it; chunks, how many launch groups the list was cut into to fit HBM."""
    lib = _lib.load()
    xs, lens = _host_list(xs)
    masks = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, HW64_NCHAN) for m in masks]
    if len(masks) != len(xs) or any(m.shape[0] != x.size // HW64_HOP for x, m in zip(xs, masks)):
        raise ValueError("hw64_resynth_utterances: one mask [len(x) // 160][64] per utterance")
    audio = [np.zeros(x.size, np.float32) for x in xs]
    shorts = [np.zeros(x.size, np.int16) for x in xs] if int16 else None
    rc = lib.sea_hw64_resynth_utterances(_ptr_array(xs), lens, _ptr_array(masks), float(threshold), _ptr_array(audio),
                                         _ptr_array(shorts), len(xs))
    _lib.check(rc, "sea_hw64_resynth_utterances")
    out = dict(audio=audio, chunks=int(lib.sea_hw64_enhance_last_chunks()))
    if int16:
        out["shorts"] = shorts
    return out


def hw64_enhance_utterances(xs, int16=False):
    """createIBM() followed by resynthesis() of its own mask for a list of utterances in host memory (float32 or int16 samples
    on the int16 scale, 16 kHz) -> dict of lists: audio float32 [L], mask [F][64] floats 0 / 1, pitch int32 [F] (F = L // 160),
    status, as hw64_ibm() gives them; int16=True: also shorts; and chunks, how many launch groups the list was cut into to fit
    HBM (the estimator's scratch is about 200 MB per four-second utterance)."""
    lib = _lib.load()
    xs, lens = _host_list(xs)
    n = len(xs)
    audio = [np.zeros(x.size, np.float32) for x in xs]
    shorts = [np.zeros(x.size, np.int16) for x in xs] if int16 else None
    masks = [np.zeros((x.size // HW64_HOP, HW64_NCHAN), np.float32) for x in xs]
    pitch = [np.zeros(x.size // HW64_HOP, np.int32) for x in xs]
    status = np.zeros(max(n, 1), np.int32)
    rc = lib.sea_hw64_enhance_utterances(_ptr_array(xs), lens, n, _ptr_array(audio), _ptr_array(shorts), _ptr_array(masks),
                                         _ptr_array(pitch), _np_ptr(status))
    _lib.check(rc, "sea_hw64_enhance_utterances")
    out = dict(audio=audio, mask=masks, pitch=pitch, status=[int(v) for v in status[:n]], chunks=int(lib.sea_hw64_enhance_last_chunks()))
    if int16:
        out["shorts"] = shorts
    return out


def hw64_enhance_plan(lengths, budget_bytes, resynth_only=False):
    """How hw64_enhance_utterances (resynth_only: hw64_resynth_utterances) cuts a list of these lengths for a budget in bytes:
    the first utterance of every chunk, then len(lengths) -- int32 [chunks + 1].  Touches no device."""
    lib = _lib.load()
    n = len(lengths)
    lens = (ctypes.c_long * max(n, 1))(*[int(v) for v in lengths])
    cuts = np.zeros(n + 1, np.int32)
    k = int(lib.sea_hw64_enhance_plan(lens, n, int(budget_bytes), int(bool(resynth_only)), _np_ptr(cuts)))
    if k < 0:
        _lib.check(1, "sea_hw64_enhance_plan")
    return cuts[:k + 1].copy()
