"""The front half of the Hu-Wang mask estimator createIBM() at 16 kHz on the 64-channel gammatone bank (HuWang.cpp:41-76 at the
constants of resyth_64sub_IBM/cpp/HuWang.h; csrc/hw64_kernel.hip), over libsea_mi355x.so: AudiPeriph, lowPass, computeACF,
crossCorr, globalPitch, timeCrn and the initial labelling.  The functions have the shapes and the result class of their
hw25_* namesakes at 64 channels, 201 delays and a hop of 160 samples, and share their bodies (hw25.py).  initGroup onwards is
not built at 16 kHz.

torch is used for device memory and streams only (plumbing); all compute is in the HIP library.
"""
from types import SimpleNamespace

from . import _lib
from .hw25 import Hw25Result, _bank_front, _bank_frontend_host, _bank_periphery, _bank_split, _bank_tables

HW64_NCHAN, HW64_DELAYS, HW64_HOP = 64, 201, 160
_BANK64 = SimpleNamespace(name="hw64", nchan=HW64_NCHAN, delays=HW64_DELAYS, hop=HW64_HOP, taps=181, gout_fn=None, scratch_fn=None)


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
