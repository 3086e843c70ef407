"""The Hu-Wang mask estimator createIBM() and its resynthesis on the 25-channel 8 kHz gammatone bank
(aurora_etsi_test/HuWang.cpp), over libsea_mi355x.so: the batched, HBM-resident forms (hw25_*_batch on a PackedBatch) and the
forms that take one utterance from host memory.

torch is used for device memory and streams only (plumbing); all compute is in the HIP library.
"""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .engine import _dptr, _np_ptr, _row_offsets, _stream_ptr, _torch

HW25_NCHAN, HW25_DELAYS, HW25_HOP = 25, 101, 80
# what the front half's wrappers need to know of a bank (hw64.py has the 64-channel one): its sizes and its calls' names;
# gout_fn: the periphery call that also returns gOut, where the bank has one of its own (None: periphery_fn takes a null);
# pitch_reads_cross: whether the bank's pitch call takes the front half's cross_hc (hw64.py says why the 64-channel one does not)
_BANK25 = SimpleNamespace(name="hw25", nchan=HW25_NCHAN, delays=HW25_DELAYS, hop=HW25_HOP, taps=91,
                          gout_fn="sea_hw25_periphery_gout_batch", scratch_fn="sea_hw25_scratch_bytes", pitch_reads_cross=True)


# ------------------------------------------------------------------------------------------------
# what the wrappers share
# ------------------------------------------------------------------------------------------------
def _hw25_input(batch):
    """createIBM takes float samples on the int16 scale: an int16 batch converts exactly, a float32 one is used as it is"""
    torch = _torch()
    if batch.data.dtype == torch.float32:
        return batch.data
    if batch.data.dtype != torch.int16:
        raise ValueError("hw25: the batch must hold int16 or float32 samples")
    return batch.data.to(torch.float32)


def _hw25_start(batch, dev=None, row_offsets=None, zeros=(), bank=_BANK25):
    """What a batch wrapper starts with: x, the float input (only without dev: the wrappers that are given device tensors pass
    their device); rows and offs, length // 80 (the bank's hop) rows per utterance and where they begin (host); d_offs, row_offsets or the
    device copy of offs; n, the rows of the batch, and total, its packed samples (at least 1 and 8, so that no tensor is
    empty); and the zeroed outputs named in zeros: mask [n][25], pitch int32 [n], status int32 [n_utt]."""
    torch = _torch()
    s = SimpleNamespace(dev=dev)
    if dev is None:
        s.x = _hw25_input(batch)
        s.dev = s.x.device
    s.rows, s.offs = batch.frame_rows(bank.hop)
    s.d_offs = row_offsets if row_offsets is not None else torch.from_numpy(s.offs).to(s.dev)
    s.n, s.total = max(int(s.rows.sum()), 1), max(int(batch.total), 8)
    shapes = dict(mask=((s.n, bank.nchan), torch.float32), pitch=(s.n, torch.int32), status=(max(batch.n_utt, 1), torch.int32))
    for k in zeros:
        setattr(s, k, torch.zeros(shapes[k][0], dtype=shapes[k][1], device=s.dev))
    return s


def _hw25_order(batch, use_order):
    return _dptr(batch.order) if use_order else None


class _Hw25Rows:
    """The results' common part: the keyword attributes, and utterance u's share of a device tensor as numpy.  host_row_offsets
    and host_rows say where its rows are (Hw25PitchResult: its front's), batch where its samples are."""
    NCHAN = HW25_NCHAN

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def _rows(self, u, t, width=1):
        """utterance u's rows of t, a tensor of `width` entries (or of one [..] entry) per row; None stays None"""
        if t is None:
            return None
        src = getattr(self, "front", self)
        r0, n = int(src.host_row_offsets[u]), int(src.host_rows[u])
        return t[r0 * width:(r0 + n) * width].cpu().numpy()

    def _block(self, u, t):
        """utterance u's [25][L] block of a tensor of 25x the packed size (a view into its padded [25][pitch] copy)"""
        off, L, nch = int(self.batch.host_offsets[u]), int(self.batch.host_lengths[u]), self.NCHAN
        pitch = (L + 7) // 8 * 8
        return t[off * nch:off * nch + nch * pitch].cpu().numpy().reshape(nch, pitch)[:, :L]


def _hw25_host(fn, x, keys, *args, status=True, bank=_BANK25):
    """The one body of the forms that take one utterance from host memory: x as contiguous float32, the zeroed outputs named
    in keys (audio [L], pitch int32 [F], every other [F][25], the bank's channels), the call fn (x, L, *args, *outputs[, status])
    -> the outputs as a dict, with the status word where the call has one."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L, F = x.size, x.size // bank.hop
    shape = dict(audio=L, pitch=F)
    r = {k: np.zeros(shape.get(k, (F, bank.nchan)), np.int32 if k == "pitch" else np.float32) for k in keys}
    word = np.zeros(1, np.int32)
    rc = getattr(_lib.load(), fn)(_np_ptr(x), L, *args, *[_np_ptr(r[k]) for k in keys], *([_np_ptr(word)] if status else []))
    _lib.check(rc, fn)
    if status:
        r["status"] = int(word[0])
    return r


# ------------------------------------------------------------------------------------------------
# the estimator's front half (HuWang.cpp:41-76; csrc/hw25_kernel.hip)
# ------------------------------------------------------------------------------------------------
def _bank_tables(bank):
    lib = _lib.load()
    t = {k: np.zeros(bank.nchan, np.float32) for k in ("cf", "bw", "midEarCoeff", "gain", "f1", "f2")}
    t.update(winsize=np.zeros(bank.nchan, np.int32), lp=np.zeros(bank.taps, np.float32), hair=np.zeros(10, np.float32))
    keys = ("cf", "bw", "midEarCoeff", "gain", "f1", "f2", "winsize", "lp", "hair")
    fn = f"sea_{bank.name}_tables_host"
    _lib.check(getattr(lib, fn)(*[_np_ptr(t[k]) for k in keys]), fn)
    return t


def hw25_tables():
    """The bank's host tables: cf, bw, midEarCoeff, gain, f1, f2 [25], winsize int32 [25], lp [91] (lowPass's Kaiser taps) and
    hair [10] = ymdt, xdt, ydt, lplusrdt, rdt, gdt, hdt, q0, c0, w0."""
    return _bank_tables(_BANK25)


def _bank_periphery(bank, batch, use_order, want_gout):
    torch = _torch()
    lib = _lib.load()
    x = _hw25_input(batch)
    hout = torch.zeros(batch.total * bank.nchan, dtype=torch.float32, device=x.device)
    outs = [hout] + [torch.zeros_like(hout) for _ in range(2 if want_gout else 1)]
    ptrs = [_dptr(t) for t in outs]
    fn = f"sea_{bank.name}_periphery_batch"
    if bank.gout_fn and want_gout:
        fn = bank.gout_fn
    elif not bank.gout_fn and not want_gout:
        ptrs.append(None)
    rc = getattr(lib, fn)(_dptr(x), *ptrs, _dptr(batch.offsets), _dptr(batch.lengths), _hw25_order(batch, use_order),
                          batch.n_utt, _stream_ptr())
    _lib.check(rc, fn)
    return tuple(outs)


def _hw25_periphery(batch, use_order, want_gout):
    return _bank_periphery(_BANK25, batch, use_order, want_gout)


def hw25_periphery_batch(batch, use_order=True):
    """AudiPeriph + lowPass for every utterance of the batch: (hOut, hEv), two float32 tensors of 25x the packed size;
    utterance u's [25][pitch] block starts at offsets[u]*25, pitch = length rounded up to 8 (hw25_split cuts them)."""
    return _hw25_periphery(batch, use_order, False)


def _bank_split(bank, batch, tensor):
    host = tensor.detach().cpu().numpy()
    out, nch = [], bank.nchan
    for off, L in zip(batch.host_offsets, batch.host_lengths):
        pitch = (int(L) + 7) // 8 * 8
        out.append(host[off * nch:off * nch + nch * pitch].reshape(nch, pitch)[:, :int(L)].copy())
    return out


def hw25_split(batch, tensor):
    """A hw25_periphery_batch() tensor -> per-utterance numpy arrays [25][L]."""
    return _bank_split(_BANK25, batch, tensor)


class Hw25Result(_Hw25Rows):
    """What hw25_frontend_batch() computed, device tensors: hout, hev (25x the packed size), cross_hc, cross_ev, pratio, mark
    [rows][25], pitch int32 [rows], acf_hc, acf_ev [rows][25][101] or None; row_offsets / host_row_offsets / host_rows say
    where utterance u's length // 80 rows are.  utterance(u) returns numpy views of one utterance under the reference's names."""

    def __init__(self, batch, **kw):
        super().__init__(batch=batch, **kw)

    def utterance(self, u):
        def rows(t):
            return self._rows(u, t)

        return dict(hOut=self._block(u, self.hout), hEv=self._block(u, self.hev), acf_hc=rows(self.acf_hc), acf_ev=rows(self.acf_ev),
                    cross_hc=rows(self.cross_hc), cross_ev=rows(self.cross_ev), pitch=rows(self.pitch), pRatio=rows(self.pratio),
                    mark=rows(self.mark))


def _bank_front(bank, result, batch, want_acf, use_order, hout=None, hev=None):
    """the one body of the correlogram wrappers (hout and hev given) and the front-half wrappers (computed here, in the same
    launch group) of both banks; the frame outputs have at least one row, so that no tensor is empty"""
    torch = _torch()
    lib = _lib.load()
    whole = hout is None
    nch = bank.nchan
    s = _hw25_start(batch, dev=None if whole else hout.device, zeros=("pitch",), bank=bank)
    fr = {k: torch.zeros((s.n, nch), dtype=torch.float32, device=s.dev) for k in ("cross_hc", "cross_ev", "pratio", "mark")}
    acf = [torch.zeros((s.n, nch, bank.delays), dtype=torch.float32, device=s.dev) if want_acf else None for _ in range(2)]
    nbytes = int(getattr(lib, bank.scratch_fn)(int(batch.total), int(batch.n_utt))) if bank.scratch_fn else 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=s.dev) if nbytes else None
    if whole:
        hout = torch.zeros(batch.total * nch, dtype=torch.float32, device=s.dev)
        hev = torch.zeros_like(hout)
    fn = f"sea_{bank.name}_frontend_batch" if whole else f"sea_{bank.name}_correlogram_batch"
    rc = getattr(lib, fn)(*([_dptr(s.x)] if whole else []), _dptr(hout), _dptr(hev), _dptr(batch.offsets), _dptr(batch.lengths),
                          _dptr(s.d_offs), _dptr(acf[0]), _dptr(acf[1]), _dptr(fr["cross_hc"]), _dptr(fr["cross_ev"]), _dptr(s.pitch),
                          _dptr(fr["pratio"]), _dptr(fr["mark"]), _dptr(scratch), _hw25_order(batch, use_order), batch.n_utt,
                          _stream_ptr())
    _lib.check(rc, fn)
    return result(batch, hout=hout, hev=hev, acf_hc=acf[0], acf_ev=acf[1], pitch=s.pitch, row_offsets=s.d_offs,
                  host_row_offsets=s.offs, host_rows=s.rows, **fr)


def hw25_correlogram_batch(batch, hout, hev, want_acf=False, use_order=True):
    """computeACF, crossCorr, globalPitch, timeCrn and the initial labelling from hw25_periphery_batch()'s tensors."""
    return _bank_front(_BANK25, Hw25Result, batch, want_acf, use_order, hout, hev)


def hw25_frontend_batch(batch, want_acf=False, use_order=True):
    """The front half of createIBM() for every utterance of the batch, one launch group on the current stream -> Hw25Result.
    The ACFs are [rows][25][101] floats per stream (about 8 MB per 4 s utterance): computed always, written only on request."""
    return _bank_front(_BANK25, Hw25Result, batch, want_acf, use_order)


def _bank_frontend_host(bank, x, want_acf):
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    L, F, nch = x.size, x.size // bank.hop, bank.nchan
    r = dict(hOut=np.zeros((nch, L), np.float32), hEv=np.zeros((nch, L), np.float32),
             acf_hc=np.zeros((F, nch, bank.delays), np.float32) if want_acf else None,
             acf_ev=np.zeros((F, nch, bank.delays), np.float32) if want_acf else None,
             cross_hc=np.zeros((F, nch), np.float32), cross_ev=np.zeros((F, nch), np.float32),
             pitch=np.zeros(F, np.int32), pRatio=np.zeros((F, nch), np.float32), mark=np.zeros((F, nch), np.float32))
    keys = ("hOut", "hEv", "acf_hc", "acf_ev", "cross_hc", "cross_ev", "pitch", "pRatio", "mark")
    fn = f"sea_{bank.name}_frontend"
    rc = getattr(lib, fn)(_np_ptr(x), L, *[_np_ptr(r[k]) if r[k] is not None else None for k in keys])
    _lib.check(rc, fn)
    return r


def hw25_frontend(x, want_acf=True):
    """One utterance from host memory (float32 or int16 samples on the int16 scale) -> dict under the reference's names:
    hOut, hEv [25][L]; acf_hc, acf_ev [F][25][101] (None without want_acf); cross_hc, cross_ev, pRatio, mark [F][25]; pitch [F]."""
    return _bank_frontend_host(_BANK25, x, want_acf)


# ------------------------------------------------------------------------------------------------
# the estimator's initial grouping and pitch tracking (HuWang.cpp:79-87: initGroup, pitchDtm; csrc/hw25_pitch_kernel.hip)
# ------------------------------------------------------------------------------------------------
HW25_STAGE_WORDS, HW25_TOO_MANY_SEGMENTS, HW25_CHANMARK_UNSET = 55, 1 << 16, 1 << 17
HW25_PITCH_STAGES = ("pitch_find1", "pitch_find2", "pitch_check", "pitch_left", "pitch_right")
HW25_GRP_STAGES = ("grp_init", "grp_thetap")


class Hw25PitchResult(_Hw25Rows):
    """What hw25_pitch_batch() computed, device tensors: pitch int32 [rows] (0 = unvoiced, else the delay 16..100 in samples
    at 8 kHz), grp [rows][25] in {-1, 0, +1} (+1: grouped with the dominant voiced source), pratio [rows][25], status int32
    [n_utt] (bits 0..15 the segment count, HW25_TOO_MANY_SEGMENTS, HW25_CHANMARK_UNSET), stages (int32 words, or None) and
    front, the Hw25Result they were computed from.  utterance(u) returns numpy arrays of one utterance, the stage arrays
    under HW25_PITCH_STAGES / HW25_GRP_STAGES when they were asked for."""
    STAGE_WORDS = HW25_STAGE_WORDS

    def __init__(self, front, **kw):
        super().__init__(front=front, **kw)

    def utterance(self, u):
        out = dict(pitch=self._rows(u, self.pitch), grp=self._rows(u, self.grp), pratio=self._rows(u, self.pratio),
                   status=int(self.status[u]))
        if self.stages is not None:
            block = self._rows(u, self.stages, self.STAGE_WORDS)
            n = len(out["pitch"])
            for k, name in enumerate(HW25_PITCH_STAGES):
                out[name] = block[k * n:(k + 1) * n].copy()
            grp = block[5 * n:].view(np.float32).reshape(2, n, self.NCHAN)
            for k, name in enumerate(HW25_GRP_STAGES):
                out[name] = grp[k].copy()
        return out


def _bank_pitch(bank, front_result, result, batch, stages, use_order):
    """the one body of the pitch wrappers of both banks: the front half with its ACF, then the bank's pitch call"""
    torch = _torch()
    lib = _lib.load()
    front = _bank_front(bank, front_result, batch, True, use_order)
    dev = front.pitch.device
    n = front.pitch.shape[0]
    pitch = torch.zeros(n, dtype=torch.int32, device=dev)
    grp = torch.zeros((n, bank.nchan), dtype=torch.float32, device=dev)
    pratio = torch.zeros_like(grp)
    status = torch.zeros(max(batch.n_utt, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n * result.STAGE_WORDS, dtype=torch.int32, device=dev) if stages else None
    nbytes = int(getattr(lib, f"sea_{bank.name}_pitch_scratch_bytes")(n, int(batch.n_utt)))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    fn = f"sea_{bank.name}_pitch_batch"
    rc = getattr(lib, fn)(_dptr(front.acf_hc), *([_dptr(front.cross_hc)] if bank.pitch_reads_cross else []), _dptr(front.pratio),
                          _dptr(front.mark), _dptr(batch.lengths), _dptr(front.row_offsets), _dptr(pitch), _dptr(grp), _dptr(pratio),
                          _dptr(status), _dptr(st), _dptr(scratch), _hw25_order(batch, use_order), batch.n_utt, _stream_ptr())
    _lib.check(rc, fn)
    return result(front, pitch=pitch, grp=grp, pratio=pratio, status=status, stages=st)


def hw25_pitch_batch(batch, stages=False, use_order=True):
    """createIBM():41-87 for every utterance of the batch: the front half with its ACF output, then initGroup and pitchDtm, one
    launch group on the current stream -> Hw25PitchResult.  stages: also keep Pitch / Grp after every step of pitchDtm."""
    return _bank_pitch(_BANK25, Hw25Result, Hw25PitchResult, batch, stages, use_order)


def hw25_pitch(x):
    """One utterance from host memory (float32 or int16 samples on the int16 scale) -> dict: pitch int32 [F], grp and pratio
    [F][25], status."""
    return _hw25_host("sea_hw25_pitch", x, ("pitch", "grp", "pratio"))


# ------------------------------------------------------------------------------------------------
# the estimator's AM labels, final grouping and the whole of createIBM (HuWang.cpp:89-106: computeAM, finalSeg, the
# binarisation; csrc/hw25_am_kernel.hip)
# ------------------------------------------------------------------------------------------------
HW25_FINAL_STAGES = ("final_reseg1", "final_reseg2", "final_reseg3", "final_dev_minus", "final_dev_plus")
HW25_FINAL_TOO_MANY_SEGMENTS, HW25_AM_TOO_LONG, HW25_AM_BAD_PITCH = 1 << 18, 1 << 19, 1 << 20


def hw25_am_tables():
    """The AM stage's host constants: a, beta (kaiserPara (0.01, ..)), n_at_pow2 int32 [11] (computeAM's N at L = 2^7 .. 2^17)
    and twiddles float32 [2^18 - 1][2] (fft's u values, period p's p entries from entry p - 1)."""
    lib = _lib.load()
    ab, n, tw = np.zeros(2, np.float32), np.zeros(11, np.int32), np.zeros(((1 << 18) - 1, 2), np.float32)
    _lib.check(lib.sea_hw25_am_tables_host(_np_ptr(ab), _np_ptr(n), _np_ptr(tw), tw.shape[0]), "sea_hw25_am_tables_host")
    return dict(a=ab[0], beta=ab[1], n_at_pow2=n, twiddles=tw)


def hw25_periphery_gout_batch(batch, use_order=True):
    """hw25_periphery_batch() with gOut, the gammatone output before the hair cell: (hOut, hEv, gOut), the same layout."""
    return _hw25_periphery(batch, use_order, True)


class Hw25AmResult(_Hw25Rows):
    """What hw25_am_batch() computed, device tensors: amcrn [rows][25] 0 / 1, status int32 [n_utt] (HW25_AM_TOO_LONG,
    HW25_AM_BAD_PITCH) and, when asked for, ratio and seng [rows][25], ampatt and am (gOut's layout).  utterance(u): numpy."""

    def __init__(self, batch, **kw):
        super().__init__(batch=batch, **kw)

    def utterance(self, u):
        out = dict(amcrn=self._rows(u, self.amcrn), status=int(self.status[u]))
        for k in ("ratio", "seng"):
            if getattr(self, k) is not None:
                out[k] = self._rows(u, getattr(self, k))
        for k in ("ampatt", "am"):
            if getattr(self, k) is not None:
                out[k] = self._block(u, getattr(self, k)).copy()
        return out


def _bank_am(bank, result, batch, gout, pitch, row_offsets, want_details, use_order):
    """the one body of the AM wrappers of both banks"""
    torch = _torch()
    lib = _lib.load()
    s = _hw25_start(batch, dev=gout.device, row_offsets=row_offsets, zeros=("status",), bank=bank)
    amcrn = torch.zeros((s.n, bank.nchan), dtype=torch.float32, device=s.dev)
    ratio, seng = (torch.zeros_like(amcrn) for _ in range(2)) if want_details else (None, None)
    ampatt, am = (torch.zeros_like(gout) for _ in range(2)) if want_details else (None, None)
    nbytes = int(getattr(lib, f"sea_{bank.name}_am_scratch_bytes")(s.total, int(batch.n_utt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=s.dev)
    fn = f"sea_{bank.name}_am_batch"
    rc = getattr(lib, fn)(_dptr(gout), _dptr(pitch), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(s.d_offs), _dptr(amcrn),
                          _dptr(ratio), _dptr(seng), _dptr(ampatt), _dptr(am), _dptr(s.status), _dptr(scratch), s.total,
                          _hw25_order(batch, use_order), batch.n_utt, _stream_ptr())
    _lib.check(rc, fn)
    return result(batch, amcrn=amcrn, ratio=ratio, seng=seng, ampatt=ampatt, am=am, status=s.status, row_offsets=s.d_offs,
                  host_row_offsets=s.offs, host_rows=s.rows)


def hw25_am_batch(batch, gout, pitch, row_offsets=None, want_details=False, use_order=True):
    """computeAM for every utterance of the batch from hw25_periphery_gout_batch()'s gOut and hw25_pitch_batch()'s pitch (int32
    [rows] on the device; row_offsets: the int64 device tensor that goes with it) -> Hw25AmResult.  want_details: also ratio,
    seng, ampatt and am."""
    return _bank_am(_BANK25, Hw25AmResult, batch, gout, pitch, row_offsets, want_details, use_order)


class Hw25MaskResult(_Hw25Rows):
    """What hw25_finalseg_batch() / hw25_ibm_batch() computed, device tensors: mask [rows][25] 0 / 1, status int32 [n_utt],
    grp_final [rows][25] or None, pitch int32 [rows] or None, stages (floats, or None).  utterance(u): numpy arrays, the stage
    arrays under HW25_FINAL_STAGES when they were asked for."""

    def utterance(self, u):
        out = dict(mask=self._rows(u, self.mask), status=int(self.status[u]))
        for k in ("grp_final", "pitch"):
            if getattr(self, k, None) is not None:
                out[k] = self._rows(u, getattr(self, k))
        if self.stages is not None:
            w = len(HW25_FINAL_STAGES) * self.NCHAN
            block = self._rows(u, self.stages, w).reshape(len(HW25_FINAL_STAGES), len(out["mask"]), self.NCHAN)
            for k, name in enumerate(HW25_FINAL_STAGES):
                out[name] = block[k].copy()
        return out


def _bank_finalseg(bank, result, grp, amcrn, cross_ev, pratio, lengths, row_offsets, host_rows, stages, use_order):
    """the one body of the final-grouping wrappers of both banks"""
    torch = _torch()
    lib = _lib.load()
    dev = grp.device
    host_rows = np.asarray(host_rows, dtype=np.int64)
    n_utt, n = len(host_rows), max(int(host_rows.sum()), 1)
    mask = torch.zeros((n, bank.nchan), dtype=torch.float32, device=dev)
    grp_final = torch.zeros_like(mask)
    status = torch.zeros(max(n_utt, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n * len(HW25_FINAL_STAGES) * bank.nchan, dtype=torch.float32, device=dev) if stages else None
    nbytes = int(getattr(lib, f"sea_{bank.name}_finalseg_scratch_bytes")(n, n_utt))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fn = f"sea_{bank.name}_finalseg_batch"
    rc = getattr(lib, fn)(_dptr(grp), _dptr(amcrn), _dptr(cross_ev), _dptr(pratio), _dptr(lengths), _dptr(row_offsets), _dptr(mask),
                          _dptr(grp_final), _dptr(status), _dptr(st), _dptr(scratch), _dptr(use_order), n_utt, _stream_ptr())
    _lib.check(rc, fn)
    return result(mask=mask, grp_final=grp_final, status=status, stages=st, pitch=None, host_row_offsets=_row_offsets(host_rows),
                  host_rows=host_rows)


def hw25_finalseg_batch(grp, amcrn, cross_ev, pratio, lengths, row_offsets, host_rows, stages=False, use_order=None):
    """finalSeg and the binarisation on device tensors [rows][25] (hw25_pitch_batch()'s grp and pratio, hw25_am_batch()'s amcrn,
    the front half's cross_ev), lengths / row_offsets int64 [n_utt] on the device, host_rows the row counts -> Hw25MaskResult.
    use_order: an int32 device tensor (launch order) or None."""
    return _bank_finalseg(_BANK25, Hw25MaskResult, grp, amcrn, cross_ev, pratio, lengths, row_offsets, host_rows, stages, use_order)


class Hw25EnhanceResult(Hw25MaskResult):
    """What hw25_enhance_batch() computed, device tensors: audio float32, packed like the batch's data (batch.split cuts it),
    with mask [rows][25], pitch int32 [rows] and status int32 [n_utt] as hw25_ibm_batch() gives them.  utterance(u): numpy."""

    def utterance(self, u):
        out = super().utterance(u)
        off, L = int(self.batch.host_offsets[u]), int(self.batch.host_lengths[u])
        out["audio"] = self.audio[off:off + L].cpu().numpy()
        return out


def _bank_ibm(bank, result, batch, stages, use_order, enhance=False):
    """the one body of the whole-estimator wrappers of both banks and of hw25_enhance_batch, which resynthesises the mask in
    the same launch group"""
    torch = _torch()
    lib = _lib.load()
    s = _hw25_start(batch, zeros=("mask", "pitch", "status"), bank=bank)
    st = torch.zeros(s.n * len(HW25_FINAL_STAGES) * bank.nchan, dtype=torch.float32, device=s.dev) if stages else None
    nbytes = int(getattr(lib, f"sea_{bank.name}_ibm_scratch_bytes")(s.total, s.n, int(batch.n_utt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=s.dev)
    head = (_dptr(s.x), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(s.d_offs))
    outs = (_dptr(s.mask), _dptr(s.pitch), _dptr(s.status))
    tail = (_dptr(scratch), s.total, s.n, _hw25_order(batch, use_order), batch.n_utt, _stream_ptr())
    res = dict(mask=s.mask, grp_final=None, status=s.status, stages=st, pitch=s.pitch, host_row_offsets=s.offs, host_rows=s.rows)
    if not enhance:
        fn = f"sea_{bank.name}_ibm_batch"
        _lib.check(getattr(lib, fn)(*head, *outs, _dptr(st), *tail), fn)
        return result(**res)
    audio = torch.zeros(s.total, dtype=torch.float32, device=s.dev)
    _lib.check(lib.sea_hw25_enhance_batch(*head, _dptr(audio), None, *outs, *tail), "sea_hw25_enhance_batch")
    return Hw25EnhanceResult(batch=batch, audio=audio, **res)


def hw25_ibm_batch(batch, stages=False, use_order=True):
    """createIBM() for every utterance of the batch, one launch group on the current stream -> Hw25MaskResult with the binary
    mask [rows][25], pitchDtm's pitch [rows] and the status (hw25_pitch_batch()'s with HW25_FINAL_TOO_MANY_SEGMENTS,
    HW25_AM_TOO_LONG).  stages: also keep Grp after each of finalSeg's five steps."""
    return _bank_ibm(_BANK25, Hw25MaskResult, batch, stages, use_order)


def hw25_ibm(x):
    """createIBM (x) for one utterance from host memory (float32 or int16 samples on the int16 scale) -> dict: mask [F][25]
    floats 0 / 1, pitch int32 [F], status."""
    return _hw25_host("sea_hw25_ibm", x, ("mask", "pitch"))


# ------------------------------------------------------------------------------------------------
# the estimator's resynthesis (HuWang.cpp:1498-1549; csrc/hw25_resynth_kernel.hip): the mask applied, audio out
# ------------------------------------------------------------------------------------------------
def hw25_resynth_tables():
    """The overlap-add tables of resynthesis(): up float64 [80], down float64 [120] and w float32 [80][8], the weight at
    position o of a hop for the eight states (bit 0 / 1 / 2: frame k - 1 / k / k + 1 exists and is set)."""
    lib = _lib.load()
    w, up, down = np.zeros((80, 8), np.float32), np.zeros(80, np.float64), np.zeros(120, np.float64)
    _lib.check(lib.sea_hw25_resynth_tables_host(_np_ptr(w), _np_ptr(up), _np_ptr(down)), "sea_hw25_resynth_tables_host")
    return dict(w=w, up=up, down=down)


def hw25_resynth_batch(batch, gout, mask, row_offsets=None, threshold=0.0, int16=False, use_order=True):
    """resynthesis() for every utterance of the batch from hw25_periphery_gout_batch()'s gOut and a mask [rows][25] on the
    device (a unit is set where mask > threshold; row_offsets: the int64 device tensor that goes with it, else length // 80 rows
    per utterance one after the other) -> float32 audio packed like batch.data (batch.split cuts it); int16=True: (audio, the
    int16 conversion of it)."""
    torch = _torch()
    lib = _lib.load()
    s = _hw25_start(batch, dev=gout.device, row_offsets=row_offsets)
    mask = mask.to(torch.float32).contiguous()
    out = torch.zeros(batch.total, dtype=torch.float32, device=s.dev)
    out16 = torch.zeros(batch.total, dtype=torch.int16, device=s.dev) if int16 else None
    rc = lib.sea_hw25_resynth_batch(_dptr(gout), _dptr(mask), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(s.d_offs),
                                    float(threshold), _dptr(out), _dptr(out16), _hw25_order(batch, use_order), batch.n_utt,
                                    _stream_ptr())
    _lib.check(rc, "sea_hw25_resynth_batch")
    return (out, out16) if int16 else out


def hw25_resynth(x, mask, threshold=0.0):
    """One utterance from host memory (float32 or int16 samples on the int16 scale) and its mask [len(x) // 80][25] -> the
    resynthesised float32 audio [len(x)]."""
    mask = np.ascontiguousarray(mask, dtype=np.float32).reshape(-1, HW25_NCHAN)
    return _hw25_host("sea_hw25_resynth", x, ("audio",), _np_ptr(mask), mask.shape[0], float(threshold), status=False)["audio"]


def hw25_enhance_batch(batch, use_order=True):
    """createIBM() followed by resynthesis() of its own mask for every utterance of the batch, one launch group on the
    current stream -> Hw25EnhanceResult."""
    return _bank_ibm(_BANK25, Hw25MaskResult, batch, False, use_order, enhance=True)


def hw25_enhance(x):
    """One utterance from host memory (float32 or int16 samples on the int16 scale) -> dict: audio float32 [L], the enhanced
    signal; mask [F][25] floats 0 / 1, pitch int32 [F], status, as hw25_ibm() gives them."""
    return _hw25_host("sea_hw25_enhance", x, ("audio", "mask", "pitch"))
