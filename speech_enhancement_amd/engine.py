"""Host-side mirror of the reference's interface for the hot path, over libsea_mi355x.so.

Names follow the reference:
  etsi_denoise(x)              etsi/cpp/AdvFrontEnd.c:125       (host arrays, the C drop-in itself)
  rfft(x)                      etsi/cpp/rfft.c:45
  DoCompCeps(data201)          etsi/cpp/CompCeps.c:309
  NoiseSup                     DoNoiseSupAlloc/Init/DoNoiseSup/Delete (etsi/cpp/NoiseSup.c:859-1440)
  resynth(x, mask, binary)     resyth_64sub_{ori,IBM}/cpp/extractwav.cpp:9
and the batched, HBM-resident forms the GPU wants (PackedBatch + *_batch).

torch is used for device memory and streams only (plumbing); all compute is in the HIP library.
"""
import ctypes

import numpy as np

from . import _lib


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------
# drop-ins on host arrays (these call the C symbols with the reference's own signatures)
# ------------------------------------------------------------------------------------------------
def etsi_denoise(x, fill=0):
    """int etsi_denoise(short*, short*, long).  Samples beyond the last full 80-sample frame are
    not written (they keep ``fill``), exactly like the reference."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.int16)
    out = np.full(x.shape, fill, dtype=np.int16)
    rc = lib.etsi_denoise(_np_ptr(x), _np_ptr(out), x.size)
    _lib.check(rc, "etsi_denoise")
    return out


def rfft(x, m=None):
    """void rfft(float*, n, m) (etsi/cpp/rfft.h:19): returns Re(0..n/2), Im(n/2-1..1); m defaults to log2 n."""
    lib = _lib.load()
    y = np.array(x, dtype=np.float32, copy=True)
    n = int(y.size)
    if n < 2 or n & (n - 1):
        raise ValueError("rfft: n must be a power of two")
    lib.rfft(_np_ptr(y), n, int(m) if m is not None else n.bit_length() - 1)
    return y


def DoCompCeps(data201):
    """DoCompCeps(Data, Coef, This) with data201[0] = Data[-1]; returns c1..c12, c0, logE."""
    lib = _lib.load()
    d = np.ascontiguousarray(data201, dtype=np.float32)
    if d.size != 201:
        raise ValueError("DoCompCeps needs Data[-1..199] (201 floats)")
    coef = np.zeros(14, np.float32)
    ptr = ctypes.c_void_p(d.ctypes.data + 4)
    _lib.check(lib.sea_compceps_frame(ptr, _np_ptr(coef)), "DoCompCeps")
    return coef


def resynth(x, mask, binary=False, frames_l_over_160=False):
    """resynth(): x int16[L], mask float32[F][64] with F=(L-320)/160+1 (or L/160 with
    frames_l_over_160, the frame count of 1dnn_resynth/extractwav.cpp:67) -> int16[L]."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.int16)
    mask = np.ascontiguousarray(mask, dtype=np.float32)
    out = np.zeros(x.size, np.int16)
    mode = int(bool(binary)) | (2 if frames_l_over_160 else 0)
    rc = lib.sea_resynth64(_np_ptr(x), x.size, _np_ptr(mask), int(mask.shape[0]), mode, _np_ptr(out))
    _lib.check(rc, "resynth")
    return out


def subbband(x):
    """subbband(): x int16[L] -> int16[64][L] (gammatone + hair cell per channel)."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.int16)
    out = np.zeros((64, x.size), np.int16)
    _lib.check(lib.sea_subband64(_np_ptr(x), x.size, _np_ptr(out)), "subbband")
    return out


def irm_target(pure64, noise64, window=1):
    """make_single_IBM's IRM target (enhancement_extract_test/cpp/show_IBM.cpp:105-169) from the [64][L] int16
    subband blocks of the clean and the noise signal (two subbband() outputs) -> float32 [F][64], the mask matrix
    resynth() takes.  window: 0 rectangular, 1 Hamming, 2 Hanning (asdk::SpecInfo's is unknown: parity unpinned)."""
    lib = _lib.load()
    pure64 = np.ascontiguousarray(pure64, dtype=np.int16)
    noise64 = np.ascontiguousarray(noise64, dtype=np.int16)
    if pure64.shape != noise64.shape or pure64.ndim != 2 or pure64.shape[0] != 64:
        raise ValueError("irm_target needs two [64][L] int16 blocks")
    L = pure64.shape[1]
    out = np.zeros((max((L - 320) // 160 + 1, 1), 64), np.float32)
    _lib.check(lib.sea_irm_target(_np_ptr(pure64), _np_ptr(noise64), L, int(window), _np_ptr(out)), "irm_target")
    return out


def gammaToneFilter(x, chan):
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros_like(x)
    _lib.check(lib.sea_gammatone_filter(_np_ptr(x), _np_ptr(y), int(chan), x.size), "gammaToneFilter")
    return y


class NoiseSup:
    """The FEParamsX NoiseSup slot (DoNoiseSupAlloc / Init / DoNoiseSup / Delete) on the GPU: one
    stream whose recursive state stays in HBM between 80-sample pushes."""

    def __init__(self):
        self._lib = _lib.load()
        self._h = self._lib.sea_ns_stream_alloc()
        if not self._h:
            raise _lib.SeaError("DoNoiseSupAlloc failed: " + self._lib.sea_last_error().decode())
        self._lib.sea_ns_stream_init(self._h)

    def init(self):
        self._lib.sea_ns_stream_init(self._h)

    def DoNoiseSup(self, in80):
        x = np.ascontiguousarray(in80, dtype=np.float32)
        assert x.size == 80
        out = np.zeros(80, np.float32)
        produced = self._lib.sea_ns_stream_push(self._h, _np_ptr(x), _np_ptr(out))
        return bool(produced), out

    def close(self):
        if self._h:
            self._lib.sea_ns_stream_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tables():
    """The constant tables the library computed (for tests against the oracle's)."""
    lib = _lib.load()
    t = dict(sigWindow=np.zeros(200, np.float32), irWindow=np.zeros(17, np.float32),
             idct=np.zeros((25, 25), np.float32), melStart=np.zeros(25, np.int32),
             melLen=np.zeros(25, np.int32), melData=np.zeros((25, 16), np.float32),
             hamming=np.zeros(100, np.float32), dct=np.zeros((12, 23), np.float32),
             ccStart=np.zeros(23, np.int32), ccLen=np.zeros(23, np.int32),
             ccData=np.zeros((23, 32), np.float32))
    keys = ("sigWindow", "irWindow", "idct", "melStart", "melLen", "melData", "hamming", "dct",
            "ccStart", "ccLen", "ccData")
    _lib.check(lib.sea_tables_host(*[_np_ptr(t[k]) for k in keys]), "sea_tables_host")
    cf, bw, me = (np.zeros(64, np.float32) for _ in range(3))
    _lib.check(lib.sea_gammatone_channels(_np_ptr(cf), _np_ptr(bw), _np_ptr(me)), "sea_gammatone_channels")
    t.update(cf=cf, bw=bw, midEar=me)
    return t


# ------------------------------------------------------------------------------------------------
# batched, HBM-resident forms
# ------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _stream_ptr():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# the six-wave NoiseSup kernels keep frame indices in 32 bits and would silently cut a longer utterance (ns_pipe6_kernel.hip,
# kMaxFrames); 2^31 frames are 172 G samples, more than the device's memory holds in and out
MAX_FRAMES_PER_UTTERANCE = 2 ** 31 - 17


def _row_offsets(rows, total=False):
    """Row counts per utterance -> the int64 host array of where each one's rows begin when they lie one after the other (the
    exclusive prefix sum; nothing in, nothing out).  total=True: one more entry, the sum."""
    starts = np.concatenate((np.zeros(1, np.int64), np.cumsum(np.asarray(rows, dtype=np.int64))))
    return starts if total else starts[:-1]


def launch_order(lengths, n_cu=256):
    """Launch order of the utterance-per-workgroup kernels: longest first (the dispatcher serves the
    oldest waves first, so the critical path -- the longest utterance -- starts at once and keeps
    priority), in rows of n_cu workgroups with every other row reversed.  Workgroups b, b+n_cu,
    b+2 n_cu, ... of a launch share a CU (tools/hwid_probe.hip), so the serpentine gives each CU a
    long, a short, a medium-long and a medium-short utterance instead of the four longest of their
    rows (measured on the bench corpus: 3.78 -> 3.67 ms, tools/order_sweep.py)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    order = np.argsort(-lengths, kind="stable").astype(np.int32)
    for k, start in enumerate(range(0, len(order), n_cu)):
        if k & 1:
            order[start:start + n_cu] = order[start:start + n_cu][::-1].copy()
    return order


class PackedBatch:
    """A batch of utterances packed back to back in one int16 tensor resident in HBM.

    data     int16 [total]     utterance u at data[offsets[u] : offsets[u]+lengths[u]]
    offsets  int64 [n]         multiples of 8 samples (16-byte aligned rows)
    lengths  int64 [n]
    order    int32 [n]         launch order (see launch_order)
    """

    def __init__(self, data, offsets, lengths, order, host_offsets, host_lengths):
        self.data, self.offsets, self.lengths, self.order = data, offsets, lengths, order
        self.host_offsets, self.host_lengths = host_offsets, host_lengths

    @property
    def n_utt(self):
        return len(self.host_lengths)

    @property
    def total(self):
        return int(self.data.numel())

    @property
    def n_frames(self):
        """NoiseSup frames (80 samples) in the batch."""
        return int(self.frame_rows()[0].sum())

    def frame_rows(self, hop=80):
        """(rows, offsets), host int64 arrays: every utterance's whole frames of ``hop`` samples, and its first row where
        the rows of the batch lie one after the other."""
        rows = np.asarray(self.host_lengths, dtype=np.int64) // hop
        return rows, _row_offsets(rows)

    @staticmethod
    def layout(lengths):
        lengths = np.asarray(lengths, dtype=np.int64)
        if len(lengths) and int(lengths.max()) // 80 >= MAX_FRAMES_PER_UTTERANCE:
            raise ValueError(f"an utterance of {int(lengths.max())} samples has {MAX_FRAMES_PER_UTTERANCE} frames or more: "
                             "the NoiseSup kernels count frames in 32 bits")
        padded = (lengths + 7) // 8 * 8
        offsets = _row_offsets(padded)
        total = int(padded.sum())
        return offsets, total, launch_order(lengths)

    @classmethod
    def from_arrays(cls, utterances, device="cuda", dtype=np.int16):
        """dtype: int16 audio everywhere; float32 only for the hw25_* calls, which take float samples on the int16 scale."""
        torch = _torch()
        lengths = np.array([len(u) for u in utterances], dtype=np.int64)
        offsets, total, order = cls.layout(lengths)
        host = np.zeros(max(total, 8), dtype)
        for u, off in zip(utterances, offsets):
            host[off:off + len(u)] = u
        return cls(torch.from_numpy(host).to(device), torch.from_numpy(offsets).to(device),
                   torch.from_numpy(lengths).to(device), torch.from_numpy(order).to(device), offsets, lengths)

    def like(self, fill=0, dtype=None):
        torch = _torch()
        return torch.full_like(self.data, fill, dtype=dtype or self.data.dtype)

    def split(self, tensor, full_frames_only=False, hop=80):
        """Cut a packed result tensor back into per-utterance numpy arrays."""
        host = tensor.detach().cpu().numpy()
        out = []
        for off, L in zip(self.host_offsets, self.host_lengths):
            n = int(L) // hop * hop if full_frames_only else int(L)
            out.append(host[off:off + n].copy())
        return out


def ns_denoise_batch(batch, out=None, want_f32=False, use_order=True):
    """etsi_denoise semantics for every utterance of the batch, one launch.  Returns
    (out_int16, out_f32 or None, first_out int32[n]).  Asynchronous on the current stream."""
    torch = _torch()
    lib = _lib.load()
    if out is None:
        out = torch.zeros_like(batch.data)
    f32 = torch.zeros(batch.total, dtype=torch.float32, device=batch.data.device) if want_f32 else None
    first = torch.full((batch.n_utt,), -1, dtype=torch.int32, device=batch.data.device)
    rc = lib.sea_ns_denoise_batch(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets),
                                  _dptr(batch.lengths), _dptr(batch.order) if use_order else None,
                                  _dptr(first), batch.n_utt, _stream_ptr())
    _lib.check(rc, "sea_ns_denoise_batch")
    return out, f32, first


def wb_denoise_batch(batch, want_f32=False, want_hb=False, use_order=True):
    """The ETSI wideband (16 kHz) mode for every utterance of the batch (frames of 160 samples): QMF split, NoiseSup on
    the low band and (want_hb) the high band's features per output frame.  Everything returned is at the 8 kHz rate and
    indexed by HALF the batch's offsets (frame f of utterance u at offsets[u] / 2 + 80 f; ``wb_split`` cuts it up); the
    per-frame rows are indexed by ceil(offsets[u] / 160) + f (``wb_rows``).  Returns a dict: out (int16 low band), f32
    (float low band or None), first_out / onset (int32 [n], in frames of 160), hp_rows [rows, 3] / code_rows [rows, 9] (or
    None), qmf_lp / qmf_hp (the float QMF streams, views of the scratch buffer).  Asynchronous on the current stream."""
    torch = _torch()
    lib = _lib.load()
    dev = batch.data.device
    half = (batch.total // 2 + 7) // 8 * 8
    out = torch.zeros(half, dtype=torch.int16, device=dev)
    f32 = torch.zeros(half, dtype=torch.float32, device=dev) if want_f32 else None
    first = torch.full((batch.n_utt,), -1, dtype=torch.int32, device=dev)
    onset = torch.zeros(batch.n_utt, dtype=torch.int32, device=dev)
    rows = int(lib.sea_wb_rows(batch.total))
    hp_rows = torch.zeros((rows, 3), dtype=torch.float32, device=dev) if want_hb else None
    code_rows = torch.zeros((rows, 9), dtype=torch.float32, device=dev) if want_hb else None
    nbytes = int(lib.sea_wb_scratch_bytes(batch.total, batch.n_utt))
    assert nbytes >= 2 * half * 4
    scratch = torch.zeros(nbytes // 4 + 4, dtype=torch.float32, device=dev)
    rc = lib.sea_wb_denoise_batch(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets), _dptr(batch.lengths),
                                  _dptr(batch.order) if use_order else None, _dptr(first), _dptr(onset), _dptr(hp_rows),
                                  _dptr(code_rows), _dptr(scratch), batch.total, batch.n_utt, _stream_ptr())
    _lib.check(rc, "sea_wb_denoise_batch")
    return dict(out=out, f32=f32, first_out=first, onset=onset, hp_rows=hp_rows, code_rows=code_rows,
                qmf_lp=scratch[:half], qmf_hp=scratch[half:2 * half])


def wb_slice_state(n_utt, device="cuda"):
    """The per-utterance state wb_denoise_batch_slice carries from slice to slice: float32 [n_utt, floats per utterance].
    Its contents do not matter before the first slice (resume = 0 reads none of it)."""
    return _torch().zeros((n_utt, int(_lib.load().sea_wb_slice_state_floats())), dtype=_torch().float32, device=device)


def wb_afe_slice_state(n_utt, device="cuda"):
    """The per-utterance state wb_afe_features_batch_slice carries from slice to slice, separate from ``wb_slice_state``:
    float32 [n_utt, floats per utterance].  Its contents do not matter before the first slice."""
    return _torch().zeros((n_utt, int(_lib.load().sea_wb_afe_slice_state_floats())), dtype=_torch().float32, device=device)


def wb_denoise_batch_slice(batch, state, frame_base, resume, want_f32=False, want_hb=False, first_out=None, onset=None,
                           use_order=True, want_flags=False):
    """One TIME SLICE of a wideband batch (sea_wb_denoise_batch_slice): ``batch`` packs THIS slice's samples of every utterance
    that has some (utterance u of every slice is the same utterance; every slice of an utterance is a multiple of 160 samples
    except its last), ``state`` is a ``wb_slice_state`` tensor with a row per utterance, ``frame_base`` the frames of 160
    samples before this slice, ``resume`` false for the first slice.  Returns wb_denoise_batch's dict for the slice, indexed by
    the slice's own offsets; first_out / onset are ABSOLUTE frame indices -- pass the previous slice's tensors back in as
    ``first_out`` / ``onset`` and utterances that have ended keep theirs.  Rows and f32 of frames without an output stay zero.
    Concatenated over the slices, everything is bit for bit wb_denoise_batch's.  Asynchronous on the current stream.

    ``want_flags`` runs sea_wb_denoise_batch_slice_fd instead (f32 and the rows come with it): the dict also holds flag_rows,
    one speech-flag byte per per-frame row of the slice (zero for frames without an output) -- the input of
    ``wb_afe_features_batch_slice``."""
    torch = _torch()
    lib = _lib.load()
    dev = batch.data.device
    n = batch.n_utt
    if state is None or state.dtype != torch.float32 or not state.is_contiguous() \
            or state.numel() < n * int(lib.sea_wb_slice_state_floats()):
        raise ValueError("state must be a contiguous float32 tensor of sea_wb_slice_state_floats() floats per utterance")
    if want_flags:
        want_f32 = want_hb = True
    half = (batch.total // 2 + 7) // 8 * 8
    out = torch.zeros(half, dtype=torch.int16, device=dev)
    f32 = torch.zeros(half, dtype=torch.float32, device=dev) if want_f32 else None
    if first_out is None:
        first_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if onset is None:
        onset = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = int(lib.sea_wb_rows(batch.total))
    hp_rows = torch.zeros((rows, 3), dtype=torch.float32, device=dev) if want_hb else None
    code_rows = torch.zeros((rows, 9), dtype=torch.float32, device=dev) if want_hb else None
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(batch.total, n)) // 4 + 4, dtype=torch.float32, device=dev)
    if want_flags:
        flag_rows = torch.zeros(rows, dtype=torch.uint8, device=dev)
        rc = lib.sea_wb_denoise_batch_slice_fd(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets),
                                               _dptr(batch.lengths), _dptr(batch.order) if use_order else None,
                                               _dptr(first_out), _dptr(onset), _dptr(flag_rows), _dptr(hp_rows),
                                               _dptr(code_rows), _dptr(scratch), batch.total, _dptr(state), n, int(frame_base),
                                               1 if resume else 0, _stream_ptr())
        _lib.check(rc, "sea_wb_denoise_batch_slice_fd")
        return dict(out=out, f32=f32, first_out=first_out, onset=onset, hp_rows=hp_rows, code_rows=code_rows,
                    flag_rows=flag_rows, qmf_lp=scratch[:half], qmf_hp=scratch[half:2 * half], state=state)
    rc = lib.sea_wb_denoise_batch_slice(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets), _dptr(batch.lengths),
                                        _dptr(batch.order) if use_order else None, _dptr(first_out), _dptr(onset),
                                        _dptr(hp_rows), _dptr(code_rows), _dptr(scratch), batch.total, _dptr(state), n,
                                        int(frame_base), 1 if resume else 0, _stream_ptr())
    _lib.check(rc, "sea_wb_denoise_batch_slice")
    return dict(out=out, f32=f32, first_out=first_out, onset=onset, hp_rows=hp_rows, code_rows=code_rows,
                qmf_lp=scratch[:half], qmf_hp=scratch[half:2 * half], state=state)


def wb_afe_features_batch_slice(batch, den, afe_state, frame_base, resume, final=None, want_pp=False):
    """The wideband feature chain over one TIME SLICE (sea_wb_afe_features_batch_slice): ``batch`` and ``den`` are the slice's
    batch and the dict ``wb_denoise_batch_slice(.., want_flags=True)`` returned for it, ``afe_state`` a ``wb_afe_slice_state``
    tensor with a row per utterance, ``frame_base`` / ``resume`` as there.  ``final``: per utterance, true where the utterance
    ends with this slice -- DoVADFlush runs after it (a slice may be empty: a stream whose end is learnt late); None flushes
    nothing.  Returns a dict for THIS slice: feats (list of float32 [n_u, 15] host arrays, the frames emitted during the slice),
    n_feat / n_ceps (int32 host arrays), feat_cc / feat_pp (device tensors [frames of the slice, 14], the cepstral frames that
    complete in it; feat_pp None without want_pp), ceps_cum / feat_cum (host prefix sums of the capacities: the slice's frames
    and the slice's frames + 6), feat15 (the device tensor behind feats); rows behind the counts are zero.
    Concatenated over the slices of an utterance, everything is bit for bit wb_afe_features_batch's."""
    return _afe_slice(batch, den, afe_state, frame_base, resume, final, want_pp, True)


def wb_features_utterances(utterances, want_lp=False):
    """A list of 16 kHz int16 utterances in host memory -> the wideband feature frames a recogniser reads
    (sea_wb_features_utterances: wb_denoise_utterances' pipeline with the feature chain run slice by slice on the device).
    Returns a dict: feats (list of float32 [n_u, 15] arrays: c1..c12, c0, logE, VAD flag per emitted frame -- what
    wb_afe_features_batch returns, however the list is cut), out (list of int16 low-band arrays with want_lp, else None),
    slices (launches the list was cut into)."""
    lib = _lib.load()
    xs = [np.ascontiguousarray(x, dtype=np.int16) for x in utterances]
    n = len(xs)
    feats = [np.zeros((x.size // 160 + 6, 15), np.float32) for x in xs]
    outs = [np.zeros(x.size // 160 * 80, np.int16) for x in xs] if want_lp else None
    if n == 0:
        return dict(feats=feats, out=outs, slices=0)
    ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    n_feat = (ctypes.c_int * n)()
    rc = lib.sea_wb_features_utterances(ptrs(xs), ptrs(outs) if want_lp else None, ptrs(feats), n_feat, lens, n)
    _lib.check(rc, "sea_wb_features_utterances")
    return dict(feats=[f[:int(k)] for f, k in zip(feats, n_feat)], out=outs, slices=int(lib.sea_host_last_slices()))


def wb_denoise_utterances(utterances, want_hb=False):
    """A list of 16 kHz int16 utterances in host memory through the wideband mode's copy / compute pipeline
    (sea_wb_denoise_utterances: time slices, uploads, launches and downloads overlapped).  Returns a dict: out (list of int16
    low-band arrays, 80 * (len // 160) samples each), hp_rows / code_rows (lists of float32 [len // 160, 3] / [.., 9], zeros
    for frames without an output; None without want_hb), slices (launches the list was cut into)."""
    lib = _lib.load()
    xs = [np.ascontiguousarray(x, dtype=np.int16) for x in utterances]
    n = len(xs)
    outs = [np.zeros(x.size // 160 * 80, np.int16) for x in xs]
    hps = [np.zeros((x.size // 160, 3), np.float32) for x in xs] if want_hb else None
    codes = [np.zeros((x.size // 160, 9), np.float32) for x in xs] if want_hb else None
    if n == 0:
        return dict(out=outs, hp_rows=hps, code_rows=codes, slices=0)
    ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    rc = lib.sea_wb_denoise_utterances(ptrs(xs), ptrs(outs), ptrs(hps) if want_hb else None, ptrs(codes) if want_hb else None,
                                       lens, n)
    _lib.check(rc, "sea_wb_denoise_utterances")
    return dict(out=outs, hp_rows=hps, code_rows=codes, slices=int(lib.sea_host_last_slices()))


def wb_compceps_batch(batch, res):
    """The wideband CompCeps on a wb_denoise_batch(.., want_f32=True, want_hb=True) result.  Returns (ceps float32
    [total, 14], ceps_cum int64 [n+1] on host, n_ceps int32 [n] tensor)."""
    torch = _torch()
    lib = _lib.load()
    cap = np.maximum(np.asarray(batch.host_lengths) // 160 - 6, 0).astype(np.int64)
    cum = _row_offsets(cap, total=True)
    total = int(cum[-1])
    dev = batch.data.device
    ceps = torch.zeros((max(total, 1), 14), dtype=torch.float32, device=dev)
    n_ceps = torch.zeros(batch.n_utt, dtype=torch.int32, device=dev)
    d_cum = torch.from_numpy(cum).to(dev)
    rc = lib.sea_wb_compceps_batch(_dptr(res["f32"]), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(res["first_out"]),
                                   _dptr(res["hp_rows"]), _dptr(res["code_rows"]), _dptr(d_cum), total, _dptr(ceps),
                                   _dptr(n_ceps), batch.n_utt, _stream_ptr())
    _lib.check(rc, "sea_wb_compceps_batch")
    return ceps, cum, n_ceps


def wb_afe_features_batch(batch, want_intermediates=False, use_order=True):
    """The wideband (16 kHz) mode's full feature chain -- DoAdvProcess with AdvProcessAlloc (16000) as it was before the author
    commented the chain out (etsi/cpp/ParmInterface.c:274-311): QMF split, NoiseSup on the low band, WaveProc -> the 26-band
    CompCeps -> PostProc -> frame-dropping VAD, with FlushAdvProcess at the end.  Mirrors ``afe_features_batch``.

    Returns a dict: feats (list of float32 [n_u, 15] host arrays: c1..c12, c0, logE, VAD flag per emitted frame), out (int16
    low band, as wb_denoise_batch), and with want_intermediates also flag_rows (uint8, one speech-flag byte per per-frame
    row; ``wb_rows`` cuts it up), feat_cc / feat_pp (per cepstral frame, after CompCeps / PostProc), ceps_cum, n_ceps,
    first_out, onset, f32, hp_rows, code_rows."""
    torch = _torch()
    lib = _lib.load()
    dev = batch.data.device
    n = batch.n_utt
    half = (batch.total // 2 + 7) // 8 * 8
    out = torch.zeros(half, dtype=torch.int16, device=dev)
    f32 = torch.zeros(half, dtype=torch.float32, device=dev)
    first = torch.full((n,), -1, dtype=torch.int32, device=dev)
    onset = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = int(lib.sea_wb_rows(batch.total))
    flag_rows = torch.zeros(rows, dtype=torch.uint8, device=dev)
    hp_rows = torch.zeros((rows, 3), dtype=torch.float32, device=dev)
    code_rows = torch.zeros((rows, 9), dtype=torch.float32, device=dev)
    scratch = torch.zeros(int(lib.sea_wb_scratch_bytes(batch.total, n)) // 4 + 4, dtype=torch.float32, device=dev)
    _lib.check(lib.sea_wb_denoise_batch_fd(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets), _dptr(batch.lengths),
                                           _dptr(batch.order) if use_order else None, _dptr(first), _dptr(onset),
                                           _dptr(flag_rows), _dptr(hp_rows), _dptr(code_rows), _dptr(scratch), batch.total, n,
                                           _stream_ptr()), "sea_wb_denoise_batch_fd")
    nfr = np.asarray(batch.host_lengths) // 160
    ccap = np.maximum(nfr - 6, 0).astype(np.int64)
    ccum = _row_offsets(ccap, total=True)
    fcap = (nfr + 6).astype(np.int64)
    fcum = _row_offsets(fcap, total=True)
    tc, tf = int(ccum[-1]), int(fcum[-1])
    feat_cc = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev)
    feat_pp = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev) if want_intermediates else None
    feat15 = torch.zeros((max(tf, 1), 15), dtype=torch.float32, device=dev)
    n_feat = torch.zeros(n, dtype=torch.int32, device=dev)
    n_ceps = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ccum, d_fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
    _lib.check(lib.sea_wb_afe_features_batch(_dptr(f32), _dptr(flag_rows), _dptr(hp_rows), _dptr(code_rows), _dptr(batch.offsets),
                                             _dptr(batch.lengths), _dptr(first), _dptr(onset), _dptr(d_ccum), tc, _dptr(feat_cc),
                                             _dptr(feat_pp), _dptr(d_fcum), _dptr(feat15), _dptr(n_feat), _dptr(n_ceps), n,
                                             _stream_ptr()), "sea_wb_afe_features_batch")
    torch.cuda.synchronize()
    host15, nf = feat15.cpu().numpy(), n_feat.cpu().numpy()
    res = dict(feats=[host15[fcum[u]:fcum[u] + int(nf[u])] for u in range(n)], out=out)
    if want_intermediates:
        res.update(flag_rows=flag_rows, feat_cc=feat_cc, feat_pp=feat_pp, ceps_cum=ccum, n_ceps=n_ceps, first_out=first,
                   onset=onset, f32=f32, hp_rows=hp_rows, code_rows=code_rows)
    return res


def wb_split(batch, tensor):
    """Cut an 8 kHz-rate result of wb_denoise_batch into per-utterance numpy arrays of 80 * (length // 160) samples."""
    host = tensor.detach().cpu().numpy()
    return [host[int(off) // 2:int(off) // 2 + int(L) // 160 * 80].copy()
            for off, L in zip(batch.host_offsets, batch.host_lengths)]


def wb_rows(batch, tensor):
    """Cut a per-frame row result of wb_denoise_batch into per-utterance numpy arrays of length // 160 rows."""
    host = tensor.detach().cpu().numpy()
    return [host[(int(off) + 159) // 160:(int(off) + 159) // 160 + int(L) // 160].copy()
            for off, L in zip(batch.host_offsets, batch.host_lengths)]


def wb_denoise(x):
    """One utterance at 16 kHz from host memory through the wideband mode: int16 low band, 80 * (len // 160) samples."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.int16)
    out = np.zeros(x.size // 160 * 80, np.int16)
    _lib.check(lib.sea_wb_denoise(_np_ptr(x), x.size, _np_ptr(out)), "sea_wb_denoise")
    return out


def wb_tables():
    """The wideband mode's tables as the library computed them (no GPU needed)."""
    lib = _lib.load()
    t = dict(qmfLp=np.zeros(118, np.float32), qmfHp=np.zeros(118, np.float32), hpMelStart=np.zeros(3, np.int32),
             hpMelLen=np.zeros(3, np.int32), hpMelW=np.zeros((3, 64), np.float32), dct=np.zeros((12, 26), np.float32))
    keys = ("qmfLp", "qmfHp", "hpMelStart", "hpMelLen", "hpMelW", "dct")
    _lib.check(lib.sea_wb_tables_host(*[_np_ptr(t[k]) for k in keys]), "sea_wb_tables_host")
    return t


def compceps_batch(batch, den_f32, first_out):
    """CompCeps on the float NoiseSup stream.  Returns (ceps float32 [total,14], ceps_cum int64
    [n+1] on host, n_ceps int32[n] tensor)."""
    torch = _torch()
    lib = _lib.load()
    cap = np.maximum(np.asarray(batch.host_lengths) // 80 - 6, 0).astype(np.int64)
    cum = _row_offsets(cap, total=True)
    total = int(cum[-1])
    dev = batch.data.device
    ceps = torch.zeros((max(total, 1), 14), dtype=torch.float32, device=dev)
    n_ceps = torch.zeros(batch.n_utt, dtype=torch.int32, device=dev)
    d_cum = torch.from_numpy(cum).to(dev)
    rc = lib.sea_compceps_batch(_dptr(den_f32), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(first_out),
                                _dptr(d_cum), total, _dptr(ceps), _dptr(n_ceps), batch.n_utt, _stream_ptr())
    _lib.check(rc, "sea_compceps_batch")
    return ceps, cum, n_ceps


def afe_features_batch(batch, want_intermediates=False):
    """The full ETSI AFE feature chain of the reference's DoAdvProcess as it was before the author
    commented it out (etsi/cpp/ParmInterface.c:274-311): NoiseSup -> WaveProc -> CompCeps ->
    PostProc -> frame-dropping VAD, with FlushAdvProcess at the end.

    Returns a dict: feats (list of float32 [n_u,15] host arrays: c1..c12, c0, logE, VAD flag per
    emitted frame), out (int16 denoised audio tensor, as ns_denoise_batch), and with
    want_intermediates also flags (per output frame speech bits), feat_cc / feat_pp (per cepstral
    frame, after CompCeps / PostProc), ceps_cum, n_ceps, first_out, onset."""
    torch = _torch()
    lib = _lib.load()
    dev = batch.data.device
    n = batch.n_utt
    out = torch.zeros_like(batch.data)
    f32 = torch.zeros(batch.total, dtype=torch.float32, device=dev)
    first = torch.full((n,), -1, dtype=torch.int32, device=dev)
    onset = torch.zeros(n, dtype=torch.int32, device=dev)
    flags = torch.zeros(max(batch.total // 8, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.sea_ns_denoise_batch_fd(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets),
                                           _dptr(batch.lengths), _dptr(batch.order), _dptr(first), _dptr(flags),
                                           _dptr(onset), n, _stream_ptr()), "sea_ns_denoise_batch_fd")
    nfr = np.asarray(batch.host_lengths) // 80
    ccap = np.maximum(nfr - 6, 0).astype(np.int64)
    ccum = _row_offsets(ccap, total=True)
    fcap = (nfr + 6).astype(np.int64)
    fcum = _row_offsets(fcap, total=True)
    tc, tf = int(ccum[-1]), int(fcum[-1])
    feat_cc = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev)
    feat_pp = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev) if want_intermediates else None
    feat15 = torch.zeros((max(tf, 1), 15), dtype=torch.float32, device=dev)
    n_feat = torch.zeros(n, dtype=torch.int32, device=dev)
    n_ceps = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ccum, d_fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
    _lib.check(lib.sea_afe_features_batch(_dptr(f32), _dptr(flags), _dptr(batch.offsets), _dptr(batch.lengths),
                                          _dptr(first), _dptr(onset), _dptr(d_ccum), tc, _dptr(feat_cc),
                                          _dptr(feat_pp) if feat_pp is not None else None, _dptr(d_fcum),
                                          _dptr(feat15), _dptr(n_feat), _dptr(n_ceps), n, _stream_ptr()),
               "sea_afe_features_batch")
    torch.cuda.synchronize()
    host15, nf = feat15.cpu().numpy(), n_feat.cpu().numpy()
    res = dict(feats=[host15[fcum[u]:fcum[u] + int(nf[u])] for u in range(n)], out=out)
    if want_intermediates:
        res.update(flags=flags, feat_cc=feat_cc, feat_pp=feat_pp, ceps_cum=ccum, n_ceps=n_ceps, first_out=first,
                   onset=onset, den_f32=f32)
    return res


def ns_slice_state(n_utt, device="cuda"):
    """The per-utterance state ns_denoise_batch_slice carries from slice to slice: float32 [n_utt, floats per utterance].
    Its contents do not matter before the first slice (resume = 0 reads none of it)."""
    return _torch().zeros((n_utt, int(_lib.load().sea_ns_slice_state_floats())), dtype=_torch().float32, device=device)


def afe_slice_state(n_utt, device="cuda"):
    """The per-utterance state afe_features_batch_slice carries from slice to slice, separate from ``ns_slice_state``:
    float32 [n_utt, floats per utterance].  Its contents do not matter before the first slice."""
    return _torch().zeros((n_utt, int(_lib.load().sea_afe_slice_state_floats())), dtype=_torch().float32, device=device)


def ns_denoise_batch_slice(batch, state, frame_base, resume, want_f32=False, want_flags=False, first_out=None, onset=None,
                           use_order=True):
    """One TIME SLICE of an 8 kHz batch (sea_ns_denoise_batch_slice): ``batch`` packs THIS slice's samples of every utterance
    that has some (utterance u of every slice is the same utterance; every slice of an utterance is a multiple of 80 samples
    except its last), ``state`` is an ``ns_slice_state`` tensor with a row per utterance, ``frame_base`` the frames of 80
    samples before this slice, ``resume`` false for the first slice.  Returns a dict for the slice, indexed by the slice's own
    offsets: out (int16), f32 (float stream or None), first_out (int32 [n], ABSOLUTE frame indices -- pass the previous
    slice's tensor back in as ``first_out`` and utterances that have ended keep theirs), state.  f32 of frames without an
    output stays zero.  Concatenated over the slices, everything is bit for bit ns_denoise_batch's.  Asynchronous on the
    current stream.

    ``want_flags`` runs sea_ns_denoise_batch_slice_fd instead (f32 comes with it): the dict also holds flags, one speech-flag
    byte per frame with an output at [offsets[u]/8 + 10*f], f within the slice (zero elsewhere), and onset (int32 [n],
    absolute; pass it on like first_out) -- the input of ``afe_features_batch_slice``."""
    torch = _torch()
    lib = _lib.load()
    dev = batch.data.device
    n = batch.n_utt
    if state is None or state.dtype != torch.float32 or not state.is_contiguous() \
            or state.numel() < n * int(lib.sea_ns_slice_state_floats()):
        raise ValueError("state must be a contiguous float32 tensor of sea_ns_slice_state_floats() floats per utterance")
    if want_flags:
        want_f32 = True
    out = torch.zeros_like(batch.data)
    f32 = torch.zeros(batch.total, dtype=torch.float32, device=dev) if want_f32 else None
    if first_out is None:
        first_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    order = _dptr(batch.order) if use_order else None
    if want_flags:
        if onset is None:
            onset = torch.zeros(n, dtype=torch.int32, device=dev)
        flags = torch.zeros(max(batch.total // 8, 1), dtype=torch.uint8, device=dev)
        rc = lib.sea_ns_denoise_batch_slice_fd(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets),
                                               _dptr(batch.lengths), order, _dptr(first_out), _dptr(flags), _dptr(onset),
                                               _dptr(state), n, int(frame_base), 1 if resume else 0, _stream_ptr())
        _lib.check(rc, "sea_ns_denoise_batch_slice_fd")
        return dict(out=out, f32=f32, first_out=first_out, onset=onset, flags=flags, state=state)
    rc = lib.sea_ns_denoise_batch_slice(_dptr(batch.data), _dptr(out), _dptr(f32), _dptr(batch.offsets), _dptr(batch.lengths),
                                        order, _dptr(first_out), _dptr(state), n, int(frame_base), 1 if resume else 0,
                                        _stream_ptr())
    _lib.check(rc, "sea_ns_denoise_batch_slice")
    return dict(out=out, f32=f32, first_out=first_out, onset=None, flags=None, state=state)


def _afe_slice(batch, den, afe_state, frame_base, resume, final, want_pp, wb):
    torch = _torch()
    lib = _lib.load()
    n = batch.n_utt
    name = "sea_wb_afe_slice_state_floats" if wb else "sea_afe_slice_state_floats"
    if afe_state is None or afe_state.dtype != torch.float32 or not afe_state.is_contiguous() \
            or afe_state.numel() < n * int(getattr(lib, name)()):
        raise ValueError(f"afe_state must be a contiguous float32 tensor of {name}() floats per utterance")
    dev = batch.data.device
    nfr = np.asarray(batch.host_lengths, dtype=np.int64) // (160 if wb else 80)
    ccum = _row_offsets(nfr, total=True)
    fcum = _row_offsets(nfr + 6, total=True)
    tc, tf = int(ccum[-1]), int(fcum[-1])
    feat_cc = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev)
    feat_pp = torch.zeros((max(tc, 1), 14), dtype=torch.float32, device=dev) if want_pp else None
    feat15 = torch.zeros((max(tf, 1), 15), dtype=torch.float32, device=dev)
    n_feat = torch.zeros(n, dtype=torch.int32, device=dev)
    n_ceps = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ccum, d_fcum = torch.from_numpy(ccum).to(dev), torch.from_numpy(fcum).to(dev)
    d_final = None
    if final is not None:
        d_final = torch.from_numpy(np.asarray(final, dtype=bool).astype(np.uint8)).to(dev)
        if d_final.numel() != n:
            raise ValueError("final must hold one entry per utterance of the slice")
    if wb:
        call, stream = "sea_wb_afe_features_batch_slice", (den["f32"], den["flag_rows"], den["hp_rows"], den["code_rows"])
    else:
        call, stream = "sea_afe_features_batch_slice", (den["f32"], den["flags"])
    rc = getattr(lib, call)(*[_dptr(t) for t in stream], _dptr(batch.offsets), _dptr(batch.lengths), _dptr(den["first_out"]),
                            _dptr(den["onset"]), _dptr(d_final), _dptr(d_ccum), tc, _dptr(feat_cc), _dptr(feat_pp), _dptr(d_fcum),
                            _dptr(feat15), _dptr(n_feat), _dptr(n_ceps), _dptr(afe_state), n, int(frame_base), 1 if resume else 0,
                            _stream_ptr())
    _lib.check(rc, call)
    torch.cuda.synchronize()
    host15, nf, nc = feat15.cpu().numpy(), n_feat.cpu().numpy(), n_ceps.cpu().numpy()
    return dict(feats=[host15[fcum[u]:fcum[u] + int(nf[u])] for u in range(n)], n_feat=nf, n_ceps=nc, feat_cc=feat_cc,
                feat_pp=feat_pp, feat15=feat15, ceps_cum=ccum, feat_cum=fcum, afe_state=afe_state)


def afe_features_batch_slice(batch, den, afe_state, frame_base, resume, final=None, want_pp=False):
    """The 8 kHz feature chain over one TIME SLICE (sea_afe_features_batch_slice): ``batch`` and ``den`` are the slice's batch
    and the dict ``ns_denoise_batch_slice(.., want_flags=True)`` returned for it, ``afe_state`` an ``afe_slice_state`` tensor
    with a row per utterance, ``frame_base`` / ``resume`` as there.  ``final``: per utterance, true where the utterance ends
    with this slice -- DoVADFlush runs after it (a slice may be empty: a stream whose end is learnt late); None flushes nothing.
    Returns a dict for THIS slice: feats (list of float32 [n_u, 15] host arrays, the frames emitted during the slice), n_feat /
    n_ceps (int32 host arrays), feat_cc / feat_pp (device tensors [frames of the slice, 14], the cepstral frames that complete
    in it; feat_pp None without want_pp), ceps_cum / feat_cum (host prefix sums of the capacities: the slice's frames and the
    slice's frames + 6), feat15 (the device tensor behind feats); rows behind the counts are zero.
    Concatenated over the slices of an utterance, everything is bit for bit afe_features_batch's."""
    return _afe_slice(batch, den, afe_state, frame_base, resume, final, want_pp, False)


def features_utterances(utterances, want_out=False):
    """A list of 8 kHz int16 utterances in host memory -> the feature frames a recogniser reads (sea_features_utterances:
    the host pipeline's time slices with the feature chain run slice by slice on the device).  Returns a dict: feats (list of
    float32 [n_u, 15] arrays: c1..c12, c0, logE, VAD flag per emitted frame -- what afe_features_batch returns, however the
    list is cut), out (list of int16 arrays as etsi_denoise writes them with want_out -- the trailing partial frame stays
    zero -- else None), slices (launches the list was cut into)."""
    lib = _lib.load()
    xs = [np.ascontiguousarray(x, dtype=np.int16) for x in utterances]
    n = len(xs)
    feats = [np.zeros((x.size // 80 + 6, 15), np.float32) for x in xs]
    outs = [np.zeros(x.size, np.int16) for x in xs] if want_out else None
    if n == 0:
        return dict(feats=feats, out=outs, slices=0)
    ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    n_feat = (ctypes.c_int * n)()
    rc = lib.sea_features_utterances(ptrs(xs), ptrs(outs) if want_out else None, ptrs(feats), n_feat, lens, n)
    _lib.check(rc, "sea_features_utterances")
    return dict(feats=[f[:int(k)] for f, k in zip(feats, n_feat)], out=outs, slices=int(lib.sea_host_last_slices()))


def cc_slice_state(n_utt, device="cuda"):
    """The per-utterance state compceps_batch_slice carries from slice to slice, separate from ``ns_slice_state``: float32
    [n_utt, floats per utterance].  Its contents do not matter before the first slice."""
    return _torch().zeros((n_utt, int(_lib.load().sea_cc_slice_state_floats())), dtype=_torch().float32, device=device)


def wb_cc_slice_state(n_utt, device="cuda"):
    """The same for wb_compceps_batch_slice, separate from ``wb_slice_state``."""
    return _torch().zeros((n_utt, int(_lib.load().sea_wb_cc_slice_state_floats())), dtype=_torch().float32, device=device)


def _cc_slice(batch, den, cc_state, frame_base, resume, wb):
    torch = _torch()
    lib = _lib.load()
    n = batch.n_utt
    name = "sea_wb_cc_slice_state_floats" if wb else "sea_cc_slice_state_floats"
    if cc_state is None or cc_state.dtype != torch.float32 or not cc_state.is_contiguous() \
            or cc_state.numel() < n * int(getattr(lib, name)()):
        raise ValueError(f"cc_state must be a contiguous float32 tensor of {name}() floats per utterance")
    dev = batch.data.device
    nfr = np.asarray(batch.host_lengths, dtype=np.int64) // (160 if wb else 80)
    cum = _row_offsets(nfr, total=True)
    total = int(cum[-1])
    ceps = torch.zeros((max(total, 1), 14), dtype=torch.float32, device=dev)
    n_ceps = torch.zeros(n, dtype=torch.int32, device=dev)
    d_cum = torch.from_numpy(cum).to(dev)
    if wb:
        rc = lib.sea_wb_compceps_batch_slice(_dptr(den["f32"]), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(den["first_out"]),
                                             _dptr(den["hp_rows"]), _dptr(den["code_rows"]), _dptr(d_cum), total, _dptr(ceps),
                                             _dptr(n_ceps), _dptr(cc_state), n, int(frame_base), 1 if resume else 0, _stream_ptr())
        _lib.check(rc, "sea_wb_compceps_batch_slice")
    else:
        rc = lib.sea_compceps_batch_slice(_dptr(den["f32"]), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(den["first_out"]),
                                          _dptr(d_cum), total, _dptr(ceps), _dptr(n_ceps), _dptr(cc_state), n, int(frame_base),
                                          1 if resume else 0, _stream_ptr())
        _lib.check(rc, "sea_compceps_batch_slice")
    torch.cuda.synchronize()
    host, nc = ceps.cpu().numpy(), n_ceps.cpu().numpy()
    return dict(ceps=[host[cum[u]:cum[u] + int(nc[u])] for u in range(n)], n_ceps=nc, ceps_dev=ceps, ceps_cum=cum,
                cc_state=cc_state)


def compceps_batch_slice(batch, den, cc_state, frame_base, resume):
    """The plain CompCeps over one TIME SLICE (sea_compceps_batch_slice): ``batch`` and ``den`` are the slice's batch and the
    dict ``ns_denoise_batch_slice(.., want_f32=True)`` (or ``want_flags=True``) returned for it, ``cc_state`` a
    ``cc_slice_state`` tensor with a row per utterance, ``frame_base`` / ``resume`` as there.  Returns a dict for THIS slice:
    ceps (list of float32 [n_u, 14] host arrays, the cepstral frames that complete in the slice), n_ceps (int32 host array),
    ceps_dev (the device tensor behind ceps, capacity = the slice's frames per utterance; rows behind the counts are zero),
    ceps_cum (host prefix sums of the capacities).  Concatenated over the slices of an utterance the rows are bit for bit
    compceps_batch's."""
    return _cc_slice(batch, den, cc_state, frame_base, resume, False)


def wb_compceps_batch_slice(batch, den, cc_state, frame_base, resume):
    """The wideband CompCeps over one TIME SLICE (sea_wb_compceps_batch_slice): as ``compceps_batch_slice`` with the dict of
    ``wb_denoise_batch_slice(.., want_f32=True, want_hb=True)`` (or ``want_flags=True``) and a ``wb_cc_slice_state`` tensor.
    Concatenated over the slices of an utterance the rows are bit for bit wb_compceps_batch's."""
    return _cc_slice(batch, den, cc_state, frame_base, resume, True)


def _denoise_ceps_utterances(utterances, want_audio, wb):
    lib = _lib.load()
    hop = 160 if wb else 80
    xs = [np.ascontiguousarray(x, dtype=np.int16) for x in utterances]
    n = len(xs)
    ceps = [np.zeros((max(x.size // hop - 6, 0) or 1, 14), np.float32) for x in xs]
    # the 8 kHz call always writes its audio: out has the input's length, the trailing partial frame stays zero
    outs = [np.zeros(x.size // 160 * 80 if wb else x.size, np.int16) for x in xs] if (want_audio or not wb) else None
    if n == 0:
        return dict(ceps=[], n_ceps=np.zeros(0, np.int32), out=[] if want_audio else None, slices=0)
    ptrs = lambda arrs: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    n_ceps = (ctypes.c_int * n)()
    name = "sea_wb_denoise_ceps_utterances" if wb else "sea_denoise_ceps_utterances"
    rc = getattr(lib, name)(ptrs(xs), ptrs(outs) if outs is not None else None, ptrs(ceps), n_ceps, lens, n)
    _lib.check(rc, name)
    nc = np.array(list(n_ceps), dtype=np.int32)
    return dict(ceps=[c[:int(k)] for c, k in zip(ceps, nc)], n_ceps=nc, out=outs if want_audio else None,
                slices=int(lib.sea_host_last_slices()))


def denoise_ceps_utterances(utterances, want_out=True):
    """A list of 8 kHz int16 utterances in host memory -> denoised audio and the plain cepstra (sea_denoise_ceps_utterances: a
    list the slice plan cuts runs the host pipeline's time slices, a small one one launch each).  Returns a dict: ceps (list of
    float32 [n_u, 14] arrays: c1..c12, c0, logE -- compceps_batch's rows, however the list is cut), n_ceps (int32 array), out
    (list of int16 arrays as etsi_denoise writes them -- the trailing partial frame stays zero -- or None without want_out),
    slices (launches the list was cut into)."""
    return _denoise_ceps_utterances(utterances, want_out, False)


def wb_denoise_ceps_utterances(utterances, want_lp=False):
    """The same for 16 kHz utterances through the wideband mode (sea_wb_denoise_ceps_utterances): ceps are wb_compceps_batch's
    rows, out the int16 low band (80 * (len // 160) samples each) with want_lp, else None."""
    return _denoise_ceps_utterances(utterances, want_lp, True)


def rfft_batch(frames):
    """frames: float32 tensor [n,256] on the GPU -> rfft of every row."""
    torch = _torch()
    lib = _lib.load()
    frames = frames.contiguous()
    out = torch.empty_like(frames)
    _lib.check(lib.sea_rfft256_batch(_dptr(frames), _dptr(out), frames.shape[0], _stream_ptr()), "sea_rfft256_batch")
    return out


def rfft_any_batch(frames, m=None):
    """frames: float32 tensor [k, n] on the GPU -> rfft (x, n, m) of every row, any size the reference's routine takes
    (etsi/cpp/rfft.c:45-180: n a power of two, 2^m <= n; m defaults to log2 n)."""
    lib = _lib.load()
    out = frames.contiguous().clone()
    n = int(out.shape[1])
    if m is None:
        m = n.bit_length() - 1
    _lib.check(lib.sea_rfft_batch(_dptr(out), n, int(m), out.shape[0], _stream_ptr()), "sea_rfft_batch")
    return out


def compceps_frames(frames201):
    """frames201: float32 tensor [n,201] on the GPU -> [n,14]."""
    torch = _torch()
    lib = _lib.load()
    frames201 = frames201.contiguous()
    out = torch.empty((frames201.shape[0], 14), dtype=torch.float32, device=frames201.device)
    _lib.check(lib.sea_compceps_frames(_dptr(frames201), _dptr(out), frames201.shape[0], _stream_ptr()),
               "sea_compceps_frames")
    return out


class MaskBatch:
    """Per-utterance mask matrices [F_u][64] packed row-wise, F_u = (L_u-320)/160+1."""

    def __init__(self, data, row_offsets, host_row_offsets, host_rows):
        self.data, self.row_offsets = data, row_offsets
        self.host_row_offsets, self.host_rows = host_row_offsets, host_rows

    @classmethod
    def from_arrays(cls, masks, device="cuda"):
        torch = _torch()
        rows = np.array([m.shape[0] for m in masks], dtype=np.int64)
        offs = _row_offsets(rows)
        host = np.concatenate([np.ascontiguousarray(m, dtype=np.float32) for m in masks], axis=0)
        return cls(torch.from_numpy(host).to(device), torch.from_numpy(offs).to(device), offs, rows)


def resynth_scratch_elems(batch):
    """float32 elements of the HBM intermediate of resynth_batch (sea_resynth_scratch_bytes / 4)."""
    return int(_lib.load().sea_resynth_scratch_bytes(int(batch.total), int(batch.n_utt))) // 4


def resynth_batch(batch, masks, binary=False, out=None, scratch=None, use_order=True, frames_l_over_160=False):
    """64-band gammatone resynthesis of every utterance of the batch (two launches on the current
    stream).  ``scratch`` (float32, resynth_scratch_elems(batch) elements) may be passed to reuse the HBM-resident
    analysis intermediate between calls."""
    torch = _torch()
    lib = _lib.load()
    if np.any(np.asarray(batch.host_lengths) < (160 if frames_l_over_160 else 320)):
        raise ValueError("resynth needs utterances of at least one mask frame")
    if out is None:
        out = torch.zeros_like(batch.data)
    if scratch is None:
        scratch = torch.empty(resynth_scratch_elems(batch), dtype=torch.float32, device=batch.data.device)
    rc = lib.sea_resynth64_batch(_dptr(batch.data), _dptr(out), _dptr(batch.offsets), _dptr(batch.lengths),
                                 _dptr(masks.data), _dptr(masks.row_offsets), _dptr(scratch),
                                 _dptr(batch.order) if use_order else None, batch.n_utt,
                                 int(bool(binary)) | (2 if frames_l_over_160 else 0), _stream_ptr())
    _lib.check(rc, "sea_resynth64_batch")
    return out, scratch


def subband_batch(batch, out=None, use_order=True):
    """subbband() for every utterance of the batch.  Returns an int16 tensor of 64x the packed
    size: utterance u's [64][pitch] block starts at offsets[u]*64, pitch = length rounded up to 8."""
    torch = _torch()
    lib = _lib.load()
    if out is None:
        out = torch.zeros(batch.total * 64, dtype=torch.int16, device=batch.data.device)
    rc = lib.sea_subband64_batch(_dptr(batch.data), _dptr(out), _dptr(batch.offsets), _dptr(batch.lengths),
                                 _dptr(batch.order) if use_order else None, batch.n_utt, _stream_ptr())
    _lib.check(rc, "sea_subband64_batch")
    return out


def irm_target_batch(batch, pure_sub, noise_sub, window=1):
    """IRM target of every utterance of the batch from two subband_batch() outputs (clean, noise).  Returns a
    MaskBatch (rows (L_u - 320) / 160 + 1 per utterance) that resynth_batch() takes as it is."""
    torch = _torch()
    lib = _lib.load()
    if np.any(np.asarray(batch.host_lengths) < 320):
        raise ValueError("irm_target needs utterances of at least one 320-sample frame")
    rows = (np.asarray(batch.host_lengths) - 320) // 160 + 1
    offs = _row_offsets(rows)
    dev = batch.data.device
    irm = torch.zeros((int(rows.sum()), 64), dtype=torch.float32, device=dev)
    d_offs = torch.from_numpy(offs).to(dev)
    _lib.check(lib.sea_irm_target_batch(_dptr(pure_sub), _dptr(noise_sub), _dptr(batch.offsets), _dptr(batch.lengths),
                                        _dptr(d_offs), _dptr(irm), int(window), batch.n_utt, _stream_ptr()),
               "sea_irm_target_batch")
    return MaskBatch(irm, d_offs, offs, rows)


# ------------------------------------------------------------------------------------------------
# the training-set builder (enhancement_extract_subband_linux/cpp/main.cpp:91-274): mix at an SNR, subbands, IRM target
# ------------------------------------------------------------------------------------------------
def snr_lin(db):
    """addnoise's `float dB = pow (10.0, db / 10.0)` with db an int: the C library's double pow, rounded to float."""
    import math
    db = np.asarray(db)
    if not np.issubdtype(db.dtype, np.integer):
        raise ValueError("addnoise takes whole dB values (the reference's addnoisedB is an int)")
    return np.array([math.pow(10.0, int(v) / 10.0) for v in db.ravel()], dtype=np.float64).astype(np.float32).reshape(db.shape)


def _mix_inputs(batch, noise_src, noise_start, db):
    torch = _torch()
    dev = batch.data.device
    if not (torch.is_tensor(noise_src) and noise_src.dtype == torch.int16 and noise_src.device == dev):
        noise_src = torch.as_tensor(np.ascontiguousarray(noise_src, dtype=np.int16)).to(dev)
    noise_src = noise_src.contiguous()
    start = np.ascontiguousarray(noise_start, dtype=np.int64)
    db = np.ascontiguousarray(db)
    if start.shape != (batch.n_utt,) or db.shape != (batch.n_utt,):
        raise ValueError("one noise start and one dB value per utterance")
    if np.any(start < 0) or np.any(start + np.asarray(batch.host_lengths) > int(noise_src.numel())):
        raise ValueError("a noise stretch does not lie inside noise_src")
    return noise_src, torch.from_numpy(start).to(dev), torch.from_numpy(snr_lin(db)).to(dev)


def addnoise_batch(batch, noise_src, noise_start, db):
    """addnoise() (enhancement_extract_subband_linux/cpp/extractwav.cpp:6-35) for every utterance of the batch: utterance u
    is mixed with noise_src[noise_start[u] : noise_start[u] + L_u] (an int16 tensor or array holding all noise recordings back
    to back) scaled to db[u] dB (ints).  Returns a dict: noise_scaled and noisy (int16 tensors laid out like batch.data),
    sums (float32 [n, 2]: the in-order float sums of squares of clean and noise) and gain (float32 [n]).  Asynchronous on the
    current stream."""
    torch = _torch()
    lib = _lib.load()
    noise_src, d_start, d_snr = _mix_inputs(batch, noise_src, noise_start, db)
    dev = batch.data.device
    scaled, noisy = torch.zeros_like(batch.data), torch.zeros_like(batch.data)
    sums = torch.zeros((batch.n_utt, 2), dtype=torch.float32, device=dev)
    gain = torch.zeros(batch.n_utt, dtype=torch.float32, device=dev)
    _lib.check(lib.sea_addnoise_batch(_dptr(batch.data), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(noise_src),
                                      _dptr(d_start), _dptr(d_snr), _dptr(scaled), _dptr(noisy), _dptr(sums), _dptr(gain),
                                      batch.n_utt, _stream_ptr()), "sea_addnoise_batch")
    return dict(noise_scaled=scaled, noisy=noisy, sums=sums, gain=gain)


def addnoise(clean, noise, db):
    """addnoise() on host arrays, one utterance (sea_addnoise): returns (noise_scaled, noisy, sums float32[2], gain)."""
    lib = _lib.load()
    clean = np.ascontiguousarray(clean, dtype=np.int16)
    noise = np.ascontiguousarray(noise, dtype=np.int16)
    if clean.shape != noise.shape or clean.ndim != 1:
        raise ValueError("addnoise needs a clean signal and a noise stretch of the same length")
    scaled, noisy = np.zeros_like(clean), np.zeros_like(clean)
    sums, gain = np.zeros(2, np.float32), np.zeros(1, np.float32)
    _lib.check(lib.sea_addnoise(_np_ptr(clean), _np_ptr(noise), clean.size, int(db), _np_ptr(scaled), _np_ptr(noisy),
                                _np_ptr(sums), _np_ptr(gain)), "sea_addnoise")
    return scaled, noisy, sums, gain[0]


def trainset_batch(batch, noise_src, noise_start, db, window=1, noisy_subband=False, use_order=True):
    """The training-set pipeline on the current stream (sea_trainset_batch): addnoise_batch, subband_batch of the clean and of
    the SCALED noise (and of the noisy signal with noisy_subband), irm_target_batch (clean, scaled noise).  Returns
    addnoise_batch's dict plus sub_clean, sub_noise, sub_noisy (int16 tensors as subband_batch returns them; sub_noisy None
    without noisy_subband) and irm (a MaskBatch)."""
    torch = _torch()
    lib = _lib.load()
    if np.any(np.asarray(batch.host_lengths) < 320):
        raise ValueError("trainset needs utterances of at least one 320-sample frame")
    noise_src, d_start, d_snr = _mix_inputs(batch, noise_src, noise_start, db)
    dev = batch.data.device
    scaled, noisy = torch.zeros_like(batch.data), torch.zeros_like(batch.data)
    sums = torch.zeros((batch.n_utt, 2), dtype=torch.float32, device=dev)
    gain = torch.zeros(batch.n_utt, dtype=torch.float32, device=dev)
    subs = [torch.zeros(batch.total * 64, dtype=torch.int16, device=dev) for _ in range(3 if noisy_subband else 2)]
    rows = (np.asarray(batch.host_lengths) - 320) // 160 + 1
    offs = _row_offsets(rows)
    irm = torch.zeros((int(rows.sum()), 64), dtype=torch.float32, device=dev)
    d_offs = torch.from_numpy(offs).to(dev)
    _lib.check(lib.sea_trainset_batch(_dptr(batch.data), _dptr(batch.offsets), _dptr(batch.lengths), _dptr(noise_src),
                                      _dptr(d_start), _dptr(d_snr), _dptr(scaled), _dptr(noisy), _dptr(sums), _dptr(gain),
                                      _dptr(subs[0]), _dptr(subs[1]), _dptr(subs[2]) if noisy_subband else None, _dptr(d_offs),
                                      _dptr(irm), int(window), _dptr(batch.order) if use_order else None, batch.n_utt,
                                      _stream_ptr()), "sea_trainset_batch")
    return dict(noise_scaled=scaled, noisy=noisy, sums=sums, gain=gain, sub_clean=subs[0], sub_noise=subs[1],
                sub_noisy=subs[2] if noisy_subband else None, irm=MaskBatch(irm, d_offs, offs, rows))


def make_trainset(clean_list, noises, rec, off, db, window=1, want_noise_scaled=False, want_subbands=False,
                  noisy_subband=False):
    """The reference's training-set loop from host memory (sea_trainset_utterances): clean_list[u] is mixed with
    noises[rec[u]][off[u] : off[u] + L_u] at db[u] dB; the list runs in chunks that fit the free HBM.  Returns a dict: noisy
    (list of int16 arrays), irm (list of float32 [(L-320)//160+1, 64]), noise_scaled (list or None), sub_clean / sub_noise
    (lists of int16 [64, L] or None), sub_noisy (the same, only with noisy_subband), chunks (how many the list was cut into)."""
    lib = _lib.load()
    xs = [np.ascontiguousarray(x, dtype=np.int16) for x in clean_list]
    ns = [np.ascontiguousarray(x, dtype=np.int16) for x in noises]
    n, m = len(xs), len(ns)
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    db = np.ascontiguousarray(db)
    if not np.issubdtype(db.dtype, np.integer):
        raise ValueError("addnoise takes whole dB values")
    db = db.astype(np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    if not (rec.shape == db.shape == off.shape == (n,)):
        raise ValueError("one recording index, offset and dB value per utterance")
    noisy = [np.zeros(x.size, np.int16) for x in xs]
    irm = [np.zeros((max((x.size - 320) // 160 + 1, 1), 64), np.float32) for x in xs]
    scaled = [np.zeros(x.size, np.int16) for x in xs] if want_noise_scaled else None
    blocks = lambda: [np.zeros((64, x.size), np.int16) for x in xs]
    sub_c, sub_n = (blocks(), blocks()) if want_subbands else (None, None)
    sub_y = blocks() if noisy_subband else None
    if n == 0:
        return dict(noisy=[], irm=[], noise_scaled=scaled, sub_clean=sub_c, sub_noise=sub_n, sub_noisy=sub_y, chunks=0)
    ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]) if arrs is not None else None
    lens = (ctypes.c_long * n)(*[x.size for x in xs])
    nlens = (ctypes.c_long * max(m, 1))(*[x.size for x in ns])
    offs = (ctypes.c_long * n)(*[int(v) for v in off])
    rc = lib.sea_trainset_utterances(ptrs(xs), lens, n, ptrs(ns), nlens, m, _np_ptr(rec), offs, _np_ptr(db), int(window),
                                     ptrs(noisy), ptrs(irm), ptrs(scaled), ptrs(sub_c), ptrs(sub_n), ptrs(sub_y))
    _lib.check(rc, "sea_trainset_utterances")
    return dict(noisy=noisy, irm=irm, noise_scaled=scaled, sub_clean=sub_c, sub_noise=sub_n, sub_noisy=sub_y,
                chunks=int(lib.sea_trainset_last_chunks()))


def ns16k_streams_push(frames, state=None, reset=None):
    """The 16 k-native NoiseSup variant behind the reference's batch plug-in symbols (aurora_etsi/NoiseSup.cpp:1140-1407;
    SURVEY 8(f) #4): frames float32 [B, nframes, 160] on the GPU, func_Wiener's frame gate applied inside.  Returns
    dict(out [B, nframes, 160], produced int32 [B, nframes], flags uint8 [B, nframes] (bit 0 SpeechFoundVar, 1 Spec, 2 Mel,
    3 VADNS), counter int32 [B, nframes] (0: the first stage did not run), wiener float32 [B, nframes, 25] (rows where
    produced), state); pass ``state`` back in to continue the same streams."""
    torch = _torch()
    lib = _lib.load()
    frames = frames.contiguous()
    B, nfr, hop = frames.shape
    assert hop == 160 and frames.dtype == torch.float32
    if state is None:
        state = torch.zeros((B, lib.sea_ns16k_state_floats()), dtype=torch.float32, device=frames.device)
        reset = True if reset is None else reset
    out = torch.zeros_like(frames)
    produced = torch.zeros((B, nfr), dtype=torch.int32, device=frames.device)
    flags = torch.zeros((B, nfr), dtype=torch.uint8, device=frames.device)
    counter = torch.zeros((B, nfr), dtype=torch.int32, device=frames.device)
    wiener = torch.zeros((B, nfr, 25), dtype=torch.float32, device=frames.device)
    rc = lib.sea_ns16k_streams_push(_dptr(frames), _dptr(out), _dptr(produced), _dptr(flags), _dptr(counter), _dptr(wiener),
                                    _dptr(state), B, nfr, int(bool(reset)), _stream_ptr())
    _lib.check(rc, "sea_ns16k_streams_push")
    return dict(out=out, produced=produced, flags=flags, counter=counter, wiener=wiener, state=state)


def ns16k_tables():
    """Host-side tables of the 16 k-native variant (no GPU needed), laid out as the reference's init code builds them."""
    lib = _lib.load()
    sw, iw, gs = np.zeros(480, np.float32), np.zeros(17, np.float32), np.zeros(25, np.int32)
    g, d = np.zeros((25, 128), np.float32), np.zeros((25, 25), np.float32)
    _lib.check(lib.sea_ns16k_tables_host(*[a.ctypes.data for a in (sw, iw, gs, g, d)]), "sea_ns16k_tables_host")
    return dict(sigWindow=sw, irWindow=iw, gammaStart=gs, gamma=g, idct=d)


def ns_streams_push(frames, state=None, reset=None, want_flags=False):
    """Batched DoNoiseSup: frames float32 [B, nframes, 80] on the GPU.  Returns (out, produced, state);
    pass ``state`` back in to continue the same streams.  want_flags: also return (flags uint8
    [B, nframes] with bit 0 SpeechFoundVar, 1 Spec, 2 Mel, 3 VADNS, frame_counter int32 [B, nframes]),
    the per-frame outputs of the reference's batch plug-in shape (NoiseSupExports.h:19-27)."""
    torch = _torch()
    lib = _lib.load()
    frames = frames.contiguous()
    B, nfr, hop = frames.shape
    assert hop == 80
    if state is None:
        state = torch.zeros((B, lib.sea_ns_state_floats()), dtype=torch.float32, device=frames.device)
        reset = True if reset is None else reset
    out = torch.zeros_like(frames)
    produced = torch.zeros((B, nfr), dtype=torch.int32, device=frames.device)
    if want_flags:
        flags = torch.zeros((B, nfr), dtype=torch.uint8, device=frames.device)
        counter = torch.zeros((B, nfr), dtype=torch.int32, device=frames.device)
        rc = lib.sea_ns_streams_push_fd(_dptr(frames), _dptr(out), _dptr(produced), _dptr(flags), _dptr(counter),
                                        _dptr(state), B, nfr, int(bool(reset)), _stream_ptr())
        _lib.check(rc, "sea_ns_streams_push_fd")
        return out, produced, state, flags, counter
    rc = lib.sea_ns_streams_push(_dptr(frames), _dptr(out), _dptr(produced), _dptr(state), B, nfr,
                                 int(bool(reset)), _stream_ptr())
    _lib.check(rc, "sea_ns_streams_push")
    return out, produced, state
