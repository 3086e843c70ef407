"""TEST INFRASTRUCTURE ONLY: the reference's wideband (16 kHz) mode driven through ctypes.

The reference build oracle/_ref/libetsi_ref.so (``make -C oracle ref``) already exports everything the mode needs:
AdvProcessAlloc (16000) switches Do16kHzProc on (etsi/cpp/ParmInterface.c:100-108), DoAdvProcess takes frames of 160
samples and writes 80 low-band int16 samples when NoiseSup produced a frame, and the Get16k_* getters hand out the
high-band state.  Three pointers at the head of FEParamsX (denoisedBuf, CurFrame, pData16k) are reached through a ctypes
mirror of the struct's scalar head; ``WbReference`` asserts four known values of that head after AdvProcessInit before it
uses any of them.  The high-band VAD's state is read 340 / 344 / 348 bytes into DataFor16kProc (nbSpeechFrames16k,
hangOver16k, meanEn16k; x86-64 LP64) and cross-checked through vadCounter16k at 328, which must count the second-stage
frames.

Loaded by the tests and by tools/gen_wb_golden.py only; nothing of the product imports it."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libetsi_ref.so")

_f32p = C.POINTER(C.c_float)
_SENTINEL = np.array([0x7A5A, -0x5A7B] * 40, dtype=np.int16)


class _FEHead(C.Structure):
    """etsi/cpp/ParmInterface.h:76-101, the part in front of the module pointers"""
    _fields_ = [(n, C.c_int) for n in (
        "Do16kHzProc", "Noc0", "VAD", "CoefNb", "FFTLength", "FrameShift", "FrameLength", "FrameCounter",
        "SpeechFoundMel", "SpeechFoundVar", "SpeechFoundSpec", "SpeechFoundVADNS", "NbSamplesToRead",
        "SamplingFrequency", "offsetDenoisedFrame")] + [
        ("StartingFrequency", C.c_float), ("NonZeroFrameOnset", C.c_long), ("ZeroFrameCounter", C.c_long),
        ("denoisedBuf", C.c_void_p), ("CurFrame", _f32p), ("pData16k", C.c_void_p)]


class _MelWin(C.Structure):
    """etsi/cpp/MelProcExports.h:21-26"""


_MelWin._fields_ = [("StartingPoint", C.c_int), ("Length", C.c_int), ("Data", _f32p), ("Next", C.POINTER(_MelWin))]


def available():
    return os.path.exists(REF_LIB)


def _load():
    if not available():
        raise FileNotFoundError(f"{REF_LIB} is missing: build it with `make -C oracle ref`")
    lib = C.CDLL(REF_LIB)
    vp, i = C.c_void_p, C.c_int
    lib.AdvProcessAlloc.restype, lib.AdvProcessAlloc.argtypes = vp, [i]
    lib.AdvProcessInit.restype, lib.AdvProcessInit.argtypes = None, [vp]
    lib.AdvProcessDelete.restype, lib.AdvProcessDelete.argtypes = None, [vp]
    lib.DoAdvProcess.restype, lib.DoAdvProcess.argtypes = i, [vp, vp, vp, vp]
    lib.DoNoiseSup.restype, lib.DoNoiseSup.argtypes = i, [vp, vp, vp]
    lib.DoCompCeps.restype, lib.DoCompCeps.argtypes = i, [vp, vp, vp]
    lib.BufInGetLast.restype, lib.BufInGetLast.argtypes = i, [vp, vp, i]
    lib.Do16kProcessing.restype, lib.Do16kProcessing.argtypes = None, [vp, vp, i]
    lib.Get16k_dataHP.restype, lib.Get16k_dataHP.argtypes = C.c_float, [vp, i]
    lib.Get16k_hpBandsSize.restype, lib.Get16k_hpBandsSize.argtypes = C.c_short, [vp]
    lib.Get16k_p_hpBands.restype, lib.Get16k_p_hpBands.argtypes = _f32p, [vp]
    lib.Get16k_p_CodeForBands16k.restype, lib.Get16k_p_CodeForBands16k.argtypes = _f32p, [vp]
    lib.Get16k_p_FirstWindow16k.restype, lib.Get16k_p_FirstWindow16k.argtypes = C.POINTER(_MelWin), [vp]
    return lib


class WbReference:
    """One front end of the reference, allocated for 16 kHz (or 8 kHz) input and initialised."""

    def __init__(self, sampling_frequency=16000):
        self.lib = _load()
        self.fe = self.lib.AdvProcessAlloc(int(sampling_frequency))
        assert self.fe
        self.head = _FEHead.from_address(self.fe)
        self.head.Noc0 = 0
        self.lib.AdvProcessInit(self.fe)
        h = self.head
        wide = sampling_frequency == 16000
        # the struct-head checks: a mirror that is off by a field fails here, before a pointer is used
        assert h.SamplingFrequency == 8000 and h.FrameShift == 80 and h.FrameLength == 200, "FEParamsX mirror is off"
        assert h.NbSamplesToRead == (160 if wide else 80) and h.Do16kHzProc == (1 if wide else 0), "FEParamsX mirror is off"
        assert h.denoisedBuf and h.CurFrame and (h.pData16k or not wide)
        self.wide = wide

    def close(self):
        if self.fe:
            p = C.c_void_p(self.fe)
            self.lib.AdvProcessDelete(C.byref(p))
            self.fe = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # the high-band VAD's state behind pData16k
    def _d16(self, offset, ctype):
        return ctype.from_address(self.head.pData16k + offset).value

    def vad16k(self):
        return dict(counter=self._d16(328, C.c_long), nbSpeech=self._d16(340, C.c_int), hangOver=self._d16(344, C.c_int),
                    meanEn=self._d16(348, C.c_float))

    def qmf(self, frame160):
        """Do16kProcessing alone on one frame of 160 floats -> (low band 80, high band 80)."""
        buf = np.array(frame160, dtype=np.float32, copy=True)
        assert buf.size == 160
        self.lib.Do16kProcessing(buf.ctypes.data, self.head.pData16k, 160)
        hp = np.array([self.lib.Get16k_dataHP(self.head.pData16k, i) for i in range(80)], dtype=np.float32)
        return buf[:80].copy(), hp

    def noise_sup(self, frame80):
        """DoNoiseSup on one frame of 80 floats (the 8 kHz front end) -> 80 floats or None."""
        x = np.ascontiguousarray(frame80, dtype=np.float32)
        y = np.zeros(80, np.float32)
        return y if self.lib.DoNoiseSup(x.ctypes.data, y.ctypes.data, self.fe) else None


def hp_mel_windows():
    """The five windows of the high band's mel filter as the reference built them: [(start, weights), ..]."""
    ref = WbReference()
    out = []
    w = ref.lib.Get16k_p_FirstWindow16k(ref.head.pData16k)
    while w:
        win = w.contents
        out.append((int(win.StartingPoint), np.ctypeslib.as_array(win.Data, shape=(win.Length,)).copy()))
        w = win.Next
    ref.close()
    return out


def qmf_taps():
    """Both filters' 118 taps from two unit impulses through the reference's Do16kProcessing: output k of an impulse at
    sample p of a first frame is tap 117 + p - 2 k (the down-shift sign (-1)^k of the high band undone)."""
    lp, hp = np.zeros(118, np.float32), np.zeros(118, np.float32)
    for p in (0, 1):
        ref = WbReference()
        x = np.zeros(160, np.float32)
        x[p] = 1.0
        outs = [ref.qmf(x)]
        outs.append(ref.qmf(np.zeros(160, np.float32)))
        ref.close()
        lo = np.concatenate([o[0] for o in outs])
        hi = np.concatenate([o[1] for o in outs])
        for k in range(160):
            j = 117 + p - 2 * k
            if 0 <= j < 118:
                lp[j] = lo[k]
                hp[j] = -hi[k] if (k % 80) & 1 else hi[k]
    return lp, hp


def trace(x, want_qmf=False):
    """The reference's wideband mode on int16 samples at 16 kHz, frame by frame (the order of oracle/ref_driver.c::
    ref_ns_trace).  Returns a dict:
      out_i16   80 * (len // 160) low-band samples as a per-frame copy would write them: zeros until the first output
      f32       [nout, 80] float NoiseSup outputs (from BufInGetLast)
      hp        [nout, 3]  the high-band energies after DoSpecSub16k (the last three of hpBands after each output)
      code      [nout, 9]  CodeForBands16k after each output
      ceps      [nceps, 14] DoCompCeps from the third output on
      first_out, onset     frame indices (-1 / the frame count if none)
      vad_states [3]       second-stage frames the high-band VAD spent in a speech run / in hang-over / idle
      qmf_lp, qmf_hp       (want_qmf) [nfr, 80] CurFrame[0..79] and Get16k_dataHP per frame, NaN before the onset"""
    x = np.ascontiguousarray(x, dtype=np.int16)
    nfr = x.size // 160
    ref = WbReference()
    lib, head = ref.lib, ref.head
    out = np.zeros(nfr * 80, np.int16)
    f32, hp, code, ceps = [], [], [], []
    qlp = np.full((nfr, 80), np.nan, np.float32)
    qhp = np.full((nfr, 80), np.nan, np.float32)
    first_out, onset = -1, nfr
    states = [0, 0, 0]
    den = np.zeros(80, np.int16)
    feat = np.zeros(16, np.float32)
    buf = np.zeros(241 + 3, np.float32)
    pd = head.pData16k
    for f in range(nfr):
        sig = x[f * 160:(f + 1) * 160].copy()
        den[:] = _SENTINEL
        before = ref.vad16k()
        lib.DoAdvProcess(sig.ctypes.data, den.ctypes.data, feat.ctypes.data, ref.fe)  # return value: SURVEY F4
        if head.NonZeroFrameOnset and onset == nfr:
            onset = f
        if want_qmf and head.NonZeroFrameOnset:
            qlp[f] = np.ctypeslib.as_array(head.CurFrame, shape=(160,))[:80]
            qhp[f] = [lib.Get16k_dataHP(pd, i) for i in range(80)]
        after = ref.vad16k()
        if after["counter"] != before["counter"]:  # the second stage ran: DoSpecSub16k was called
            if after["nbSpeech"] > 0:
                states[0] += 1
            elif (15 if before["nbSpeech"] > 4 else before["hangOver"]) != 0:
                states[1] += 1
            else:
                states[2] += 1
        if not np.array_equal(den, _SENTINEL):
            if first_out < 0:
                first_out = f
            out[f * 80:(f + 1) * 80] = den
            lib.BufInGetLast(head.denoisedBuf, buf.ctypes.data, 241)
            f32.append(buf[161:241].copy())
            n = int(lib.Get16k_hpBandsSize(pd))
            hp.append(np.ctypeslib.as_array(lib.Get16k_p_hpBands(pd), shape=(n,))[n - 3:].copy())
            code.append(np.ctypeslib.as_array(lib.Get16k_p_CodeForBands16k(pd), shape=(9,)).copy())
            if len(f32) >= 3:
                lib.DoCompCeps(buf.ctypes.data + 4, feat.ctypes.data, ref.fe)
                ceps.append(feat[:14].copy())
    nstage1 = ref.vad16k()["counter"]
    ref.close()
    nout = len(f32)
    assert sum(states) == nout and (nout == 0 or nstage1 == nout), (states, nstage1, nout)
    res = dict(out_i16=out, f32=np.array(f32, np.float32).reshape(nout, 80), hp=np.array(hp, np.float32).reshape(nout, 3),
               code=np.array(code, np.float32).reshape(nout, 9), ceps=np.array(ceps, np.float32).reshape(len(ceps), 14),
               first_out=first_out, onset=onset, vad_states=np.array(states, np.int64))
    if want_qmf:
        res.update(qmf_lp=qlp, qmf_hp=qhp)
    return res


def ns_8k_on_frames(frames80):
    """The reference's own 8 kHz DoNoiseSup fed float frames: [nout, 80] outputs and the index of the first."""
    ref = WbReference(8000)
    outs, first = [], -1
    for f, fr in enumerate(frames80):
        y = ref.noise_sup(fr)
        if y is not None:
            if first < 0:
                first = f
            outs.append(y)
    ref.close()
    return np.array(outs, np.float32).reshape(len(outs), 80), first
