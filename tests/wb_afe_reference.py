"""TEST INFRASTRUCTURE ONLY: the reference's wideband (16 kHz) FEATURE CHAIN driven through ctypes.

The reference keeps the chain after NoiseSup commented out of DoAdvProcess (etsi/cpp/ParmInterface.c:274-311); its pieces
are all exported by the reference build oracle/_ref/libetsi_ref.so (``make -C oracle ref``): DoWaveProc, DoCompCeps,
DoPostProc, DoVADProc and FlushAdvProcess.  ``trace`` calls them in the order of that block -- the order of
oracle/ref_driver.c::ref_afe_trace -- on a front end allocated with AdvProcessAlloc (16000), Noc0 = 0.  The struct mirror,
its checks and the library loader are tests/wb_reference.py's.

Loaded by the tests and by tools/gen_wb_afe_golden.py only; nothing of the product imports it."""
import ctypes as C

import numpy as np

from tests import wb_reference as W

available = W.available


def _prototypes(lib):
    vp, i = C.c_void_p, C.c_int
    for name in ("DoWaveProc", "DoPostProc", "DoVADProc", "DoVADFlush", "FlushAdvProcess"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i, [vp, vp]


def trace(x):
    """The reference's wideband chain on int16 samples at 16 kHz.  Returns a dict:
      feat_cc   [nceps, 14] after DoWaveProc + DoCompCeps          feat_pp  [nceps, 14] after DoPostProc
      feat15    [nemit, 15] emitted frames in emission order: null vectors of the all-zero lead, DoVADProc's, the flush's
      flags     [nout] one byte per frame with a NoiseSup output: bit 0 SpeechFoundVar, 1 Spec, 2 Mel, 3 VADNS after it
      out_frames [nout] indices of those frames                     n_null   emitted null vectors of the lead
      bypass    [nceps] the in-order float64 sum of squares of the frame's 200 samples was < 100 (DoWaveProc left it alone)
      logE      [nceps] feat_cc[:, 13]                              first_out, onset   as tests/wb_reference.py::trace"""
    x = np.ascontiguousarray(x, dtype=np.int16)
    nfr = x.size // 160
    ref = W.WbReference()
    lib, head = ref.lib, ref.head
    _prototypes(lib)
    assert head.offsetDenoisedFrame == -head.FrameLength, "FEParamsX mirror is off"
    den = np.zeros(80, np.int16)
    feat = np.zeros(16, np.float32)
    buf = np.zeros(241 + 3, np.float32)
    feat_cc, feat_pp, feat15, flags, out_frames, bypass = [], [], [], [], [], []
    first_out, onset, n_null = -1, nfr, 0
    for f in range(nfr):
        sig = x[f * 160:(f + 1) * 160].copy()
        den[:] = W._SENTINEL
        zeros_before = head.ZeroFrameCounter
        lib.DoAdvProcess(sig.ctypes.data, den.ctypes.data, feat.ctypes.data, ref.fe)  # return value: SURVEY F4
        if head.NonZeroFrameOnset and onset == nfr:
            onset = f
        if head.ZeroFrameCounter > zeros_before:  # null MFCC vector, VAD = NON_SPEECH (ParmInterface.c:314-329)
            assert not feat[:14].any()
            feat15.append(np.zeros(15, np.float32))
            n_null += 1
        if np.array_equal(den, W._SENTINEL):
            continue
        if first_out < 0:
            first_out = f
        out_frames.append(f)
        if head.offsetDenoisedFrame < 0:
            head.offsetDenoisedFrame += head.FrameShift
        cepstral = head.offsetDenoisedFrame >= 0
        if cepstral:
            n = head.FrameLength + head.offsetDenoisedFrame + 1
            assert n == 241
            lib.BufInGetLast(head.denoisedBuf, buf.ctypes.data, n)
            before = buf[1:201].copy()
            energy = 0.0
            for v in before.astype(np.float64):
                energy += v * v
            bypass.append(energy < 100.0)
            lib.DoWaveProc(buf.ctypes.data + 4, ref.fe)
            assert np.array_equal(before, buf[1:201]) == bypass[-1], "the float64 sum and DoWaveProc's own check disagree"
            lib.DoCompCeps(buf.ctypes.data + 4, feat.ctypes.data, ref.fe)
            feat_cc.append(feat[:14].copy())
            lib.DoPostProc(feat.ctypes.data, ref.fe)
            feat_pp.append(feat[:14].copy())
        flags.append((1 if head.SpeechFoundVar else 0) | (2 if head.SpeechFoundSpec else 0) | (4 if head.SpeechFoundMel else 0)
                     | (8 if head.SpeechFoundVADNS else 0))
        if cepstral and lib.DoVADProc(feat.ctypes.data, ref.fe):
            feat15.append(feat[:15].copy())
    while lib.FlushAdvProcess(feat.ctypes.data, ref.fe):
        feat15.append(feat[:15].copy())
    ref.close()
    nceps = len(feat_cc)
    cc = np.array(feat_cc, np.float32).reshape(nceps, 14)
    return dict(feat_cc=cc, feat_pp=np.array(feat_pp, np.float32).reshape(nceps, 14),
                feat15=np.array(feat15, np.float32).reshape(len(feat15), 15), flags=np.array(flags, np.uint8),
                out_frames=np.array(out_frames, np.int32), n_null=n_null, bypass=np.array(bypass, bool), logE=cc[:, 13].copy(),
                first_out=first_out, onset=onset)


def pp_weight(logE):
    """DoPostProc's weighting before its clamp (PostProc.c:129), in float32 as the reference takes it."""
    e = np.asarray(logE, np.float32)
    return (e * np.float32(64) - np.float32(211)) / np.float32(64)
