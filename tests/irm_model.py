"""An independent float64 model of the ideal-ratio-mask target (oracle/resynth_oracle.c, ora_irm_target; the device form is
csrc/irm_kernel.hip) -- numpy only, no loop over bins, no table of the restatement's.

Definition: per channel c of the two [64][L] int16 blocks, frames of 320 samples every 160, F = (L - 320) // 160 + 1.  The window is
the double formula rounded to float (kind 0 rectangular, 1 Hamming 0.54 - 0.46 cos(2 pi n / 319), 2 Hanning 0.5 - 0.5 cos(2 pi n / 319))
and multiplied by the float sample IN FLOAT, as the restatement and the kernel both do; from there on everything is double: the
512-point spectrum of the zero-padded frame (numpy.fft.rfft), |X[k]|^2 over bins 0..63 summed, IRM = P / (P + N).  Output [F][64]
float64, NaN where both sums are 0.

Every misreading the tests must be able to see is a keyword of irm(), so model and mutants are one text; MUTANTS names them.
"""
import numpy as np

FRAME, HOP, NFFT, NBINS, NCHAN, TILE = 320, 160, 512, 64, 64, 16


def n_frames(L):
    return (L - FRAME) // HOP + 1 if L >= FRAME else 0


def window(kind, denominator=319.0):
    n = np.arange(FRAME, dtype=np.float64)
    if kind == 1:
        w = 0.54 - 0.46 * np.cos(2.0 * np.pi * n / denominator)
    elif kind == 2:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / denominator)
    else:
        w = np.ones(FRAME)
    return w.astype(np.float32)


def _frames(x, starts):
    """[64][L] int16 -> [64][F][320] int16, frame f from starts[f]; samples from L on read as 0"""
    L = x.shape[1]
    pad = np.concatenate([x, np.zeros((x.shape[0], FRAME + HOP + 8), x.dtype)], axis=1)
    idx = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(FRAME)[None, :]
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < pad.shape[1]), (L, idx.max())
    return pad[:, idx]


def irm(pure, noise, kind=1, *, window_denominator=319.0, window_as=None, late_start=0, skip_bin=None, extra_bin=None,
        bin_gain=None, skip_component=None, component_gain=None, slot15_reads_next_tile=False, noise_from_pure_tile=None,
        tail_into_last_row=False):
    """The model.  The keywords (all off by default) are the mutants:
      window_denominator   the window's /319 read as another figure (320)
      window_as            another window kind than the one asked for
      late_start           frames after the first start this many samples late
      skip_bin             this bin left out of the sum (63)
      extra_bin            this bin taken in as well (64)
      bin_gain             (k, factor): the power of bin k times factor
      skip_component       polyphase component r (samples 4 m + r of the frame) left out
      component_gain       (r, factor): polyphase component r scaled
      slot15_reads_next_tile  frame slot 15 of every 16-frame tile reads the next tile's first frame (160 samples on)
      noise_from_pure_tile the noise sum of this tile (frames 16 t .. 16 t + 15) is the pure stream's
      tail_into_last_row   the power of the incomplete frame F (the samples from 160 F on, then zeros) is added into row F - 1
    """
    pure, noise = np.asarray(pure), np.asarray(noise)
    assert pure.dtype == np.int16 and noise.dtype == np.int16 and pure.shape == noise.shape and pure.shape[0] == NCHAN
    L = pure.shape[1]
    F = n_frames(L)
    if F == 0:
        return np.zeros((0, NCHAN))
    w = window(kind if window_as is None else window_as, window_denominator)
    starts = HOP * np.arange(F + 1)                        # the last one is the incomplete frame behind the utterance
    starts[1:F] += late_start
    if slot15_reads_next_tile:
        starts[:F][np.arange(F) % TILE == TILE - 1] += HOP

    def sums(x):
        fr = _frames(x, starts).astype(np.float32) * w     # float32 x float32 -> float32, rounded once
        fr = fr.astype(np.float64)
        if skip_component is not None:
            fr[..., skip_component::4] = 0.0
        if component_gain is not None:
            fr[..., component_gain[0]::4] *= component_gain[1]
        spec = np.fft.rfft(fr, NFFT, axis=-1)
        power = spec.real ** 2 + spec.imag ** 2            # [64][F + 1][257]
        if bin_gain is not None:
            power[..., bin_gain[0]] *= bin_gain[1]
        keep = np.zeros(NFFT // 2 + 1, bool)
        keep[:NBINS] = True
        if skip_bin is not None:
            keep[skip_bin] = False
        if extra_bin is not None:
            keep[extra_bin] = True
        s = power[..., keep].sum(axis=-1)                  # [64][F + 1]
        if tail_into_last_row:
            s[:, F - 1] += s[:, F]
        return s[:, :F]

    P, N = sums(pure), sums(noise)
    if noise_from_pure_tile is not None:
        t = noise_from_pure_tile
        N[:, TILE * t:TILE * (t + 1)] = P[:, TILE * t:TILE * (t + 1)]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = P / (P + N)
    return np.ascontiguousarray(r.T)


# name -> keywords; the figures behind each are printed by tests/test_irm_cpu.py
MUTANTS = {
    "window /320": dict(window_denominator=320.0),
    "Hanning for Hamming": dict(window_as=2),
    "rectangular for Hamming": dict(window_as=0),
    "frames start one sample late": dict(late_start=1),
    "bin 63 left out": dict(skip_bin=63),
    "bin 64 included": dict(extra_bin=64),
    "one bin's power off by 0.2 %": dict(bin_gain=(21, 1.002)),
    "polyphase component 3 left out": dict(skip_component=3),
    "slot 15 reads the next tile": dict(slot15_reads_next_tile=True),
    "noise sum of tile 1 from the pure stream": dict(noise_from_pure_tile=1),
    "tile tail taken into the last row": dict(tail_into_last_row=True),
}
# the three small errors the issue measured on the inputs of test_irm_target_vs_oracle: all under the old 1e-4
SMALL_MUTANTS = {
    "one bin's power off by 0.2 %": dict(bin_gain=(21, 1.002)),
    "bin 63 off by 1 %": dict(bin_gain=(63, 1.01)),
    "polyphase component 1 scaled by 1.0005": dict(component_gain=(1, 1.0005)),
}
