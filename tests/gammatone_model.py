"""tests/gammatone_model.py -- TEST INFRASTRUCTURE ONLY: an independent float64 model of the gammatone / resynthesis half.

Written from the formulas of resyth_64sub_ori/cpp/extractwav.cpp:41-54,133-211,258-278 and HuWang.h alone; it imports
neither the oracle nor the library's tables (numpy only) and shares no structure with oracle/resynth_oracle.c or
csrc/resynth_kernel.hip: where those run the 4-stage complex recursion sample by sample in float32, this evaluates

    out[n] = gain * sum_{k>=1} k^3 e^{-2 pi bw k/fs} cos(2 pi cf k/fs) in[n-k],   gain = midEar (2 pi bw/fs)^4 / 3

-- the sampled gammatone t^3 e^{-2 pi b t} cos(2 pi f t) -- as one FIR convolution through numpy.fft.  Derivation: with
a = (f1 + j f2) = e^{-2 pi bw/fs} e^{j 2 pi cf/fs}, s_i = p_i + j q_i and u = a z^-1 the recurrences of :199-209 read
S0 = aX/(1-u), S1 = S0/(1-u), S2 = S1 (1+u)/(1-u), S3 (1-u) = S2 (1+2u) + u S1, hence S3 = aX (1+4u+u^2)/(1-u)^4
= X sum_{k>=1} k^3 a^k z^-(k-1); the output is taken BEFORE the update (:192), one more sample of delay.
tests/test_resynth_model_cpu.py checks this algebra against the literal recurrences (`recurrence_bank`) instead of
trusting it.

A `Model` is built with the reading of the source it encodes; the defaults are the source's, every other value is one
plausible MISREADING (a mutant) that the tests must be able to tell from the truth:
    after_update    output[n] taken after the state update instead of before
    x2_coeff        the coefficient of x[2] in p[3] (source: 2)
    gain_div3       the /3 of the gain
    rise_guard      `if (frame > 0)` around the rising half-window.  Without it frame 0 would have a rising half too, which
                    has no sample to land on before the signal; the mutant is the in-bounds form of that reading: every
                    frame carries both halves and window f is laid from sample f*160, not (f-1)*160
    ibm_ge          the binary mask's threshold as >= 0.5 instead of > 0.5
    ear_div_twice   the division by midEarCoeff after BOTH passes (:87, :90) instead of once
    bs3383_nearest  the nearest BS3383 table row instead of linear interpolation between two
"""
import numpy as np

FS = 16000
NCHAN = 64
WINDOW = FS // 50
OFFSET = FS // 100

# BS3383 table 1 (equal-loudness contours): frequency, af, bf, tf -- data of a public standard
_BS_F = np.array([20.0, 25.0, 31.5, 40.0, 50.0, 63.0, 80.0, 100.0, 125.0, 160.0, 200.0, 250.0, 315.0, 400.0, 500.0, 630.0,
                  800.0, 1000.0, 1250.0, 1600.0, 2000.0, 2500.0, 3150.0, 4000.0, 5000.0, 6300.0, 8000.0, 10000.0, 12500.0])
_BS_AF = np.array([2.347, 2.190, 2.050, 1.879, 1.724, 1.579, 1.512, 1.466, 1.426, 1.394, 1.372, 1.344, 1.304, 1.256, 1.203,
                   1.135, 1.062, 1.000, 0.967, 0.943, 0.932, 0.933, 0.937, 0.952, 0.974, 1.027, 1.135, 1.266, 1.501])
_BS_BF = np.array([0.00561, 0.00527, 0.00481, 0.00404, 0.00383, 0.00286, 0.00259, 0.00257, 0.00256, 0.00255, 0.00254, 0.00248,
                   0.00229, 0.00201, 0.00162, 0.00111, 0.00052, 0.00000, -0.00039, -0.00067, -0.00092, -0.00105, -0.00104,
                   -0.00088, -0.00055, 0.00000, 0.00089, 0.00211, 0.00488])
_BS_TF = np.array([74.3, 65.0, 56.3, 48.4, 41.7, 35.5, 29.8, 25.1, 20.7, 16.8, 13.8, 11.2, 8.9, 7.2, 6.0, 5.0, 4.4, 4.2, 3.7, 2.6,
                   1.0, -1.2, -3.6, -3.9, -1.1, 6.6, 15.3, 16.4, 11.6])

# Meddis 1988 hair cell constants (HuWang.h:36-44)
MED_Y, MED_G, MED_L, MED_R, MED_X, MED_A, MED_B, MED_H, MED_M = 5.05, 2000.0, 2500.0, 6580.0, 66.31, 3.0, 300.0, 48000.0, 1.0


class Model:
    def __init__(self, after_update=False, x2_coeff=2.0, gain_div3=True, rise_guard=True, ibm_ge=False, ear_div_twice=True,
                 bs3383_nearest=False):
        self.after_update = bool(after_update)
        self.x2_coeff = float(x2_coeff)
        self.gain_div3 = bool(gain_div3)
        self.rise_guard = bool(rise_guard)
        self.ibm_ge = bool(ibm_ge)
        self.ear_div_twice = bool(ear_div_twice)
        self.bs3383_nearest = bool(bs3383_nearest)
        self._banks = {}
        # channel table, extractwav.cpp:41-54: 64 centre frequencies equally spaced on the ERB-rate scale 50 Hz .. 8 kHz
        erb = np.linspace(21.4 * np.log10(50 * 0.00437 + 1.0), 21.4 * np.log10(8000 * 0.00437 + 1.0), NCHAN)
        self.cf = (10.0 ** (erb / 21.4) - 1.0) / 0.00437
        self.bw = 24.7 * (self.cf * 0.00437 + 1.0) * 1.019
        self.midEar = 10.0 ** ((self.loudness_phons(self.cf) - 60.0) / 20.0)
        # filter coefficients, :175-182
        T = 2.0 * np.pi / FS
        self.gain = self.midEar * (T * self.bw) ** 4 / (3.0 if self.gain_div3 else 1.0)
        self.f1 = np.cos(self.cf * T) * np.exp(-T * self.bw)
        self.f2 = np.sin(self.cf * T) * np.exp(-T * self.bw)

    def loudness_phons(self, freq):
        """BS3383 section 4 at 60 dB, table rows interpolated linearly in frequency (:258-278)"""
        freq = np.asarray(freq, dtype=np.float64)
        if self.bs3383_nearest:
            i = np.abs(freq[..., None] - _BS_F).argmin(-1)
            af, bf, tf = _BS_AF[i], _BS_BF[i], _BS_TF[i]
        else:
            af, bf, tf = (np.interp(freq, _BS_F, t) for t in (_BS_AF, _BS_BF, _BS_TF))
        return 4.2 + af * (60.0 - tf) / (1.0 + bf * (60.0 - tf))

    # ---- the filter ------------------------------------------------------------------------------------------------
    def _closed_form(self):
        return not self.after_update and self.x2_coeff == 2.0

    def impulse_bank(self, n):
        """[64][n]: every channel's response to a unit impulse at sample 0"""
        if not self._closed_form():
            imp = np.zeros(n)
            imp[:1] = 1.0
            return self.recurrence_bank(imp)
        k = np.arange(n, dtype=np.float64)
        T = 2.0 * np.pi / FS
        return self.gain[:, None] * k ** 3 * np.exp(-T * self.bw[:, None] * k) * np.cos(T * self.cf[:, None] * k)

    def impulse_response(self, c, n):
        return self.impulse_bank(n)[c]

    def recurrence_bank(self, x):
        """The literal recurrences of :184-210 in float64, all 64 channels side by side (x is [n] or [64][n])."""
        x = np.asarray(x, dtype=np.float64)
        n = x.shape[-1]
        xin = np.broadcast_to(x, (NCHAN, n))
        f1, f2, gain, c2 = self.f1, self.f2, self.gain, self.x2_coeff
        p = [np.zeros(NCHAN) for _ in range(4)]
        q = [np.zeros(NCHAN) for _ in range(4)]
        out = np.zeros((NCHAN, n))
        for t in range(n):
            if not self.after_update:
                out[:, t] = p[3] * gain
            xs = [f1 * p[i] - f2 * q[i] for i in range(4)]
            ys = [f2 * p[i] + f1 * q[i] for i in range(4)]
            p[0] = xin[:, t] * f1 + xs[0]
            q[0] = xin[:, t] * f2 + ys[0]
            p[1] = p[0] + xs[1]
            q[1] = q[0] + ys[1]
            p[2] = p[1] + xs[1] + xs[2]
            q[2] = q[1] + ys[1] + ys[2]
            p[3] = p[2] + xs[1] + c2 * xs[2] + xs[3]
            q[3] = q[2] + ys[1] + c2 * ys[2] + ys[3]
            if self.after_update:
                out[:, t] = p[3] * gain
        return out

    def _bank_spectrum(self, n):
        if n not in self._banks:
            if len(self._banks) >= 2:
                self._banks.clear()
            nfft = 1 << max(2 * n - 1, 1).bit_length()
            self._banks[n] = (nfft, np.fft.rfft(self.impulse_bank(n), nfft, axis=-1))
        return self._banks[n]

    def gammatone_bank(self, x, chans=None):
        """x: [n] (one input for every channel) or [len(chans)][n] (one input per channel) -> [len(chans)][n]"""
        x = np.asarray(x, dtype=np.float64)
        chans = np.arange(NCHAN) if chans is None else np.atleast_1d(chans)
        n = x.shape[-1]
        out = np.zeros((len(chans), n))
        if n == 0:
            return out
        nfft, H = self._bank_spectrum(n)
        X = np.fft.rfft(x, nfft, axis=-1)
        for lo in range(0, len(chans), 16):                      # 16 channels at a time: bounded memory at n = 48000
            sl = slice(lo, lo + 16)
            out[sl] = np.fft.irfft((X[sl] if X.ndim == 2 else X) * H[chans[sl]], nfft, axis=-1)[:, :n]
        return out

    def gammatone(self, x, c):
        return self.gammatone_bank(x, [c])[0]

    # ---- the overlap-add weights, :91-107 --------------------------------------------------------------------------
    @staticmethod
    def frame_count(L, frames_l_over_160=False):
        return L // OFFSET if frames_l_over_160 else (L - WINDOW) // OFFSET + 1

    def ola_weights(self, mask, L, binary=False, frames_l_over_160=False):
        """[64][L]: frame f's raised cosine is centred on sample f*160 -- its rising half 0.5 (1 - cos(pi j/160)) covers
        hop f-1 (none for frame 0), its falling half 0.5 (1 + cos(pi j/160)) hop f -- and is scaled by the mask entry
        where that is > 0 (ratio mask) or by 1 where it is > 0.5 (binary mask)."""
        mask = np.asarray(mask, dtype=np.float64)
        F = self.frame_count(L, frames_l_over_160)
        assert mask.shape == (F, NCHAN) and F >= 1
        if binary:
            m = ((mask >= 0.5) if self.ibm_ge else (mask > 0.5)).astype(np.float64)
        else:
            m = np.where(mask > 0, mask, 0.0)
        j = np.arange(OFFSET)
        up, down = 0.5 * (1.0 - np.cos(np.pi * j / OFFSET)), 0.5 * (1.0 + np.cos(np.pi * j / OFFSET))
        hops = -(-L // OFFSET) + 2
        if self.rise_guard:                          # hop h: falling half of frame h, rising half of frame h + 1
            fall = np.vstack([m, np.zeros((hops - F, NCHAN))])
            rise = np.vstack([m[1:], np.zeros((hops - F + 1, NCHAN))])
        else:                                        # mutant: window f starts at f*160 with both halves
            rise = np.vstack([m, np.zeros((hops - F, NCHAN))])
            fall = np.vstack([np.zeros((1, NCHAN)), m, np.zeros((hops - F - 1, NCHAN))])
        w = fall[:, None, :] * down[None, :, None] + rise[:, None, :] * up[None, :, None]      # [hop][j][chan]
        return w.reshape(hops * OFFSET, NCHAN)[:L].T

    # ---- resynth(), :55-121 ----------------------------------------------------------------------------------------
    def resynth(self, x, mask, binary=False, frames_l_over_160=False):
        """forward filter, / midEar, reverse, filter, / midEar, reverse, weight, channel sum: the float64 sum [L] before
        the cast to short"""
        x = np.asarray(x, dtype=np.float64)
        L = x.shape[0]
        me = self.midEar[:, None]
        g = self.gammatone_bank(x)
        g = self.gammatone_bank((g / me)[:, ::-1])
        g = (g / me if self.ear_div_twice else g)[:, ::-1]
        return np.sum(self.ola_weights(mask, L, binary, frames_l_over_160) * g, axis=0)

    # ---- subbband(): gammatone + Meddis hair cell, :212-257 --------------------------------------------------------
    @staticmethod
    def haircell(g):
        """The difference scheme of Meddis' transmitter model on g [..., n] (any leading shape) -> firing rate [..., n]"""
        g = np.asarray(g, dtype=np.float64)
        dt = 1.0 / FS
        ymdt, xdt, ydt = MED_Y * MED_M * dt, MED_X * dt, MED_Y * dt
        lplusrdt, rdt, gdt, hdt = (MED_L + MED_R) * dt, MED_R * dt, MED_G * dt, MED_H
        kt0 = MED_G * MED_A / (MED_A + MED_B)
        c0 = MED_M * MED_Y * kt0 / (MED_L * kt0 + MED_Y * (MED_L + MED_R))
        lead = g.shape[:-1]
        c = np.full(lead, c0)
        q = np.full(lead, c0 * (MED_L + MED_R) / kt0)
        w = np.full(lead, c0 * MED_R / MED_X)
        out = np.zeros(g.shape)
        for n in range(g.shape[-1]):
            s = g[..., n] + MED_A
            kt = np.where(s > 0.0, gdt * s / np.where(s > 0.0, s + MED_B, 1.0), 0.0)
            replenish = np.where(q < MED_M, ymdt - ydt * q, 0.0)
            eject = kt * q
            reuptakeandloss = lplusrdt * c
            reuptake = rdt * c
            reprocess = xdt * w
            q = np.maximum(q + replenish - eject + reprocess, 0.0)
            c = np.maximum(c + eject - reuptakeandloss, 0.0)
            w = np.maximum(w + reuptake - reprocess, 0.0)
            out[..., n] = hdt * c
        return out

    def subband(self, x, chans=None):
        """[len(chans)][L] float64: the hair cell's output per channel before the cast to short"""
        return self.haircell(self.gammatone_bank(x, chans))


_DEFAULT = Model()
cf, bw, midEar, gain, f1, f2 = _DEFAULT.cf, _DEFAULT.bw, _DEFAULT.midEar, _DEFAULT.gain, _DEFAULT.f1, _DEFAULT.f2
impulse_response = _DEFAULT.impulse_response
gammatone = _DEFAULT.gammatone
gammatone_bank = _DEFAULT.gammatone_bank
ola_weights = _DEFAULT.ola_weights
resynth = _DEFAULT.resynth
haircell = Model.haircell
subband = _DEFAULT.subband

MUTANTS = {
    "output_after_update": dict(after_update=True),
    "x2_not_doubled": dict(x2_coeff=1.0),
    "gain_without_div3": dict(gain_div3=False),
    "no_frame0_guard": dict(rise_guard=False),
    "ibm_threshold_ge": dict(ibm_ge=True),
    "ear_division_once": dict(ear_div_twice=False),
    "bs3383_nearest_row": dict(bs3383_nearest=True),
}


def cast_short(v):
    """The reference's (short) of a float (extractwav.cpp:120-121 as x86 compilers do it): truncate toward zero, keep
    the low 16 bits."""
    t = np.trunc(np.asarray(v, dtype=np.float64)).astype(np.int64)
    return ((t + 32768) % 65536 - 32768).astype(np.int16)


def wrapped_absdiff(a, b):
    """|a - b| of two int16 arrays in arithmetic modulo 2^16: a 1-LSB disagreement that straddles the wrap counts as 1"""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return np.abs((d + 32768) % 65536 - 32768)


def int16_figures(got, want):
    """(max |delta| in LSB, share of differing samples) in wrapped arithmetic; (0, 0.0) for empty arrays"""
    d = wrapped_absdiff(got, want)
    return (int(d.max()), float(np.mean(d != 0))) if d.size else (0, 0.0)


def stream_figure(got, want):
    """worst max |delta| / peak over the rows of two [rows][n] float streams (rows whose model is all zero: absolute)"""
    got, want = np.atleast_2d(np.asarray(got, dtype=np.float64)), np.atleast_2d(np.asarray(want, dtype=np.float64))
    peak = np.abs(want).max(axis=-1)
    return float((np.abs(got - want).max(axis=-1) / np.where(peak > 0, peak, 1.0)).max())
