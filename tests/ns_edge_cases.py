"""Named, seeded, deterministic signals that take the branches of the NoiseSup frame loop, its feature chain and the
16 k-native variant which the speech-like corpus (harmonics at 3000, uniform noise in +-700) never takes: the quiet-signal
clamps, the noise-estimate floors, the SNR jump in the first ten frames, the acceleration latch, PostProc's middle weight,
the raised hang-over, WaveProc without a maximum.  Data only: tests/test_edge_coverage_cpu.py measures which branches of
oracle/ns_oracle.c and oracle/ns16k_oracle.c they take (tools/oracle_coverage.py), tests/test_oracle.py pins the
restatement to the reference on them, tests/test_gpu_edge_inputs.py runs the kernels on them.

Every length is the shortest (in the steps that were searched, see each line) at which the signal still takes the
branches it is there for; the whole 8 kHz set is below 400 000 samples.

signals_wb() is the wideband (16 kHz) set: four signals carried over from the 8 kHz recipes and the wideband edge set, whose
branches are those of the reference's own wideband code (tools/wb_oracle_coverage.py, tests/test_wb_edge_coverage_cpu.py);
below 800 000 samples.  tests/wb_edge_cuts.py records where the time-slice tests cut it."""
import collections

import numpy as np

HOP = 80


def _rng(seed):
    return np.random.default_rng(seed)


def _i16(v):
    return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)


def _tone(n, freq, amp, rate=8000.0):
    return amp * np.sin(2 * np.pi * freq * np.arange(n) / rate)


def _utt(seed, n):
    from speech_enhancement_amd import corpus
    return corpus.synth_utterance(seed, n)


# ---- 8 kHz, int16 --------------------------------------------------------------------------------------------------
# The lengths were searched with tools/oracle_coverage.py --only NAME in the steps each line names.
def uniform_pm2(n=HOP * 20):
    """uniform integers in +-2: ns_vad's meanEn clamped to its floor of 80 (reached from 8 frames on; 8 / 12 / 20 / 40 tried,
    20 kept so that cepstral frames exist); WaveProc's energy bypass on every frame"""
    return _rng(1).integers(-2, 3, n).astype(np.int16)


def uniform_pm12(n=HOP * 60):
    """uniform integers in +-12: takes no branch of its own -- a stationary signal two decades below the corpus' noise
    floor, kept as the neighbour of uniform_pm2 (denoised to a few units: logE just above PostProc's 275/64)"""
    return _rng(2).integers(-12, 13, n).astype(np.int16)


def sparse_ones(n=HOP * 20):
    """a 1 every 97th sample: frames of one or no non-zero sample behind an open gate; the meanEn floor again, with a frame
    energy of exactly 64 or 65 (8 / 12 / 20 tried)"""
    x = np.zeros(n, np.int16)
    x[::97] = 1
    return x


def onset_tone(n=HOP * 100):
    """noise of sigma 15, a 20 000-amplitude tone switched on at sample 480 and a second burst at frame 80: SNR jump >= 10 dB
    while nbFrame[1] < 10 (ns_gain_fact), acceleration > 2.5 latches fdSpeechInVADQ and the latched path after it
    (speech_q_spec), trigger >= 4 before frame 35 raises the VAD hang-over to 50 (vad_decide), waveproc without a maximum,
    PostProc's middle weight (100 = the second burst plus five frames; 120 adds nothing)"""
    x = _rng(3).standard_normal(n) * 15.0
    x[480:480 + HOP * 30] += _tone(HOP * 30, 1000.0, 20000.0)
    x[HOP * 80:HOP * 95] += _tone(HOP * 15, 700.0, 20000.0)
    return _i16(x)


def loud_then_zeros(n_loud=HOP * 60, n_zero=12000):
    """a loud (clipped) utterance followed by 12 000 zeros: meanEn falls to its floor from above, the noise estimates fall
    through many decades, waveproc's `nom <= 1` (20+4000 does not reach the meanEn floor; 40+8000 and 60+12000 do)"""
    loud = np.clip(_utt(6, n_loud).astype(np.int32) * 6, -32768, 32767).astype(np.int16)
    return np.concatenate([loud, np.zeros(n_zero, np.int16)])


def square_fullscale(n=HOP * 30):
    """full-scale square wave of period 16: takes no branch of its own -- the largest values every sum of the frame loop can
    hold, the int16 cast at its limits"""
    return np.where((np.arange(n) // 8) % 2 == 0, 32767, -32768).astype(np.int16)


def dc_fullscale(n=HOP * 30):
    """full-scale DC: takes no branch of its own -- all energy in bin 0, the DC-offset filter's longest transient"""
    return np.full(n, 32767, np.int16)


def nyquist_fullscale(n=HOP * 30):
    """full-scale alternating samples: takes no branch of its own -- all energy in the last bin, the others at rounding level"""
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


def square4_burst(n=HOP * 60):
    """noise of sigma 15 with a full-scale square wave of period 4 from sample 840 to 2440: every Teager value of the burst is
    2 d^2, the 9-point int32 sums wrap negative, and a maximum next to the burst finds no neighbour 25..79 samples away --
    waveproc's four `&& found` exits (both loops); speech found by SpeechFoundVADNS alone (vad_proc).  Start 800 / 820 /
    840 / 860 and the four phases tried: 840 with the wave starting on its second sample takes all four exits."""
    x = _rng(8).standard_normal(n) * 15.0
    k = np.arange(840, 2440)
    x[840:2440] += np.where(((k + 1) // 2) % 2 == 0, 32767.0, -32767.0)
    return _i16(x)


def low_tone_in_noise(n=HOP * 80):
    """noise of sigma 300 with a 120 Hz tone of amplitude 300 on frames 30..49: speech found by the mel measure (gains of
    bands 1..3) alone (vad_proc).  120 / 200 / 300 Hz at 0.5 / 1 / 2 / 4 times sigma tried: 120 Hz at 1 gives most frames."""
    x = _rng(9).standard_normal(n) * 300.0
    x[HOP * 30:HOP * 50] += _tone(HOP * 20, 120.0, 300.0)
    return _i16(x)


def utt_gap_utt(n_utt=HOP * 100, n_gap=24000):
    """a corpus utterance, 24 000 zeros, the utterance again: the second stage's noise estimate reaches eps (ns_filter_calc)
    and the trackers come back up from their floors (40+8000 and 60+16000 do not reach the floor)"""
    u = _utt(9, n_utt)
    return np.concatenate([u, np.zeros(n_gap, np.int16), u])


def exp_ramp(n=HOP * 50):
    """noise under an exponential ramp over 9 nepers up to full scale: meanEn leaves its floor, the acceleration latch and the
    raised hang-over without an onset (50 / 100 / 150 frames tried: the steepest takes most)"""
    t = np.arange(n) / float(n)
    return _i16(_rng(4).uniform(-1.0, 1.0, n) * 32000.0 * np.exp(9.0 * (t - 1.0)))


def exp_fade(n=HOP * 150):
    """noise under an exponential fade over 12 nepers from full scale, ending in samples of 0 and +-1: averSNR <= 1e-5
    (the 16 k-native gain_fact16), meanEn down to its floor (reached at 150 frames, not at 50 / 100)"""
    t = np.arange(n) / float(n)
    return _i16(_rng(5).uniform(-1.0, 1.0, n) * 32000.0 * np.exp(-12.0 * t))


def ones_then_zeros(n_noise=HOP * 10, n_zero=HOP * 1020):
    """ten frames of +-1 noise followed by 1020 all-zero frames: the noise estimate of both stages decays to eps = e^-10 and
    is clamped there (ns_filter_calc: the second stage from 200 zero frames on, the first between 1000 and 1020, searched in
    steps of 20), logE below CompCeps' floor e^-50"""
    return np.concatenate([_rng(6).integers(-1, 2, n_noise).astype(np.int16), np.zeros(n_zero, np.int16)])


_SIGNALS_8K = (uniform_pm2, uniform_pm12, sparse_ones, onset_tone, loud_then_zeros, square_fullscale, dc_fullscale,
               nyquist_fullscale, square4_burst, low_tone_in_noise, utt_gap_utt, exp_ramp, exp_fade, ones_then_zeros)


def signals_8k():
    """name -> int16 signal, in a fixed order"""
    return collections.OrderedDict((f.__name__, f()) for f in _SIGNALS_8K)


# ---- 16 k-native variant: float frames of 160 samples ---------------------------------------------------------------
# func_Wiener skips every frame whose (int) sum of squares is 0 without touching its state, so a run of zeros never
# lets the noise estimate decay there: the floors need frames that pass the gate with almost nothing in most bins.
def dc_rise_small(n=160 * 60):
    """16 k: a raised-cosine rise over one frame to a DC of 0.2 (frame energy 2.4 .. 6.4, the gate passes): nothing but
    rounding noise above the lowest bins -- both floors of filter_calc16 (the first stage at once, the second from frame 56;
    44 .. 60 in steps of 4 tried)"""
    x = np.full(n, 0.2)
    x[:160] = 0.1 * (1.0 - np.cos(np.pi * np.arange(160) / 160.0))
    return x.astype(np.float32)


def sub_integer_noise(n=160 * 60):
    """16 k: Gaussian noise of sigma 0.3 (frame energy about 14): the whole loop below integer amplitudes"""
    return (_rng(7).standard_normal(n) * 0.3).astype(np.float32)


def exp_fade_float(n=160 * 150):
    """16 k: the 12-neper fade without the rounding to integers, down to amplitude 0.2 and frames the gate drops one by one"""
    t = np.arange(n) / float(n)
    return (_rng(5).uniform(-1.0, 1.0, n) * 32000.0 * np.exp(-12.0 * t)).astype(np.float32)


def onset_tone_milli(n=160 * 50):
    """16 k: onset_tone scaled by 0.004 -- noise whose frames the gate drops, then a tone of amplitude 80: the first frames
    the loop ever sees are the onset"""
    return (onset_tone(n).astype(np.float32) * np.float32(0.004)).astype(np.float32)


def streams_16k():
    """name -> float32 signal (a whole number of 160-sample frames): the 8 kHz signals as floats (all but the 1030-frame
    ones_then_zeros, whose zero frames the gate of this variant drops) and the four float-only ones"""
    s = collections.OrderedDict()
    for name, x in signals_8k().items():
        if name != "ones_then_zeros":
            s[name] = x[: len(x) // 160 * 160].astype(np.float32)
    for f in (dc_rise_small, sub_integer_noise, exp_fade_float, onset_tone_milli):
        s[f.__name__] = f()
    return s


# ---- wideband (16 kHz int16) mode: the quiet, onset, loud-then-zero and fade signals at 16 kHz -----------------------------
WB_CARRIED = ("uniform_pm2", "onset_tone", "loud_then_zeros", "exp_fade")   # the four carried over from the 8 kHz recipes


def signals_wb():
    """name -> int16 signal at 16 kHz: the same recipes with twice the samples per unit of time, then the wideband edge set"""
    s = collections.OrderedDict([("uniform_pm2", uniform_pm2(160 * 20)), ("onset_tone", _onset_tone_wb()),
                                 ("loud_then_zeros", _loud_then_zeros_wb()), ("exp_fade", exp_fade(160 * 150))])
    for f in _SIGNALS_WB:
        s[f.__name__] = f()
    return s


def _onset_tone_wb(n=160 * 100):
    x = _rng(3).standard_normal(n) * 15.0
    x[960:960 + 160 * 30] += _tone(160 * 30, 1000.0, 20000.0, 16000.0) + _tone(160 * 30, 5500.0, 6000.0, 16000.0)
    x[160 * 80:160 * 95] += _tone(160 * 15, 700.0, 20000.0, 16000.0)
    return _i16(x)


def _loud_then_zeros_wb():
    from speech_enhancement_amd import corpus
    loud = np.clip(corpus.synth_wideband(6, 160 * 60).astype(np.int32) * 8, -32768, 32767).astype(np.int16)
    return np.concatenate([loud, np.zeros(24000, np.int16)])


# ---- the wideband edge set --------------------------------------------------------------------------------------------------
# What the REFERENCE's own wideband code needs beyond the four above and the other inputs of the wideband GPU tests: branches
# are named by the reference's file, function and line, as tools/wb_oracle_coverage.py reports them.  The lengths and first
# frames were found with that tool's --only NAME and --first FILE:LINE (a bisection over prefixes of the signal).
WB_HOP = 160


def ones_then_zeros_wb(n_noise=WB_HOP * 10, n_zero=WB_HOP * 1500):
    """ten frames of +-1 noise, 1500 all-zero frames, ten frames of +-1 noise again: FilterCalc's two noise-estimate floors on
    the QMF low band (NoiseSup.c:515 first taken at frame 114, :543 at frame 450) and the high band's noise estimate clamped
    at its floor in DoSpecSub16k (16kHzProcessing.c:461, first at frame 1373: the estimate loses 1 % per frame from the level
    the ten noise frames left).  1020 zero frames do not reach the high band's clamp, 1500 do; bisected to 1374 frames in all.
    An all-zero frame gives high-band rows of 0 whatever the estimate holds, so the clamp shows only in what follows: the
    zeros go on to frame 1510, where the estimate without its clamp would stand at 0.25 of the floor, and the closing noise
    (WB_TAIL_START) subtracts 1.5 times the estimate from band energies of about a hundred."""
    rng = _rng(6)
    head, tail = rng.integers(-1, 2, n_noise).astype(np.int16), rng.integers(-1, 2, n_noise).astype(np.int16)
    return np.concatenate([head, np.zeros(n_zero, np.int16), tail])


WB_TAIL_START = 1510       # the frame at which ones_then_zeros_wb's closing noise begins


def square8_burst_wb(n=WB_HOP * 40, start=1680):
    """noise of sigma 15 with a full-scale square wave of period 8 (period 4 in the QMF low band) from sample 1680 to 4880:
    GetMaximaPositions' search that finds no neighbouring maximum, to the right and to the left (WaveProc.c:145 / :155 first
    at frame 16, :130 / :140 at frame 34), and speech found by SpeechFoundVADNS alone (VAD.c:249, first at frame 17).  Periods
    4 / 8 / 16, starts 1680 / 1700 / 1720 / 1760 and both phases tried: only period 8 at 1680 or 1760 gives frames with the
    last measure alone, 1680 kept; 35 frames are needed, 40 kept."""
    x = _rng(8).standard_normal(n) * 15.0
    k = np.arange(start, start + 3200)
    x[start:start + 3200] += np.where((k // 4) % 2 == 0, 32767.0, -32767.0)
    return _i16(x)


def low_tone_after_burst_wb(n=WB_HOP * 56):
    """noise of sigma 300, a Hann-shaped 1500 Hz tone of amplitude 300 on frames 2..11 and a 120 Hz tone of amplitude 300 on
    frames 30..49: speech found by SpeechFoundMel alone (VAD.c:249, first at frame 34).  The 8 kHz recipe without the early
    tone never gives it at 16 kHz (80 / 120 / 200 / 300 Hz at 0.12 .. 4 times sigma tried: the three measures fire together or
    not at all): the early tone, while the frame counter is below 15, lifts the running maxima of the spectral and the
    variance measure but not that of mel bands 1..3, so the later low tone passes the mel measure only.  Early tone at 1000 /
    1500 Hz with amplitude 300 / 1000 / 3000 and the low tone at 0.25 / 0.5 / 1 times sigma tried: 1500 Hz at 300 with 1 gives
    nine such frames, the louder early tones none."""
    x = _rng(9).standard_normal(n) * 300.0
    x[WB_HOP * 2:WB_HOP * 12] += np.hanning(WB_HOP * 10) * _tone(WB_HOP * 10, 1500.0, 300.0, 16000.0)
    x[WB_HOP * 30:WB_HOP * 50] += _tone(WB_HOP * 20, 120.0, 300.0, 16000.0)
    return _i16(x)


def short_onset_wb(n=WB_HOP * 12):
    """noise of sigma 15 and a 20 000-amplitude 1000 Hz tone from sample 960 to the end of a 12-frame utterance: the ring of
    seven still holds four speech frames in a row when DoVADFlush runs with the frame counter at 35 or less, so the flush
    raises the hang-over (VAD.c:394).  20 frames tried first; bisected to 11, 12 kept."""
    x = _rng(3).standard_normal(n) * 15.0
    x[960:] += _tone(n - 960, 1000.0, 20000.0, 16000.0)
    return _i16(x)


_SIGNALS_WB = (ones_then_zeros_wb, square8_burst_wb, low_tone_after_burst_wb, short_onset_wb)
