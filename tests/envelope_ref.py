"""fp64 numpy restatement of the spectral envelope (include/t2vae.h, csrc/envelope.hip): the true-envelope iteration on a
cepstral lifter, the warp of a spectrum's envelope, `formant_shift` and the formant-preserving `pitch_shift` on the framing of
vocoder_ref, the phase vocoder of tsm_ref and the filter of resample_ref; the same envelope in float32 on scipy.fft, the
yardstick of the device tolerance; a synthetic vowel, a distance between the envelopes of two signals and an F0 estimator."""
import fractions

import numpy as np
import scipy.fft
import scipy.signal

import resample_ref as R
import tsm_ref as P
import vocoder_ref as V

BINS = 513
MAX_RATIO = 1023
FORMANTS = ((700.0, 80.0), (1200.0, 100.0), (2600.0, 140.0))      # the vowel's resonances: (centre, bandwidth) in Hz


def ratio(semitones):
    """(p, q) with p / q = 2^(semitones / 12), both in 1..1023: t2v_hip.pitch_ratio"""
    f = fractions.Fraction(2.0 ** (float(semitones) / 12.0))
    g = f.limit_denominator(MAX_RATIO)
    if g.numerator > MAX_RATIO:
        g = 1 / (1 / f).limit_denominator(MAX_RATIO)
    return g.numerator, g.denominator


def log_floor(mag):
    """(513, n) fp32 magnitudes -> (n,) fp32: max(1e-7f max_k m[k], 1e-10f), the product in fp32"""
    mag = np.asarray(mag, dtype=np.float32)
    return np.maximum(np.float32(1e-7) * mag.max(axis=0), np.float32(1e-10)).astype(np.float32)


def _lifter(x, order, rfft):
    """x (513, n): the columns even-extended to 1024 points, DFT / 1024, cepstral bins above `order` zeroed, DFT, real part"""
    full = np.concatenate([x, x[-2:0:-1]], axis=0)                  # x[1024 - k] = x[k]
    c = rfft(full, axis=0).real / x.dtype.type(1024.0)
    c[order + 1:] = 0
    return rfft(np.concatenate([c, c[-2:0:-1]], axis=0), axis=0).real


def _log_envelope(mag, order, iters, dtype, rfft):
    mag = np.asarray(mag, dtype=np.float32)
    if mag.ndim != 2 or mag.shape[0] != BINS or not 1 <= order <= 256 or not 0 <= iters <= 32:
        raise ValueError("log_envelope: (513, n) magnitudes, order in 1..256, iters in 0..32")
    L = np.log(np.maximum(mag, log_floor(mag)[None, :]).astype(dtype))
    A = L
    for _ in range(iters + 1):
        E = _lifter(A, order, rfft).astype(dtype)
        A = np.maximum(L, E)
    return E


def log_envelope(mag, order=32, iters=8):
    """(513, n) fp32 magnitudes -> the natural-log true envelope (513, n) in fp64; the floor is the kernel's fp32 floor"""
    return _log_envelope(mag, order, iters, np.float64, np.fft.rfft)


def log_envelope32(mag, order=32, iters=8):
    """the same algorithm in float32 throughout, on scipy.fft (which keeps single precision)"""
    E = _log_envelope(mag, order, iters, np.float32, scipy.fft.rfft)
    assert E.dtype == np.float32
    return E


def positions(p, q):
    """(i, a) of every bin: i = (k p) // q, a = ((k p) % q) / q"""
    pos = np.arange(BINS, dtype=np.int64) * p
    return pos // q, (pos % q) / float(q)


def warp_log_envelope(E, p, q):
    """Ew[k] = (1 - a) E[i] + a E[i + 1]; E[512] for i >= 512"""
    E = np.asarray(E, dtype=np.float64)
    i, a = positions(p, q)
    lo, hi = np.minimum(i, BINS - 1), np.minimum(i + 1, BINS - 1)
    Ew = (1.0 - a)[:, None] * E[lo] + a[:, None] * E[hi]
    return np.where((i >= BINS - 1)[:, None], E[BINS - 1][None, :], Ew)


def warp(mag, E, p, q):
    """mag (513, n), E its log envelope -> mag exp(Ew - E) in fp64; p == q is the identity"""
    mag = np.asarray(mag, dtype=np.float64)
    if p == q:
        return mag.copy()
    return mag * np.exp(warp_log_envelope(E, p, q) - np.asarray(E, dtype=np.float64))


def resample(x, sr_in, sr_out):
    """resample_ref's filter applied as scipy.signal.resample_poly does"""
    up, down, _, g = R.window(sr_in, sr_out)
    return scipy.signal.resample_poly(np.asarray(x, dtype=np.float64), up, down, window=g)


def formant_shift(y, semitones, order=32, iters=8):
    """(N,) -> ((N // 256) 256,): the envelope moved up by 2^(semitones / 12), harmonics and phases kept"""
    p, q = ratio(semitones)
    y = np.asarray(y, dtype=np.float64)
    if p == q:
        return y
    spec = V.stft(y)
    mag = np.abs(spec)
    m = warp(mag, log_envelope(mag.astype(np.float32), order, iters), q, p)
    return V.istft(m * np.exp(1j * np.angle(spec)))


def pitch_shift(y, semitones, preserve=False, order=32, iters=8, phase_lock=True):
    """(N,) -> the shifted waveform: stft, the envelope warped by (p, q) when preserving, the phase vocoder at q / p, istft,
    the resampler p -> q"""
    p, q = ratio(semitones)
    y = np.asarray(y, dtype=np.float64)
    if p == q:
        return y
    spec = V.stft(y)
    mag, phase = np.abs(spec), np.angle(spec)
    if preserve:
        mag = warp(mag, log_envelope(mag.astype(np.float32), order, iters), p, q)
    m, ph = P.phase_vocoder_row(mag, phase, q, p, phase_lock)
    out = V.istft(m * np.exp(1j * ph))[:P.out_samples(len(y), q, p)]
    return resample(out, p, q)


def vowel(f0, seconds=1.0, sr=16000):
    """an impulse train at f0 through two-pole resonators at 700 / 1200 / 2600 Hz in cascade, peak 0.5, fp64"""
    n = int(round(seconds * sr))
    x = np.zeros(n)
    x[(np.arange(0.0, n, sr / float(f0))).astype(np.int64)] = 1.0
    for hz, bw in FORMANTS:
        r = np.exp(-np.pi * bw / sr)
        x = scipy.signal.lfilter([1.0], [1.0, -2.0 * r * np.cos(2.0 * np.pi * hz / sr), r * r], x)
    return 0.5 * x / np.abs(x).max()


def mean_log_envelope(y, order=24, iters=8):
    """(513,): the log envelope of y's frames, averaged over the middle half of the frames"""
    mag = np.abs(V.stft(np.asarray(y, dtype=np.float64))).astype(np.float32)
    T = mag.shape[1]
    return log_envelope(mag[:, T // 4:T // 4 + max(T // 2, 1)], order, iters).mean(axis=1)


def log_spectral_distance(ea, eb, lo=5, hi=400):
    """RMS over bins lo..hi-1 of the difference of two log envelopes with its mean removed, in dB"""
    d = (np.asarray(ea, dtype=np.float64) - np.asarray(eb, dtype=np.float64))[lo:hi]
    return float(np.sqrt(np.mean((d - d.mean()) ** 2)) * 20.0 / np.log(10.0))


def envelope_distance(y, z, order=24):
    """log-spectral distance in dB between the mean order-24, 8-iteration envelopes of two signals, bins 5..399"""
    return log_spectral_distance(mean_log_envelope(y, order), mean_log_envelope(z, order))


def moved_envelope(e, p, q):
    """(513,) log envelope moved up along frequency by p / q: read at k q / p"""
    return warp_log_envelope(np.asarray(e, dtype=np.float64)[:, None], q, p)[:, 0]


def f0_autocorrelation(y, sr=16000, lo=60.0, hi=400.0):
    """F0 in Hz: the lag of the highest peak of the autocorrelation of the middle half of y within sr / hi .. sr / lo"""
    y = np.asarray(y, dtype=np.float64)
    seg = y[len(y) // 4:len(y) // 4 + len(y) // 2]
    seg = seg - seg.mean()
    spec = np.fft.rfft(seg, 2 * len(seg))
    ac = np.fft.irfft(spec * np.conj(spec))[:len(seg)]
    a, b = int(sr / hi), int(sr / lo)
    return sr / float(a + int(np.argmax(ac[a:b + 1])))
