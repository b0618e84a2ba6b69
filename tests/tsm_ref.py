"""fp64 numpy restatement of the phase vocoder (include/t2vae.h, csrc/tsm.hip): the core, identity phase locking and the
lengths; `time_stretch` on numpy's FFT (the framing of vocoder_ref); and a tone-frequency estimator for the end-to-end
tests."""
import numpy as np

import vocoder_ref as V

BINS = 513
HOP = 256


def out_frames(n, num, den):
    """ceil(n den / num)"""
    return -((-int(n) * den) // num)


def out_samples(n_samples, num, den):
    """what time_stretch keeps of a row of n_samples: min((T_out - 1) 256, ceil(n_samples den / num))"""
    t_out = out_frames(n_samples // HOP + 1, num, den)
    return min((t_out - 1) * HOP, out_frames(n_samples, num, den))


def positions(n, num, den):
    """(i, a) of every output frame of a row of n frames: i = (j num) // den, a = ((j num) % den) / den"""
    p = np.arange(out_frames(n, num, den), dtype=np.int64) * num
    return p // den, (p % den) / float(den)


def peaks(m):
    """m (513,): bins strictly greater than their neighbours at distance 1 and 2 (those that exist)"""
    pk = np.ones(BINS, dtype=bool)
    for d in (1, 2):
        pk[d:] &= m[d:] > m[:-d]
        pk[:-d] &= m[:-d] > m[d:]
    return pk


def nearest_peak(pk):
    """for every bin the index of its nearest peak, the lower one on a tie; None when there is no peak"""
    idx = np.flatnonzero(pk)
    if idx.size == 0:
        return None
    k = np.arange(BINS)
    r = np.searchsorted(idx, k)                       # idx[r - 1] < k <= idx[r]
    lo = idx[np.clip(r - 1, 0, idx.size - 1)]
    hi = idx[np.clip(r, 0, idx.size - 1)]
    lo = np.where(r == 0, hi, lo)
    hi = np.where(r == idx.size, lo, hi)
    return np.where(np.abs(k - lo) <= np.abs(hi - k), lo, hi)


def phase_vocoder_row(mag, phase, num, den, phase_lock=False):
    """mag, phase (513, n): one row's frames.  Returns (mag_out, phase_out) (513, n_out) in fp64; phase_out is the full sum in
    radians (compare modulo 2 pi)."""
    mag, phase = np.asarray(mag, dtype=np.float64), np.asarray(phase, dtype=np.float64)
    n = mag.shape[1]
    i, a = positions(n, num, den)
    end = i + 1 >= n
    nxt = np.minimum(i + 1, n - 1)
    m1 = np.where(end[None, :], 0.0, mag[:, nxt])
    mag_out = (1.0 - a)[None, :] * mag[:, i] + a[None, :] * m1
    expect = (np.pi / 2.0) * np.arange(BINS, dtype=np.float64)[:, None]
    d = phase[:, nxt] - phase[:, i] - expect
    d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi)) + expect
    d = np.where(end[None, :], expect, d)
    acc = phase[:, :1] + np.concatenate([np.zeros((BINS, 1)), np.cumsum(d, axis=1)[:, :-1]], axis=1)
    if not phase_lock:
        return mag_out, acc
    out = acc.copy()
    cache = {}
    for j, fi in enumerate(i.tolist()):
        if fi not in cache:
            cache[fi] = nearest_peak(peaks(mag[:, fi]))
        kp = cache[fi]
        if kp is not None:
            out[:, j] = acc[kp, j] + phase[:, fi] - phase[kp, fi]
    return mag_out, out


def phase_distance(a, b):
    """|a - b| modulo 2 pi, in [0, pi]"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(d - 2.0 * np.pi * np.round(d / (2.0 * np.pi)))


def time_stretch(y, num, den, phase_lock=False):
    """(N,) -> the stretched waveform in fp64, out_samples(N, num, den) samples: stft, phase_vocoder_row, istft"""
    y = np.asarray(y, dtype=np.float64)
    spec = V.stft(y)
    m, p = phase_vocoder_row(np.abs(spec), np.angle(spec), num, den, phase_lock)
    out = V.istft(m * np.exp(1j * p))
    return out[:out_samples(len(y), num, den)]


def tone_frequency(y, sr):
    """Frequency of the strongest sinusoid of y in Hz: the peak of the Hann-windowed FFT of the middle half of the signal,
    refined by a parabola through the log magnitudes of the peak bin and its neighbours.  Returns (Hz, bin spacing in Hz)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y) // 2
    seg = y[len(y) // 4:len(y) // 4 + n]
    spec = np.abs(np.fft.rfft(seg * np.hanning(n)))
    k = int(np.argmax(spec[1:-1])) + 1
    la, lb, lc = np.log(np.maximum(spec[k - 1:k + 2], 1e-300))
    shift = 0.5 * (la - lc) / (la - 2.0 * lb + lc)
    return (k + shift) * sr / float(n), sr / float(n)
