"""fp64 numpy restatement of the pitch tracker's measure (include/t2vae.h, csrc/f0.hip): YIN steps 1-5 at 16 kHz, hop 256,
integration window 1024.  The GPU tests compare t2v_hip.f0 with it; tests/test_prosody.py checks it on steady tones.

Frame t of a waveform of n samples (n // 256 + 1 frames, samples outside [0, n) count as 0), s = 256 t - 512:
    d(tau)  = sum_{j<1024} (x[s+j] - x[s+j+tau])^2, tau = 1..tau_max
    d'(tau) = d(tau) tau / sum_{k<=tau} d(k), 1 where that sum is 0
    tau*    = the smallest tau in [tau_min, tau_max] with d' < threshold, then tau + 1 while d'(tau + 1) < d'(tau)
    f0      = 16000 / (tau* + delta), delta = clamp(0.5 (a - c) / (a - 2b + c), -1, 1) for a, b, c = d'(tau* - 1 .. tau* + 1)
              when both neighbours lie in 1..tau_max and a - 2b + c > 0, else 0
"""
import math

import numpy as np

SR, HOP, W = 16000, 256, 1024


def lags(fmin=60.0, fmax=500.0):
    return int(math.floor(SR / fmax)), int(math.ceil(SR / fmin))


def n_frames(n):
    return n // HOP + 1


def yin(x, fmin=60.0, fmax=500.0, threshold=0.1):
    """x: 1-D waveform.  Returns a dict of per-frame arrays: f0 (Hz, 0 unvoiced), aperiodicity (d' at tau*, 1 unvoiced),
    tau (tau*, 0 unvoiced), a, b, c (NaN where the frame is unvoiced or a neighbour lies outside 1..tau_max), den
    (a - 2b + c), margin (how far the frame's decisions are from flipping: the smallest |d'(tau) - threshold| over
    tau_min..tau_max and the smallest |d'(tau + 1) - d'(tau)| met in the descent, its stopping step included)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    tau_min, tau_max = lags(fmin, fmax)
    T = n_frames(n)
    pad_l = 2 * HOP
    xp = np.zeros(pad_l + HOP * (T - 1) + 2 * HOP + tau_max + 1)
    xp[pad_l:pad_l + n] = x
    out = {k: np.full(T, v) for k, v in (('f0', 0.0), ('aperiodicity', 1.0), ('a', np.nan), ('b', np.nan), ('c', np.nan),
                                         ('den', np.nan), ('margin', np.inf))}
    out['tau'] = np.zeros(T, dtype=np.int64)
    for t in range(T):
        seg = xp[HOP * t:HOP * t + W + tau_max]                 # x[s .. s + W + tau_max), s = 256 t - 512
        shifted = np.lib.stride_tricks.sliding_window_view(seg, W)[1:tau_max + 1]
        d = np.concatenate([[0.0], ((seg[:W] - shifted) ** 2).sum(axis=1)])       # d[tau], d[0] unused
        cum = np.cumsum(d)
        dp = np.ones(tau_max + 1)
        nz = cum > 0
        dp[nz] = d[nz] * np.arange(tau_max + 1)[nz] / cum[nz]
        dp[0] = np.nan
        margin = np.abs(dp[tau_min:tau_max + 1] - threshold).min()
        below = np.nonzero(dp[tau_min:tau_max + 1] < threshold)[0]
        if below.size:
            tau = tau_min + int(below[0])
            while tau + 1 <= tau_max:
                margin = min(margin, abs(dp[tau + 1] - dp[tau]))
                if not dp[tau + 1] < dp[tau]:
                    break
                tau += 1
            delta = 0.0
            if tau - 1 >= 1 and tau + 1 <= tau_max:
                a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
                den = a - 2.0 * b + c
                out['a'][t], out['b'][t], out['c'][t], out['den'][t] = a, b, c, den
                if den > 0:
                    delta = min(max(0.5 * (a - c) / den, -1.0), 1.0)
            out['tau'][t] = tau
            out['f0'][t] = SR / (tau + delta)
            out['aperiodicity'][t] = dp[tau]
        out['margin'][t] = margin
    return out


def harmonic_tone(freq, n, harmonics=5, decay=0.6, amp=0.3, phase_seed=0):
    """a steady tone: `harmonics` partials of amplitude decay^k at random phases"""
    rs = np.random.RandomState(phase_seed)
    t = np.arange(n) / SR
    y = np.zeros(n)
    for k in range(1, harmonics + 1):
        y += decay ** (k - 1) * np.sin(2 * np.pi * k * freq * t + rs.uniform(0, 2 * np.pi))
    return amp * y / np.abs(y).max()


def glide_signal(n, seed):
    """the GPU tests' waveform: a 110 -> 330 -> 110 Hz glide f(t) = 110 + 220 (0.5 - 0.5 cos(2 pi t / duration)) of six
    harmonics of amplitude 0.6^k at random phases, scaled by 0.2, plus noise of sigma 0.003; 3000 samples of exact zeros from
    n / 6 and 3000 samples of noise alone (sigma 0.05) from n / 2 (both cut to the signal)."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / SR
    dur = n / SR
    f = 110.0 + 220.0 * (0.5 - 0.5 * np.cos(2 * np.pi * t / dur))
    phase = 2 * np.pi * np.cumsum(f) / SR
    y = np.zeros(n)
    for k in range(1, 7):
        y += 0.6 ** k * np.sin(k * phase + rs.uniform(0, 2 * np.pi))
    y = 0.2 * y + 0.003 * rs.randn(n)
    z0, z1 = n // 6, min(n, n // 6 + 3000)
    y[z0:z1] = 0.0
    q0, q1 = n // 2, min(n, n // 2 + 3000)
    y[q0:q1] = 0.05 * rs.randn(q1 - q0)
    return y.astype(np.float32)
