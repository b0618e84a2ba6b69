"""fp64 numpy restatement of the loudness meter (include/t2vae.h, csrc/loudness.hip): the K-weighting of ITU-R BS.1770-4 as
libebur128 and pyloudnorm derive it, 400 ms blocks with a 100 ms hop, both gates, pooling over rows, the K-weighted level on
the front end's frame grid and the energy fields of the evaluation.  Written from the definitions with numpy only; the filter
is a direct-form loop (scipy.signal.lfilter, where installed, is what the tests compare it with)."""
import math

import numpy as np

OFFSET = -0.691
ABS_GATE = -70.0
HOP = 256

# ITU-R BS.1770-4, table 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high pass (numerator 1 -2 1)
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)


def coefficients(sr):
    """(b0, b1, b2, a1, a2, d1, d2) in fp64 for the rate sr"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
         2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.array(c + [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def coefficients_f32(sr):
    """the coefficients as the kernel gets them: rounded to fp32, as fp64 numbers"""
    return coefficients(sr).astype(np.float32).astype(np.float64)


def biquad(b, a, x):
    """direct form I loop in fp64: y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2], zero initial state"""
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    x1 = x2 = y1 = y2 = 0.0
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    for i in range(len(x)):
        xi = float(x[i])
        yi = b0 * xi + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xi, y1, yi
        y[i] = yi
    return y


def kweight(x, coef, use_lfilter=True):
    """the K-weighted signal of x (fp64) under the seven coefficients"""
    b0, b1, b2, a1, a2, d1, d2 = (float(v) for v in coef)
    stages = (([b0, b1, b2], [1.0, a1, a2]), ([1.0, -2.0, 1.0], [1.0, d1, d2]))
    z = np.asarray(x, dtype=np.float64)
    if use_lfilter:
        try:
            from scipy.signal import lfilter
        except ImportError:
            lfilter = None
        if lfilter is not None:
            for b, a in stages:
                z = lfilter(b, a, z)
            return z
    for b, a in stages:
        z = biquad(b, a, z)
    return z


def lufs(power):
    return OFFSET + 10.0 * math.log10(power) if power > 0.0 else float('-inf')


def block_powers(z, sr):
    """mean squares of the complete 400 ms blocks at a 100 ms hop"""
    hop = sr // 10
    blk = 4 * hop
    n = len(z)
    nb = (n - blk) // hop + 1 if n >= blk else 0
    c = np.concatenate([[0.0], np.cumsum(z * z)])
    return np.array([(c[j * hop + blk] - c[j * hop]) / blk for j in range(nb)], dtype=np.float64)


def gate(powers):
    """(gated sum, gated count, absolute-gate margin dB, relative-gate margin dB): the margins are the distance of the nearest
    block level to each gate (inf without blocks)"""
    powers = np.asarray(powers, dtype=np.float64)
    lv = np.array([lufs(p) for p in powers])
    above = lv > ABS_GATE
    m_abs = float(np.min(np.abs(lv - ABS_GATE))) if len(lv) else float('inf')
    if not above.any():
        return 0.0, 0, m_abs, float('inf')
    rel = lufs(float(powers[above].mean())) - 10.0
    keep = above & (lv > rel)
    return float(powers[keep].sum()), int(keep.sum()), m_abs, float(np.min(np.abs(lv - rel)))


def frame_ms(z, n=None):
    """mean square over [256 t - 512, 256 t + 512) for the n // 256 + 1 frames, zeros outside [0, n)"""
    n = len(z) if n is None else n
    frames = n // HOP + 1
    c = np.concatenate([[0.0], np.cumsum(np.asarray(z[:n], dtype=np.float64) ** 2)])
    out = np.zeros(frames)
    for t in range(frames):
        lo, hi = max(HOP * t - 512, 0), min(HOP * t + 512, n)
        out[t] = (c[hi] - c[lo]) / 1024.0 if hi > lo else 0.0
    return out


def energy_db(ms):
    return OFFSET + 10.0 * np.log10(np.maximum(np.asarray(ms, dtype=np.float64), 1e-12))


def measure(x, sr, coef=None):
    """everything the meter gives for one row x, as a dict"""
    coef = coefficients_f32(sr) if coef is None else coef
    x = np.asarray(x, dtype=np.float64)
    z = kweight(x, coef)
    bp = block_powers(z, sr)
    gsum, gcount, m_abs, m_rel = gate(bp)
    return dict(integrated=lufs(gsum / gcount) if gcount else float('-inf'), ungated=lufs(float(np.mean(z * z))),
                momentary_max=lufs(float(bp.max())) if len(bp) else float('-inf'), gated_sum=gsum, gated_blocks=gcount,
                n_blocks=len(bp), block_powers=bp, frame_ms=frame_ms(z), margin_abs=m_abs, margin_rel=m_rel)


def pooled(sums, counts):
    """loudness of several rows together from their gated sums and counts (the relative gate stays per row)"""
    c = sum(counts)
    return lufs(sum(sums) / c) if c else float('-inf')


def sounding(db, floor_db=40.0):
    db = np.asarray(db, dtype=np.float64)
    return db > db.max() - floor_db


def spread_db(db, floor_db=40.0):
    """standard deviation of the frame level over the frames within floor_db of the loudest"""
    db = np.asarray(db, dtype=np.float64)
    return float(np.std(db[sounding(db, floor_db)]))


def path_energy(db_x, db_y, path, floor_db=40.0):
    """(rmse dB, Pearson correlation) of two dB tracks along the path points where both sides sound; None where undefined"""
    db_x, db_y = np.asarray(db_x, dtype=np.float64), np.asarray(db_y, dtype=np.float64)
    path = np.asarray(path)
    sx, sy = sounding(db_x, floor_db), sounding(db_y, floor_db)
    i, j = path[:, 0], path[:, 1]
    keep = sx[i] & sy[j]
    if not keep.any():
        return None, None
    a, b = db_x[i[keep]], db_y[j[keep]]
    rmse = float(np.sqrt(np.mean((a - b) ** 2)))
    da, db_ = a - a.mean(), b - b.mean()
    den = math.sqrt(float((da * da).sum()) * float((db_ * db_).sum()))
    return rmse, (float((da * db_).sum()) / den if den > 0.0 else None)


def gating_signal(sr, seed=0):
    """6 s of noise bursts of amplitude 0.3, 0.05 and 0.5 with 1e-4 noise between them"""
    rng = np.random.RandomState(seed)
    x = 1e-4 * rng.randn(6 * sr)
    for (t0, t1), amp in (((0.5, 1.7), 0.3), ((2.2, 3.4), 0.05), ((4.0, 5.5), 0.5)):
        a, b = int(t0 * sr), int(t1 * sr)
        x[a:b] = amp * rng.randn(b - a)
    return x
