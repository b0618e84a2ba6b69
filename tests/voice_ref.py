"""fp64 numpy reference of t2v_voice_quality (include/t2vae.h), written from the definitions, and the test signals.

voice_quality(x) gives the six planes of one waveform, one value per frame of the front end's grid (frame t covers the samples
[256 t - 512, 256 t + 512), zeros outside the waveform, len(x) // 256 + 1 frames), and `lag_margin`, how far the cepstral peak
stands above the second-best quefrency, in dB.  With dtype=np.float32 the same arithmetic runs in single precision (numpy's
FFT included): the distance between the two is what the rounding of one fp32 implementation costs, and four times its largest
value per plane, over gpu_rows(), is the tolerance of the GPU tests (FP32_MAX below, profiles/voice_parity.txt)."""
import numpy as np

SR, HOP, WIN = 16000, 256, 1024
FEATS = ('level_db', 'alpha_db', 'hammarberg_db', 'slope_db_khz', 'cpp_db', 'cpp_lag')
SILENT_DB = -200.0
FRAMES_PER_WORKGROUP = 8             # T2V_VOICE_FRAMES: the lengths of gpu_rows() straddle a workgroup's tile
FLOOR_REL, CEP_FLOOR_REL, CEP_FLOOR_ABS = 1e-9, 1e-3, 1e-4
K_LO, K_MID, K_HAM, K_HI = 4, 64, 128, 320      # 50 Hz, 1 kHz, 2 kHz, 5 kHz in bins of 15.625 Hz
S0, S1 = 32, 96                                 # the slope's band, 500 .. 1500 Hz
Q0, QP, Q1 = 16, 32, 266                        # the regression's quefrencies; the peak's start at QP (500 .. 60 Hz)
COUNT_FLOOR_DB = 40.0

# The largest |fp32 arithmetic - fp64| per plane over the frames of gpu_rows() that are not silent, measured with
# measure_fp32() (numpy 2.2, whose FFT of float32 input runs in float32), rounded up to two digits.
FP32_MAX = {'level_db': 7.5e-6, 'alpha_db': 4.7e-6, 'hammarberg_db': 9.6e-6, 'slope_db_khz': 1.3e-5, 'cpp_db': 9.8e-5}
GPU_TOL = {k: 4.0 * v for k, v in FP32_MAX.items()}
LAG_EXEMPT_CAP = 0.02                # share of frames whose peak is closer to the second best than the cpp tolerance


def n_frames(n):
    return n // HOP + 1


def window():
    """the front end's periodic Hann window: fp64, rounded once to fp32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)).astype(np.float32)


def frames_of(x):
    x = np.asarray(x)
    T = n_frames(len(x))
    padded = np.zeros(512 + HOP * (T - 1) + 512, dtype=x.dtype)
    padded[512:512 + len(x)] = x
    return padded[HOP * np.arange(T)[:, None] + np.arange(WIN)[None, :]]


def voice_quality(x, dtype=np.float64):
    """the planes of FEATS and lag_margin as a dict of (frames,) arrays of `dtype`; x: 1-D float32 samples, at least one"""
    f = dtype
    xw = frames_of(np.asarray(x, dtype=np.float32)).astype(f) * window().astype(f)[None, :]
    X = np.fft.rfft(xw, axis=1)
    P = (X.real.astype(f) ** 2 + X.imag.astype(f) ** 2).astype(f)
    T = P.shape[0]
    mx = P.max(axis=1)
    silent = P.sum(axis=1) == 0
    fl = np.maximum(f(FLOOR_REL) * mx, f(np.finfo(np.float32).tiny))
    out = {k: np.zeros(T, dtype=f) for k in FEATS + ('lag_margin',)}
    with np.errstate(divide='ignore', invalid='ignore'):
        db = lambda v: f(10.0) * np.log10(v)
        out['level_db'] = db(np.maximum(P[:, K_LO:K_HI].sum(axis=1), fl))
        out['alpha_db'] = db(np.maximum(P[:, K_MID:K_HI].sum(axis=1), fl) / np.maximum(P[:, K_LO:K_MID].sum(axis=1), fl))
        out['hammarberg_db'] = db(np.maximum(P[:, :K_HAM].max(axis=1), fl) / np.maximum(P[:, K_HAM:K_HI].max(axis=1), fl))
        L = db(np.maximum(P, fl[:, None]))
        L = L - L.mean(axis=1, keepdims=True)           # neither the slope nor c[q >= 1] sees a constant
        kc = (np.arange(S0, S1 + 1) - (S0 + S1) // 2).astype(f)
        bin_khz = f(SR / WIN / 1000.0)
        out['slope_db_khz'] = (L[:, S0:S1 + 1] * kc[None, :]).sum(axis=1) / (f((kc ** 2).sum()) * bin_khz)
        c = np.fft.rfft(np.concatenate([L, L[:, 511:0:-1]], axis=1), axis=1).real.astype(f) / f(WIN)
        a = np.abs(c[:, Q0:Q1 + 1])
        cfl = np.maximum(f(CEP_FLOOR_REL) * a.max(axis=1), f(CEP_FLOOR_ABS))
        C = f(20.0) * np.log10(np.maximum(a, cfl[:, None]))
        qc = (np.arange(Q0, Q1 + 1) - (Q0 + Q1) // 2).astype(f)
        mean = C.mean(axis=1)
        slope = ((C - mean[:, None]) * qc[None, :]).sum(axis=1) / f((qc ** 2).sum())
        peak = C[:, QP - Q0:]
        at = peak.argmax(axis=1)                        # the first, so the lowest, of equals
        top = peak[np.arange(T), at]
        rest = peak.copy()
        rest[np.arange(T), at] = -np.inf
        out['cpp_db'] = top - (mean + slope * qc[QP - Q0 + at])
        out['cpp_lag'] = (QP + at).astype(f)
        out['lag_margin'] = top - rest.max(axis=1)
    for k in FEATS:
        out[k] = np.where(silent, f(SILENT_DB if k == 'level_db' else 0.0), out[k]).astype(f)
    out['lag_margin'] = np.where(silent, f(np.inf), out['lag_margin'])
    return out


def planes(x, dtype=np.float64):
    """(6, frames) in FEATS order"""
    r = voice_quality(x, dtype)
    return np.stack([r[k] for k in FEATS])


def counted(level_db):
    """one bool per frame: not silent and within COUNT_FLOOR_DB of the loudest frame (t2v_hip.voice_counted)"""
    level = np.asarray(level_db, dtype=np.float64)
    return (level > level.max() - COUNT_FLOOR_DB) & (level > SILENT_DB)


# ---------------------------------------------------------------------- signals
def tone(f0, n, power=1, snr_db=None, seed=0, fmax=7000.0, amp=0.3):
    """harmonics k f0 <= fmax of amplitude 1 / k^power at random phases, scaled so that the first has `amp`; white noise snr_db
    under the tone's power; float32"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / SR
    x = np.zeros(n)
    for k in range(1, int(fmax // f0) + 1):
        x += np.sin(2.0 * np.pi * k * f0 * t + rs.uniform(0.0, 2.0 * np.pi)) / k ** power
    if snr_db is not None:
        x += rs.randn(n) * np.sqrt(np.mean(x ** 2) if n > 1 else 0.5) * 10.0 ** (-snr_db / 20.0)
    return (amp * x).astype(np.float32)


def noise(n, seed=0, amp=0.1):
    return (amp * np.random.RandomState(seed).randn(n)).astype(np.float32)


def line_spectrum(f0, power=1, fmax=7000.0):
    """(alpha_db, hammarberg_db) of the tone's line spectrum: its harmonics' powers summed, and their peaks, per band"""
    k = np.arange(1, int(fmax // f0) + 1)
    f, p = k * f0, 1.0 / k.astype(np.float64) ** (2 * power)
    band = lambda lo, hi: p[(f >= lo) & (f < hi)]
    return (10.0 * np.log10(band(1000.0, 5000.0).sum() / band(50.0, 1000.0).sum()),
            10.0 * np.log10(band(0.0, 2000.0).max() / band(2000.0, 5000.0).max()))


def gpu_rows():
    """the rows of the GPU parity test, a list of (name, float32 samples): 1 / k and 1 / k^2 tones at 70, 220.5 and 480 Hz
    under white noise at 30 and 10 dB SNR, white noise, a DC row, a single impulse (a flat spectrum up to rounding in four
    frames, silence in the other four) and an all-zero row, at lengths that give one frame, partly empty edge frames and a workgroup's
    tile boundary from both sides"""
    W = FRAMES_PER_WORKGROUP
    lengths = [16000, 256 * W, 257, 16000, 255, 256 * W + 1, 16000, 256, 1, 16000, 256 * (W - 1), 513]
    rows = []
    for power in (1, 2):
        for f0 in (70.0, 220.5, 480.0):
            for snr in (30.0, 10.0):
                n = lengths[len(rows)]
                rows.append(('tone 1/k^%d %g Hz %g dB, %d' % (power, f0, snr, n), tone(f0, n, power, snr, seed=len(rows))))
    rows.append(('noise, 16000', noise(16000, seed=99)))
    rows.append(('dc, 513', np.full(513, 0.25, dtype=np.float32)))
    imp = np.zeros(256 * (W - 1), dtype=np.float32)
    imp[300] = 0.5                   # frames 0..3 see it under window weights from 0.02 to 0.98, frames 4..7 are silent
    rows.append(('impulse, %d' % imp.size, imp))
    rows.append(('zeros, %d' % (256 * W + 1), np.zeros(256 * W + 1, dtype=np.float32)))
    return rows


def measure_fp32(rows=None):
    """({plane: max |fp32 - fp64|}, share of frames exempt from the lag comparison, frames) over rows (default gpu_rows()):
    a frame is exempt when the fp64 peak stands less than the cpp tolerance above the second best"""
    worst = dict.fromkeys(FEATS[:5], 0.0)
    exempt = total = 0
    for _, x in (rows or gpu_rows()):
        r64, r32 = voice_quality(x), voice_quality(x, np.float32)
        assert np.array_equal(r64['level_db'] == SILENT_DB, r32['level_db'] == SILENT_DB)
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(r32[k].astype(np.float64) - r64[k]).max()))
        exempt += int((r64['lag_margin'] <= GPU_TOL['cpp_db']).sum())
        total += len(r64['cpp_db'])
    return worst, exempt / total, total
