"""fp64 direct forms of what csrc/resample.hip computes, for the tests: the polyphase resampler, the trim bounds and the crop /
16-bit write-out, written from the definitions in include/t2vae.h with numpy only."""
import math

import numpy as np

HOP = 256
RATES = (48000, 44100, 22050, 24000, 11025, 8000)       # -> 16 000 Hz
LENGTHS = (1, 7, 1000, 1777)


def window(sr_in, sr_out, zeros=16, beta=8.6, rolloff=0.95):
    """(up, down, half, g): g in fp64, sum 1 — the `window` of scipy.signal.resample_poly; the taps are up g"""
    g0 = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g0, int(sr_in) // g0
    half = zeros * max(up, down)
    fc = rolloff / max(up, down)
    k = np.arange(2 * half + 1, dtype=np.float64)
    g = fc * np.sinc(fc * (k - half)) * np.kaiser(2 * half + 1, beta)
    return up, down, half, g / g.sum()


def resample(x, up, down, half, taps):
    """y[m] = sum_i t[m down - i up + half] x[i] for m < ceil(n up / down), in fp64 with the taps as given (the fp32-rounded
    ones for a comparison with the kernel).  Returns (y, sum_i |t x| per output, taps that met a sample per output)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(taps, dtype=np.float64)
    n = len(x)
    n_out = -((-n * up) // down)
    y, mag, cnt = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    for m in range(n_out):
        a = m * down + half
        i_hi = min(a // up, n - 1)                       # tap index a - i up >= 0
        i_lo = max(-((2 * half - a) // up), 0)           # tap index a - i up <= 2 half: i >= ceil((a - 2 half) / up)
        if i_hi < i_lo:
            continue
        i = np.arange(i_lo, i_hi + 1)
        prod = t[a - i * up] * x[i]
        y[m], mag[m], cnt[m] = prod.sum(), np.abs(prod).sum(), len(i)
    return y, mag, cnt


def taps_per_phase(up, half):
    """the longest phase's tap count: the K of the kernel's K-term chain"""
    return (2 * half) // up + 1


def frame_ms(x):
    """mean square of the frames [256 t - 512, 256 t + 512) of x, zeros outside, n // 256 + 1 frames, fp64"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    pad = np.concatenate([np.zeros(512), x, np.zeros(1024)])
    return np.array([np.mean(pad[HOP * t:HOP * t + 1024] ** 2) for t in range(n // HOP + 1)])


def trim_bounds(x, top_db=40.0, pad_frames=2):
    """(start, end, margin): the bounds, and the smallest relative distance |ms / (ref thr) - 1| of any frame from the threshold
    (inf for an all-zero row)"""
    n = len(x)
    ms = frame_ms(x)
    ref = ms.max()
    if not ref > 0:
        return 0, n, float('inf')
    cut = ref * 10.0 ** (-top_db / 10.0)
    margin = float(np.min(np.abs(ms / cut - 1.0)))
    on = np.nonzero(ms > cut)[0]
    first, last = int(on[0]), int(on[-1])
    return HOP * max(0, first - pad_frames), min(n, HOP * (last + 1 + pad_frames)), margin


def crop_pcm16(y, start, end):
    """(int16 samples, clipped count, max |y| as fp32) of y[start:end] (fp32): rint(y 32768) in fp32, clamped"""
    seg = np.asarray(y, dtype=np.float32)[start:end]
    r = np.rint(seg * np.float32(32768.0))
    clipped = int(np.sum((r > 32767) | (r < -32768)))
    peak = np.float32(np.max(np.abs(seg))) if len(seg) else np.float32(0)
    return np.clip(r, -32768, 32767).astype(np.int16), clipped, peak


def trim_cases():
    """[(name, fp32 samples)]: the constructed signals of the trim tests.  Silence is noise 55 dB under the tone (the trim's
    default threshold is 40 dB), so the frames that decide the bounds are the ones that overlap the tone."""
    rng = np.random.RandomState(7)

    def tone(n):
        return 0.5 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 16000.0 + 0.3)

    def hush(n):
        return 1e-3 * (2 * rng.rand(n) - 1)

    cases = [('silence_tone_silence', np.concatenate([hush(1500), tone(3000), hush(1277)])),
             ('sound_to_the_last_sample', np.concatenate([hush(1300), tone(1501)])),
             ('all_zero', np.zeros(1500)),
             ('one_sample', np.array([0.5]))]
    return [(name, x.astype(np.float32)) for name, x in cases]
