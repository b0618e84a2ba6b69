"""numpy restatement of the phase start from magnitudes (include/t2vae.h, csrc/phase_init.hip): single-pass spectrogram
inversion (Beauregard, Harish and Wyse 2015) in the integer turns the kernels use, so the two can be compared bit for bit.

mag (513, n) fp32, one row's frames; N = 1024, hop 256, so a partial at bin x advances x / 4 turns per frame.  A turn is
2^32; every turn quantity is uint32 and wraps.
    peak        bin k in 1..511 with M[k] > M[k - 1] and M[k] > M[k + 1], compared in fp32 (a plateau has no peak)
    offset      p = (0.5 (a - c)) / ((a - 2 b) + c) in fp64 from a, b, c = M[k - 1], M[k], M[k + 1]; |p| < 1 / 2
    advance     adv(k, m) = ((k & 3) << 30) + rint(p 2^30) at a peak, 0 elsewhere: (k + p) / 4 turns
    accumulator acc(k, m) = sum of adv(k, m') over m' <= m: an integer sum, so any order and any chunking give the same bits
    assignment  kp = the peak of frame m nearest to k (a tie: the lower one),
                turns(k, m) = acc(kp, m) - ((k - kp) << 31) + rint(p(kp, m) 2^31):  -pi (k - kp - p), the phase of the
                periodic Hann window's transform at k - kp - p bins from the partial, referred to the frame's first sample
    phase       float32(float64(int32(turns)) 2 pi / 2^32), in [-pi, pi); a frame without a peak is +0 in every bin
`rint` is round-half-even, as the kernel's.  `start` is the fp64 chain of the tests: the phase, and the waveform it gives with
one inverse transform (vocoder_ref.istft)."""
import numpy as np

import vocoder_ref as V

BINS = 513
TURN = 2.0 * np.pi


def peaks(mag):
    """mag (513, n) fp32 -> bool (513, n)"""
    m = np.asarray(mag, dtype=np.float32)
    pk = np.zeros(m.shape, dtype=bool)
    pk[1:-1] = (m[1:-1] > m[:-2]) & (m[1:-1] > m[2:])
    return pk


def offsets(mag, pk):
    """p in fp64 at the peaks, 0 elsewhere; the operations in the kernel's order"""
    m = np.asarray(mag, dtype=np.float32).astype(np.float64)
    p = np.zeros(m.shape)
    a, b, c = m[:-2], m[1:-1], m[2:]
    with np.errstate(all='ignore'):
        q = (0.5 * (a - c)) / ((a - 2.0 * b) + c)
    p[1:-1] = np.where(pk[1:-1], q, 0.0)
    return p


def _fixed(p, bits):
    """(uint32)(int32) rint(p 2^bits)"""
    return np.rint(p * float(1 << bits)).astype(np.int64).astype(np.uint32)


def advances(mag):
    """(pk, p, adv uint32 (513, n))"""
    pk = peaks(mag)
    p = offsets(mag, pk)
    k = np.arange(BINS, dtype=np.uint32)[:, None]
    adv = np.where(pk, ((k & np.uint32(3)) << np.uint32(30)) + _fixed(p, 30), np.uint32(0)).astype(np.uint32)
    return pk, p, adv


def accumulate(adv):
    """the inclusive sum along time modulo 2^32"""
    return (np.cumsum(adv.astype(np.uint64), axis=1) & np.uint64(0xffffffff)).astype(np.uint32)


def nearest_peak(pk):
    """pk (513,) bool -> for every bin the index of its nearest peak, the lower one on a tie; None without a peak"""
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


def radians(turns):
    """uint32 turns -> float32 radians in [-pi, pi), one fp32 rounding"""
    return (turns.astype(np.uint32).view(np.int32).astype(np.float64) * (TURN / 4294967296.0)).astype(np.float32)


def spsi_turns(mag):
    """mag (513, n) fp32 -> (turns uint32 (513, n), has_peak bool (n,), acc uint32 (513, n))"""
    pk, p, adv = advances(mag)
    acc = accumulate(adv)
    n = acc.shape[1]
    turns = np.zeros((BINS, n), dtype=np.uint32)
    has = pk.any(axis=0)
    k = np.arange(BINS, dtype=np.int64)
    for m in range(n):
        kp = nearest_peak(pk[:, m])
        if kp is None:
            continue
        d = ((k - kp) & 1).astype(np.uint32) << np.uint32(31)             # ((uint32)(k - kp)) << 31
        turns[:, m] = acc[kp, m] - d + _fixed(p[kp, m], 31)
    return turns, has, acc


def spsi_phase(mag):
    """mag (513, n) fp32 -> phase (513, n) fp32 in [-pi, pi), +0 in a frame without a peak"""
    turns, has, _ = spsi_turns(mag)
    return np.where(has[None, :], radians(turns), np.float32(0.0)).astype(np.float32)


def spsi_batch(mag, n_frames):
    """mag (B, 513, stride), rows of n_frames[b] frames -> (B, 513, stride) fp32, +0 from each count on; nothing at or past
    a count is read"""
    mag = np.asarray(mag)
    out = np.zeros(mag.shape, dtype=np.float32)
    for b, n in enumerate(n_frames):
        n = min(max(int(n), 0), mag.shape[2])
        if n:
            out[b, :, :n] = spsi_phase(mag[b, :, :n])
    return out


def start(mag):
    """mag (513, n) -> the waveform of M exp(i spsi_phase(M)), one inverse transform in fp64 (the magnitudes reach the peak
    rules as fp32, as they reach the kernel)"""
    mag = np.asarray(mag, dtype=np.float64)
    ph = spsi_phase(mag.astype(np.float32)).astype(np.float64)
    return V.istft(mag * np.exp(1j * ph))


def random_angles(shape):
    """the reference's draw: np.angle(np.exp(2j pi np.random.rand(...))) from the global state"""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape)))


def voiced_share(f0, edge=8):
    """share of frames with f0 > 0, `edge` frames dropped at each end"""
    f = np.asarray(f0)[edge:len(f0) - edge]
    return float(np.mean(f > 0))
