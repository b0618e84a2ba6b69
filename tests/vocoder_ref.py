"""numpy restatement of the two vocoder-quality pieces of csrc/vocoder.hip (include/t2vae.h): the non-negative
least-squares mel inversion and fast Griffin-Lim.  fp64 is the reference of tests/test_vocoder_fast_gpu.py; the same
functions run with dtype=np.float32 are its yardstick of what single precision costs (the convention of tests/tsne_ref.py).

Mel inversion, per frame, m = exp(mel) (80), B the (80, 513) mel filterbank, P = pinv(B), L = ||B||_2^2:
    M_0 = max(P m, 0);  n_iters times:  r = B M - m,  M <- max(M - B^T r / L, 0)
The step 1 / L makes 0.5 ||B M - m||^2 non-increasing.  Every sum runs in the kernel's order: P m over the mels ascending, a
filter's B M over its bins ascending, a bin's B^T r as (lower filter's term) + (upper filter's term).

Fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013, in librosa's form), alpha = momentum / (1 + momentum):
    X = M exp(i angles), tprev = 0;  n_iters times:  rebuilt = STFT(ISTFT(X)),  a = rebuilt - alpha tprev,  tprev = rebuilt,
    X = M a / |a| (M where |a| = 0);  the signal is ISTFT(X).  momentum = 0 is plain Griffin-Lim.
Framing as the kernels have it: reflect pad 512, periodic Hann of 1024, hop 256, the inverse a windowed irfft (imaginary
parts of bins 0 and 512 ignored), overlap-added, divided by the window sum-square where it is > tiny(float32), 512 samples
trimmed at each end.
"""
import numpy as np

SR, N_FFT, HOP, N_BIN, N_MEL = 16000, 1024, 256, 513, 80


def _cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def hann(dtype=np.float64):
    n = np.arange(N_FFT)
    return (0.5 - 0.5 * np.cos(2 * np.pi * n / N_FFT)).astype(dtype)


def stft(y, dtype=np.float64):
    """(N,) -> complex (513, N // 256 + 1)"""
    y = np.asarray(y, dtype=dtype)
    p = np.pad(y, N_FFT // 2, mode='reflect')
    T = len(y) // HOP + 1
    fr = np.stack([p[HOP * t:HOP * t + N_FFT] for t in range(T)]) * hann(dtype)
    return np.fft.rfft(fr, axis=1).T.astype(_cdtype(dtype))


def istft(spec, dtype=np.float64):
    """complex (513, T) -> ((T - 1) * 256,)"""
    T = spec.shape[1]
    w = hann(dtype)
    fr = np.fft.irfft(np.asarray(spec, dtype=_cdtype(dtype)).T, n=N_FFT, axis=1).astype(dtype) * w
    n = N_FFT + HOP * (T - 1)
    y, wss = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for t in range(T):
        y[HOP * t:HOP * t + N_FFT] += fr[t]
        wss[HOP * t:HOP * t + N_FFT] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[N_FFT // 2:n - N_FFT // 2]


def with_magnitude(a, mag):
    """mag times the unit phasor of a; (mag, 0) where |a| = 0"""
    r = np.abs(a)
    ok = r > 0
    return np.where(ok, a * (mag / np.where(ok, r, 1)), mag).astype(a.dtype)


def griffin_lim(mag, angles, n_iters, momentum=0.0, dtype=np.float64):
    """mag, angles (513, T) -> ((T - 1) * 256,) after n_iters iterations of fast Griffin-Lim"""
    if not 0.0 <= momentum < 1.0:
        raise ValueError("momentum must be in [0, 1), got %r" % (momentum,))
    mag, angles = np.asarray(mag, dtype=dtype), np.asarray(angles, dtype=dtype)
    alpha = dtype(momentum / (1.0 + momentum))
    X = (mag * np.cos(angles) + 1j * (mag * np.sin(angles))).astype(_cdtype(dtype))
    tprev = np.zeros_like(X)
    for _ in range(n_iters):
        rebuilt = stft(istft(X, dtype), dtype)
        a = rebuilt - alpha * tprev
        tprev = rebuilt
        X = with_magnitude(a, mag)
    return istft(X, dtype)


def spectral_convergence(y, mag):
    """|| |STFT(y)| - M || / || M ||, in fp64"""
    mag = np.asarray(mag, dtype=np.float64)
    return float(np.linalg.norm(np.abs(stft(np.asarray(y, dtype=np.float64))) - mag) / np.linalg.norm(mag))


# ------------------------------------------------------------------ mel inversion
def lipschitz(basis):
    """L = ||B||_2^2 of the filterbank as stored (fp64 of its values)"""
    return float(np.linalg.norm(np.asarray(basis, dtype=np.float64), 2) ** 2)


def filter_rows(basis):
    """per filter: first bin, bin count and the weights of that range as (80, maxw), zero past each count"""
    B = np.asarray(basis)
    nz = [np.nonzero(row)[0] for row in B]
    start = np.array([int(i[0]) if len(i) else 0 for i in nz])
    length = np.array([int(i[-1] - i[0] + 1) if len(i) else 0 for i in nz])
    rows = np.zeros((B.shape[0], max(int(length.max()), 1)), dtype=B.dtype)
    for f in range(B.shape[0]):
        rows[f, :length[f]] = B[f, start[f]:start[f] + length[f]]
    return start, length, rows


def bin_taps(basis):
    """per bin: the lower of its (at most two, adjacent) filters and the two weights; ValueError for any other basis"""
    B = np.asarray(basis)
    n_mel = B.shape[0]
    lo = np.zeros(B.shape[1], dtype=np.int64)
    for k in range(B.shape[1]):
        f = np.nonzero(B[:, k])[0]
        lo[k] = min(int(f[0]), n_mel - 2) if len(f) else 0
        if len(f) and int(f[-1]) > lo[k] + 1:
            raise ValueError("bin %d lies in filters %s: not a two-tap filterbank" % (k, f.tolist()))
    k = np.arange(B.shape[1])
    return lo, B[lo, k], B[lo + 1, k]


def clipped_pinv(m, pinv, dtype=np.float64):
    """max(P m, 0), summed over the mels in ascending order.  m (80, T), pinv (513, 80) -> (513, T)"""
    m, P = np.asarray(m, dtype=dtype), np.asarray(pinv, dtype=dtype)
    acc = np.zeros((P.shape[0], m.shape[1]), dtype=dtype)
    for j in range(P.shape[1]):
        acc += P[:, j:j + 1] * m[j:j + 1]
    return np.maximum(acc, 0)


def apply_basis(basis, M, dtype=np.float64):
    """B M with each filter's sum over its bins in ascending order.  M (513, T) -> (80, T)"""
    start, length, rows = filter_rows(np.asarray(basis, dtype=dtype))
    M = np.asarray(M, dtype=dtype)
    acc = np.zeros((len(start), M.shape[1]), dtype=dtype)
    for j in range(rows.shape[1]):
        k = np.minimum(start + j, M.shape[0] - 1)         # past a filter's count the weight is 0
        acc += rows[:, j:j + 1] * M[k]
    return acc


def nnls(m, basis, pinv, n_iters, dtype=np.float64, trace=None):
    """n_iters projected-gradient steps from the clipped pseudo-inverse.  m = exp(mel) (80, T) -> M (513, T).  trace: a list
    that receives 0.5 ||B M - m||^2 (fp64, dense product) of the start and of every iterate."""
    B = np.asarray(basis, dtype=dtype)
    m = np.asarray(m, dtype=dtype)
    inv_l = dtype(1.0) / dtype(np.float32(lipschitz(basis)))          # L reaches the kernel as one float
    lo, w0, w1 = bin_taps(B)
    M = clipped_pinv(m, pinv, dtype)

    def objective():
        d = np.asarray(basis, dtype=np.float64) @ M.astype(np.float64) - m.astype(np.float64)
        return 0.5 * float(np.sum(d * d))

    if trace is not None:
        trace.append(objective())
    for _ in range(n_iters):
        r = apply_basis(B, M, dtype) - m
        g = w0[:, None] * r[lo] + w1[:, None] * r[lo + 1]
        M = np.maximum(M - g * inv_l, 0)
        if trace is not None:
            trace.append(objective())
    return M


def nnls_dense(m, basis, pinv, n_iters):
    """the same iteration with dense fp64 products (the form of the algorithm's description)"""
    B = np.asarray(basis, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    L = np.linalg.norm(B, 2) ** 2
    M = np.maximum(np.asarray(pinv, dtype=np.float64) @ m, 0)
    for _ in range(n_iters):
        M = np.maximum(M - B.T @ (B @ M - m) / L, 0)
    return M


def mel_residual(basis, M, m):
    """per-frame ||B M - m||_2 in fp64.  -> (T,)"""
    d = np.asarray(basis, dtype=np.float64) @ np.asarray(M, dtype=np.float64) - np.asarray(m, dtype=np.float64)
    return np.sqrt(np.sum(d * d, axis=0))


def tone(f0, seconds=2.0, harmonics=5):
    """a steady tone: harmonics k = 1..5 of f0 with amplitudes 1 / k, zero phase"""
    t = np.arange(int(seconds * SR)) / SR
    return sum(np.sin(2 * np.pi * k * f0 * t) / k for k in range(1, harmonics + 1))


def frame_magnitudes(y):
    """|rfft| of the unpadded frames of 1024 / hop 256 under the periodic Hann window.  (N,) -> (513, (N - 1024) // 256 + 1)"""
    y = np.asarray(y, dtype=np.float64)
    T = (len(y) - N_FFT) // HOP + 1
    fr = np.stack([y[HOP * t:HOP * t + N_FFT] for t in range(T)]) * hann()
    return np.abs(np.fft.rfft(fr, axis=1)).T
