"""Reference audio_processing.py:7-92: `window_sumsquare`, `griffin_lim` (on the HIP kernels of csrc/vocoder.hip) and the
dynamic range compression pair."""
import numpy as np
import torch


def window_sumsquare(window, n_frames, hop_length=200, win_length=800, n_fft=800, dtype=np.float32, norm=None):
    """Sum-square envelope of `window` over n_frames frames hop_length apart (librosa 0.6), length
    n_fft + hop_length * (n_frames - 1); host numpy, the reference's signature and result."""
    from scipy.signal import get_window
    if win_length is None:
        win_length = n_fft
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    win_sq = get_window(window, win_length, fftbins=True)
    if norm is not None:
        win_sq = win_sq / np.linalg.norm(win_sq, ord=norm)
    win_sq = win_sq ** 2
    lpad = (n_fft - win_length) // 2
    win_sq = np.pad(win_sq, (lpad, n_fft - win_length - lpad))
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


INITS = ('random', 'spsi')


def check_init(init):
    """the initial phase of Griffin-Lim: 'random' (the reference's np.random draw) or 'spsi'; ValueError otherwise"""
    if init not in INITS:
        raise ValueError("griffin_lim: init must be one of %s, got %r" % (', '.join(repr(v) for v in INITS), init))
    return init


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None, lengths=None, momentum=0.0, init='random'):
    """magnitudes (B, 513, T) -> signal (B, (T-1)*256) after n_iters Griffin-Lim iterations on the device (t2v_griffin_lim).
    angles: initial phase (B, 513, T); None draws it as the reference does, from np.random on the host, so a caller who
    seeds np.random gets the reference's starting point.  lengths: optional per-utterance frame counts (samples past
    (T_b-1)*256 are zero).  Every utterance needs T >= 4 frames.  The result is returned on the magnitudes' device.
    momentum in [0, 1): fast Griffin-Lim (librosa's default is 0.99); 0 is the reference's plain iteration.
    init='spsi': the initial phase is computed on the device from the magnitudes (`t2v_hip.spsi_phase`, single-pass
    spectrogram inversion) and np.random is not touched; giving `angles` as well is a ValueError.  With n_iters=0 the result
    is `t2v_hip.istft(magnitudes, spsi_phase(magnitudes), lengths, tables)`: the start alone, which keeps every partial
    coherent in time."""
    import t2v_hip
    from stft import STFT
    momentum = t2v_hip.check_momentum(momentum)
    if check_init(init) == 'spsi' and angles is not None:
        raise ValueError("griffin_lim: init='spsi' computes the initial phase; it cannot be combined with angles")
    if not isinstance(stft_fn, STFT):
        raise TypeError("griffin_lim runs on the HIP STFT (stft.STFT, e.g. TacotronSTFT.stft_fn), got %r" % type(stft_fn))
    if angles is None and init == 'random':
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size())))
        angles = torch.from_numpy(angles.astype(np.float32))
    T = magnitudes.size(-1)
    n = [T] if lengths is None else torch.as_tensor(lengths).reshape(-1).tolist()
    if min(n) < 4:
        raise ValueError("griffin_lim needs at least 4 frames per utterance (each iteration's transform reflect-pads its "
                         "(T-1)*256 samples by 512), got %s" % n)
    m = stft_fn.on_gpu(magnitudes)
    if init == 'spsi':
        a = t2v_hip.spsi_phase(m, lengths)
        if int(n_iters) == 0:
            return t2v_hip.istft(m, a, lengths, stft_fn.tables(m.device)).to(magnitudes.device)
    else:
        a = angles.to(m.device).float()
    return t2v_hip.griffin_lim(m, a, lengths, stft_fn.tables(m.device), n_iters, momentum).to(magnitudes.device)


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    return torch.exp(x) / C
