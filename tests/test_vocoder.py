"""Griffin-Lim vocoder and the reference's inverse-STFT surface, CPU side: an fp64 numpy restatement of STFT.inverse and
griffin_lim against the reference's own outputs (tests/golden/griffin_lim.npz, tools/gen_golden_griffin_lim.py), the
host-side window_sumsquare, and the API of stft.STFT / TacotronSTFT.  Also the restatement used by test_vocoder_gpu.py."""
import os

import numpy as np
import pytest


def hann64():
    n = np.arange(1024)
    return 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)


def stft64(y):
    """(N,) -> complex (513, N//256 + 1): reflect pad 512, periodic Hann, rfft"""
    p = np.pad(y, 512, mode='reflect')
    T = len(y) // 256 + 1
    fr = np.stack([p[256 * t:256 * t + 1024] for t in range(T)]) * hann64()
    return np.fft.rfft(fr, axis=1).T


def istft64(mag, phase):
    """STFT.inverse: the reference's pinv(scale F) basis x scale is irfft (imaginary parts of bins 0 and 512 ignored);
    window, overlap-add, / window_sumsquare where > tiny(float32), trim 512 samples at each end"""
    T = mag.shape[1]
    w = hann64()
    fr = np.fft.irfft((mag * np.exp(1j * phase)).T, n=1024, axis=1) * w
    n = 1024 + 256 * (T - 1)
    y, wss = np.zeros(n), np.zeros(n)
    for t in range(T):
        y[256 * t:256 * t + 1024] += fr[t]
        wss[256 * t:256 * t + 1024] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[512:n - 512]


def griffin_lim64(mag, angles, n_iters):
    y = istft64(mag, angles)
    for _ in range(n_iters):
        y = istft64(mag, np.angle(stft64(y)))
    return y


def reference_angles(seed, shape):
    """the reference's initial phase (audio_processing.py:60) under np.random.seed(seed)"""
    np.random.seed(seed)
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def spectral_convergence(y, mag):
    return float(np.linalg.norm(np.abs(stft64(y)) - mag) / np.linalg.norm(mag))


@pytest.fixture(scope='module')
def gl_golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'griffin_lim.npz'))


def test_fp64_restatement_reproduces_reference_inverse(gl_golden):
    g = gl_golden
    y = istft64(g['magnitude'].astype(np.float64), g['phase'].astype(np.float64))
    ref = g['inverse']
    assert y.shape == ref.shape == (256 * (g['magnitude'].shape[1] - 1),)
    assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    # and the reference's transform is the fp64 STFT of the clip
    X = stft64(g['clip'].astype(np.float64) / 32768.0)
    assert np.abs(np.abs(X) - g['magnitude']).max() <= 1e-5 * g['magnitude'].max()


def test_fp64_restatement_reproduces_reference_griffin_lim(gl_golden):
    g = gl_golden
    mag = g['magnitude'].astype(np.float64)
    angles = reference_angles(int(g['seed']), (1,) + mag.shape)[0]
    y = griffin_lim64(mag, angles.astype(np.float64), int(g['n_iters']))
    rel = np.linalg.norm(g['griffin_lim'] - y) / np.linalg.norm(y)
    assert rel <= 1.0001 * float(g['gl_rel_l2_vs_fp64']), rel


def test_window_sumsquare_matches_reference(gl_golden):
    from audio_processing import window_sumsquare
    T = gl_golden['magnitude'].shape[1]
    w = window_sumsquare('hann', T, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
    assert w.dtype == np.float32 and np.array_equal(w, gl_golden['window_sumsquare'])


def test_tacotron_stft_vocoder_surface():
    import torch
    from layers import TacotronSTFT
    from stft import STFT
    s = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    assert list(s.state_dict().keys()) == ['mel_basis']
    assert isinstance(s.stft_fn, STFT) and (s.stft_fn.filter_length, s.stft_fn.hop_length) == (1024, 256)
    assert callable(s.spectral_de_normalize) and callable(s.mel_to_magnitude)
    x = torch.tensor([0.5, 1.0, 2.0])
    assert torch.allclose(s.spectral_de_normalize(s.spectral_normalize(x)), x)


def test_stft_other_geometry_is_refused():
    from stft import STFT
    with pytest.raises(NotImplementedError):
        STFT(800, 200, 800)
    STFT(1024, 256, 1024)


def test_griffin_lim_refuses_fewer_than_four_frames():
    import torch
    from audio_processing import griffin_lim
    from stft import STFT
    with pytest.raises(ValueError):
        griffin_lim(torch.ones(1, 513, 3), STFT(1024, 256, 1024), 2)

