#!/usr/bin/env python
"""Write tests/golden/griffin_lim.npz by running the reference's own STFT / griffin_lim on CPU (test infrastructure).

    python tools/gen_golden_griffin_lim.py [--out DIR]

Needs the read-only reference and oracle/_refimport (run it as its own process, like oracle/gen_golden.py).  The
product's stft.py / audio_processing.py / layers.py share their module names with the reference's, so the product
package is never put on sys.path here.  Stored: the first 16384 samples of samples/refs/ref_hap.wav (int16, 16 kHz), the
reference STFT(1024, 256, 1024) magnitude / phase and inverse of them, window_sumsquare for that T, and the reference
griffin_lim output under np.random.seed(seed) with the relative L2 distance between it and an fp64 numpy restatement
started from the same angles.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import _refimport  # noqa: E402

SEED, N_ITERS = 7, 30
OFFSET, N = 0, 16384            # the first 16384 samples -> T = 65 frames


def _win():
    n = np.arange(1024)
    return 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)


def stft64(y):
    """(N,) -> complex (513, N//256 + 1): reflect pad 512, periodic Hann, rfft"""
    p = np.pad(y, 512, mode='reflect')
    T = len(y) // 256 + 1
    fr = np.stack([p[256 * t:256 * t + 1024] for t in range(T)]) * _win()
    return np.fft.rfft(fr, axis=1).T


def istft64(mag, phase):
    """the reference's pinv basis = irfft; window, overlap-add, / window_sumsquare where > tiny(float32), trim 512"""
    T = mag.shape[1]
    w = _win()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    R = _refimport.load()
    import audio_processing as r_audio     # the reference's (its directory is first on sys.path now)
    from scipy.io.wavfile import read
    sr, wav = read(os.path.join(_refimport.REF, 'samples', 'refs', 'ref_hap.wav'))
    assert sr == 16000 and wav.dtype == np.int16
    clip = wav[OFFSET:OFFSET + N].copy()
    x = torch.from_numpy(clip.astype(np.float32) / 32768.0)[None]
    stft = R['stft'].STFT(1024, 256, 1024)
    with torch.no_grad():
        mag, phase = stft.transform(x)
        inv = stft.inverse(mag, phase)
        T = mag.size(2)
        wss = r_audio.window_sumsquare('hann', T, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
        np.random.seed(SEED)
        gl = r_audio.griffin_lim(mag, stft, N_ITERS)
    np.random.seed(SEED)
    angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mag.size()))).astype(np.float32)
    gl64 = griffin_lim64(mag[0].double().numpy(), angles[0].astype(np.float64), N_ITERS)
    gl = gl[0].numpy()
    rel = float(np.linalg.norm(gl - gl64) / np.linalg.norm(gl64))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'griffin_lim.npz')
    np.savez_compressed(path, clip=clip, offset=np.int64(OFFSET), magnitude=mag[0].numpy(), phase=phase[0].numpy(),
                        inverse=inv[0, 0].numpy(), window_sumsquare=wss, seed=np.int64(SEED), n_iters=np.int64(N_ITERS),
                        griffin_lim=gl, gl_rel_l2_vs_fp64=np.float64(rel))
    print('wrote %s: T=%d, reference griffin_lim vs fp64 relative L2 %.3e' % (path, T, rel))


if __name__ == '__main__':
    main()
