#!/usr/bin/env python
"""Cost of the spectral envelope (t2v_spectral_envelope, csrc/envelope.hip) and of the formant-preserving pitch shift on one GPU.

    python tools/bench_envelope.py [--runs 7] [--out FILE]

8 and 64 rows of 5 s at 16 kHz (a synthetic vowel plus seeded noise, float32; 313 frames a row), order 32, at 0 and 8
true-envelope iterations:
  * envelope: device time of the C call alone, writing the log envelope (a pair of events around `inner` back-to-back calls
    on spectrograms made beforehand, median of `runs` after a warm-up);
  * env+warp: the same call writing the log envelope and the magnitudes warped by 4 semitones' ratio;
  * HBM floor: the time the call's bytes take at the chip's measured HBM copy rate: the magnitudes read once, 4 x 513 x B x T
    bytes, and as much written per output.  The rows stay in the 256 MiB Infinity Cache across the back-to-back calls, so the
    ratio to that floor counts bytes; it is not HBM efficiency.  The kernel does 2 (iters + 1) 1024-point transforms a
    frame in LDS, and is expected to be bound by them;
  * FFT us: envelope time / (B x T x 2 (iters + 1)), the call's time per 1024-point transform with the whole chip at work
    (not the latency of one);
  * pitch_shift us: t2v_hip.pitch_shift by 4 semitones, the whole call, plain and with preserve_formants (event-timed the same
    way; iters as in the row).
Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

SECONDS, SR = 5.0, 16000
BATCHES = (8, 64)
ITERS = (0, 8)
ORDER = 32
SEMITONES = 4
HBM_COPY_BYTES_PER_S = 6.29e12               # the copy rate measured on this chip (tools/bench_resample.py)


def rows_of(B):
    """B rows: an impulse train at 100..240 Hz through three two-pole resonators, plus noise"""
    from scipy.signal import lfilter
    rng = np.random.RandomState(B)
    n = int(SECONDS * SR)
    y = np.zeros((B, n))
    for b in range(B):
        x = np.zeros(n)
        x[np.arange(0.0, n, SR / (100.0 + 140.0 * b / B)).astype(np.int64)] = 1.0
        for hz, bw in ((700.0, 80.0), (1200.0, 100.0), (2600.0, 140.0)):
            r = np.exp(-np.pi * bw / SR)
            x = lfilter([1.0], [1.0, -2.0 * r * np.cos(2.0 * np.pi * hz / SR), r * r], x)
        y[b] = 0.5 * x / np.abs(x).max()
    return (y + 0.01 * rng.randn(B, n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import torch
    import t2v_hip
    lib = t2v_hip.load_library()
    res = {'seconds_per_row': SECONDS, 'runs': args.runs, 'order': ORDER, 'device': torch.cuda.get_device_name(0)}

    def event_us(fn, inner):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / inner)
        return statistics.median(ts)

    p, q = t2v_hip.pitch_ratio(SEMITONES)
    lines = ['%4s %5s %12s %9s %9s %12s %9s %9s %10s %12s' % ('B', 'iters', 'envelope us', 'floor us', 'x floor', 'env+warp us',
                                                            'floor us', 'FFT us', 'shift us', 'preserve us')]
    for B in BATCHES:
        y = torch.from_numpy(rows_of(B)).cuda()
        S = y.size(1)
        n = [S] * B
        mag, _ = t2v_hip.stft_polar(y, None, t2v_hip._tsm_tables(y.device))
        T = mag.size(2)
        frames = torch.full((B,), T, dtype=torch.int32, device='cuda')
        env, out = torch.empty_like(mag), torch.empty_like(mag)
        plain_us = event_us(lambda: t2v_hip.pitch_shift(y, n, SEMITONES), 5)
        res['pitch_shift_B%d_us' % B] = round(plain_us, 1)
        for iters in ITERS:
            def launch(ratio, mag_out):
                rc = lib.t2v_spectral_envelope(t2v_hip._p(mag), t2v_hip._p(frames), B, T, T, ORDER, iters, ratio[0], ratio[1],
                                               t2v_hip._p(env), None if mag_out is None else t2v_hip._p(mag_out), T, t2v_hip._stream())
                assert rc == 0, rc
            e_us = event_us(lambda: launch((1, 1), None), 20)
            w_us = event_us(lambda: launch((p, q), out), 20)
            unit = 4 * 513 * B * T
            floor_e, floor_w = 2 * unit / HBM_COPY_BYTES_PER_S * 1e6, 3 * unit / HBM_COPY_BYTES_PER_S * 1e6
            fft_us = e_us / (B * T * 2 * (iters + 1))
            keep_us = event_us(lambda: t2v_hip.pitch_shift(y, n, SEMITONES, preserve_formants=True, order=ORDER, iters=iters), 5)
            key = 'B%d_it%d' % (B, iters)
            res.update({'envelope_%s_us' % key: round(e_us, 1), 'hbm_floor_envelope_%s_us' % key: round(floor_e, 2),
                        'warp_%s_us' % key: round(w_us, 1), 'hbm_floor_warp_%s_us' % key: round(floor_w, 2),
                        'fft_%s_us' % key: round(fft_us, 5), 'pitch_shift_preserve_%s_us' % key: round(keep_us, 1)})
            lines.append('%4d %5d %12.1f %9.2f %9.1f %12.1f %9.2f %9.4f %10.1f %12.1f'
                         % (B, iters, e_us, floor_e, e_us / floor_e, w_us, floor_w, fft_us, plain_us, keep_us))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
