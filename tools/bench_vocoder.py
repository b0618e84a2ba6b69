#!/usr/bin/env python
"""Griffin-Lim vocoder timing on one GPU: prints one JSON line.

    python tools/bench_vocoder.py [--runs 20] [--warmup 3]

For each (B, T, n_iters) in (1, 600, 60), (8, 600, 60), (1, 600, 30): the median over `runs` timed calls (HIP events
around audio_processing.griffin_lim, after warm-up) with the initial angles already on the device, so the host RNG is
not timed.  gl_iter_us = the per-iteration cost at B = 1, T = 600: (t(60) - t(30)) / 30, i.e. k_gl_iter's duration
plus the launch gap between two iterations."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

TARGET_MS = 2.5           # (1, 600, 60)


def time_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    from audio_processing import griffin_lim
    from stft import STFT
    stft = STFT(1024, 256, 1024)
    g = torch.Generator(device='cuda').manual_seed(0)
    res = {}
    for B, T, n_iters in ((1, 600, 60), (8, 600, 60), (1, 600, 30)):
        mag = torch.rand(B, 513, T, device='cuda', generator=g)
        angles = (torch.rand(B, 513, T, device='cuda', generator=g) * 2 - 1) * 3.14159265
        ms = time_ms(lambda: griffin_lim(mag, stft, n_iters, angles=angles), args.runs, args.warmup)
        res['B%d_T%d_it%d_ms' % (B, T, n_iters)] = round(ms, 4)
    res['gl_iter_us'] = round((res['B1_T600_it60_ms'] - res['B1_T600_it30_ms']) / 30 * 1e3, 2)
    res['target_B1_T600_it60_ms'] = TARGET_MS
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
