#!/usr/bin/env python
"""Cost of the loudness meter (t2v_hip.loudness, csrc/loudness.hip) on one GPU.

    python tools/bench_loudness.py [--runs 7] [--out FILE]

64 rows of 5 s (seeded noise, float32) at 16 000 and at 48 000 Hz:
  * kernel: device time of t2v_loudness alone (the C call on buffers made beforehand: the filter kernel and the reduction; a
    pair of events around `inner` back-to-back calls, median of `runs` after a warm-up), next to the time the bytes it must move
    (every sample once) take at the chip's measured HBM copy rate (6.29 TB/s) and to the samples it filters per second;
  * call: the same through t2v_hip.loudness (length checks, allocation, upload of the lengths, the copy of the per-row scalars
    to the host), wall time with a synchronise;
  * scipy: scipy.signal.lfilter (both biquads) in float64 plus numpy block and frame sums on the same rows, in 16 worker
    processes (or as many CPUs as the machine has, if fewer): what a user without this kernel would run.  Measured before the
    GPU is touched.
Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

B, SECONDS = 64, 5.0
RATES = (16000, 48000)
HBM_COPY_BYTES_PER_S = 6.29e12               # the copy rate measured on this chip (tools/bench_resample.py)


def rows_of(sr):
    rng = np.random.RandomState(sr)
    return rng.uniform(-0.5, 0.5, (B, int(SECONDS * sr))).astype(np.float32)


def _meter_row(job):
    import loudness_ref
    x, sr, coef = job
    z = loudness_ref.kweight(x.astype(np.float64), coef)
    return loudness_ref.gate(loudness_ref.block_powers(z, sr))[:2], loudness_ref.frame_ms(z)


def scipy_seconds(x, sr, workers, runs):
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing
    import loudness_ref
    coef = loudness_ref.coefficients_f32(sr)
    jobs = [(x[b], sr, coef) for b in range(x.shape[0])]
    ts = []
    with ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context('spawn')) as pool:
        list(pool.map(_meter_row, jobs[:workers]))                     # the workers are up and have imported scipy
        for _ in range(runs):
            t0 = time.perf_counter()
            list(pool.map(_meter_row, jobs))
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    workers = min(16, os.cpu_count() or 1)
    data = {sr: rows_of(sr) for sr in RATES}
    res = {'rows': B, 'seconds_per_row': SECONDS, 'runs': args.runs, 'cpu_workers': workers}
    for sr in RATES:                                                   # before the GPU is initialised
        res['scipy_%d_s' % sr] = round(scipy_seconds(data[sr], sr, workers, args.runs), 4)

    import torch
    import t2v_hip
    lib = t2v_hip.load_library()
    res['device'] = torch.cuda.get_device_name(0)

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

    def wall_us(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(ts)

    lines = ['%7s %12s %12s %10s %14s %12s %12s' % ('rate', 'kernel us', 'HBM floor us', 'x floor', 'Gsamples/s', 'call us',
                                                    'scipy / call')]
    for sr in RATES:
        x = torch.from_numpy(data[sr]).cuda()
        S, hop = x.size(1), sr // 10
        n = [S] * B
        n_dev = torch.tensor(n, dtype=torch.int32, device='cuda')
        table = torch.from_numpy(t2v_hip.loudness_table(sr).copy()).cuda()
        ms_stride, blk_stride = S // 256 + 1, (S - 4 * hop) // hop + 1
        ms = torch.empty(B, ms_stride, device='cuda')
        blocks = torch.empty(B, blk_stride, device='cuda')
        rows = torch.empty(B, 8, dtype=torch.int32, device='cuda')
        scratch = torch.empty(lib.t2v_loudness_scratch_bytes(B, S, hop), dtype=torch.uint8, device='cuda')

        def launch():
            rc = lib.t2v_loudness(t2v_hip._p(x), t2v_hip._p(n_dev), S, B, t2v_hip._p(table), hop, t2v_hip._p(ms), ms_stride,
                                  t2v_hip._p(blocks), blk_stride, t2v_hip._p(rows), t2v_hip._p(scratch), t2v_hip._stream())
            assert rc == 0, rc
        k_us = event_us(launch, 10)
        floor = x.numel() * 4 / HBM_COPY_BYTES_PER_S * 1e6
        call = wall_us(lambda: t2v_hip.loudness(x, n, sr))
        res.update({'kernel_%d_us' % sr: round(k_us, 1), 'hbm_floor_%d_us' % sr: round(floor, 2), 'call_%d_us' % sr: round(call, 1),
                    'gsamples_per_s_%d' % sr: round(x.numel() / k_us * 1e-3, 1)})
        lines.append('%7d %12.1f %12.2f %10.1f %14.1f %12.1f %12.1f'
                     % (sr, k_us, floor, k_us / floor, x.numel() / k_us * 1e-3, call, res['scipy_%d_s' % sr] * 1e6 / call))
        lines.append('%d Hz: scipy.signal.lfilter + numpy sums, float64, %d processes: %.3f s for the %d rows'
                     % (sr, workers, res['scipy_%d_s' % sr], B))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
