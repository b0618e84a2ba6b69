#!/usr/bin/env python
"""Cost of the phase vocoder (t2v_hip.time_stretch, csrc/tsm.hip) on one GPU.

    python tools/bench_tsm.py [--runs 7] [--out FILE]

8 and 64 rows of 5 s at 16 kHz (seeded noise plus a tone, float32), at the rates 0.8 and 1.25, with and without phase locking:
  * vocoder: device time of t2v_phase_vocoder alone (the C call on spectrograms and scratch made beforehand; a pair of events
    around `inner` back-to-back calls, median of `runs` after a warm-up), next to the time its bytes take at the chip's measured
    HBM copy rate: magnitude and phase read once and written once, plus, with locking, the accumulators written and read and
    frame i's magnitude and phase read again.  The rows stay in the 256 MiB Infinity Cache across the back-to-back calls, so
    the ratio to that floor counts bytes; it is not HBM efficiency;
  * stretch: t2v_hip.time_stretch, the whole call (transform, vocoder, inverse, lengths), event-timed the same way;
  * transforms: stft_polar + istft alone on the same rows, what the call costs without the vocoder.
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
RATES = (0.8, 1.25)
HBM_COPY_BYTES_PER_S = 6.29e12               # the copy rate measured on this chip (tools/bench_resample.py)


def rows_of(B):
    rng = np.random.RandomState(B)
    n = int(SECONDS * SR)
    t = np.arange(n) / float(SR)
    return (0.1 * rng.randn(B, n) + 0.3 * np.sin(2 * np.pi * 220.0 * t)[None, :]).astype(np.float32)


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
    res = {'seconds_per_row': SECONDS, 'runs': args.runs, 'device': torch.cuda.get_device_name(0)}

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

    lines = ['%4s %6s %5s %12s %12s %9s %12s %14s' % ('B', 'rate', 'lock', 'vocoder us', 'HBM floor us', 'x floor',
                                                      'stretch us', 'transforms us')]
    for B in BATCHES:
        y = torch.from_numpy(rows_of(B)).cuda()
        S = y.size(1)
        n = [S] * B
        tables = t2v_hip._tsm_tables(y.device)
        mag, phase = t2v_hip.stft_polar(y, None, tables)
        T = mag.size(2)
        frames = torch.full((B,), T, dtype=torch.int32, device='cuda')

        def transforms():
            m, p = t2v_hip.stft_polar(y, None, tables)
            t2v_hip.istft(m, p, None, tables)
        tr_us = event_us(transforms, 5)
        res['transforms_B%d_us' % B] = round(tr_us, 1)
        for rate in RATES:
            num, den = t2v_hip.stretch_ratio(rate)
            t_out = t2v_hip.stretch_frames(T, num, den)
            mag_out = torch.empty(B, 513, t_out, device='cuda')
            phase_out = torch.empty_like(mag_out)
            for lock in (0, 1):
                scratch = torch.empty(max(int(lib.t2v_phase_vocoder_scratch_bytes(B, t_out, lock)), 1), dtype=torch.uint8, device='cuda')

                def launch():
                    rc = lib.t2v_phase_vocoder(t2v_hip._p(mag), t2v_hip._p(phase), t2v_hip._p(frames), B, T, T, num, den, lock,
                                               t2v_hip._p(mag_out), t2v_hip._p(phase_out), t_out, t2v_hip._p(scratch),
                                               t2v_hip._stream())
                    assert rc == 0, rc
                k_us = event_us(launch, 10)
                traffic = 4 * B * 513 * (2 * T + 2 * t_out + (4 * t_out if lock else 0))
                floor = traffic / HBM_COPY_BYTES_PER_S * 1e6
                st_us = event_us(lambda: t2v_hip.time_stretch(y, n, rate, bool(lock)), 5)
                key = 'B%d_r%g_lock%d' % (B, rate, lock)
                res.update({'vocoder_%s_us' % key: round(k_us, 1), 'hbm_floor_%s_us' % key: round(floor, 2),
                            'stretch_%s_us' % key: round(st_us, 1)})
                lines.append('%4d %6g %5d %12.1f %12.2f %9.1f %12.1f %14.1f' % (B, rate, lock, k_us, floor, k_us / floor, st_us, tr_us))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
