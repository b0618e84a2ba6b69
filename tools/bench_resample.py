#!/usr/bin/env python
"""Cost of the polyphase resampler (t2v_hip.resample, csrc/resample.hip) and of what prepare_corpus.py does around it, on one GPU.

    python tools/bench_resample.py [--runs 7] [--out FILE]

64 rows of 5 s (seeded noise, int16 as a wav holds it) at 48 000 and at 44 100 Hz -> 16 000 Hz:
  * kernel: device time of t2v_resample alone (the C call on buffers made beforehand; a pair of events around `inner`
    back-to-back calls, median of `runs` after a warm-up), for int16 and for float32 input, next to the time the bytes it must
    move (input once, output once) take at the chip's measured HBM copy rate (6.29 TB/s) and to its fma count;
  * call: the same through t2v_hip.resample (length checks, allocation, upload of the lengths), wall time with a synchronise;
  * trim + crop: t2v_hip.trim_bounds and t2v_hip.crop(pcm16=True, return_stats=True) on the resampled batch, wall time;
  * scipy: scipy.signal.resample_poly with the same window on the same rows, float64, in 16 worker processes (or as many CPUs as
    the machine has, if fewer): what a user without this stage would run.  Measured before the GPU is touched;
  * files: writing the 64 rows as int16 wavs to a temporary directory and reading them back (wavio.read_wav), the upload of the
    int16 batch, the download of the cropped int16 batch and the writing of the prepared wavs: the rest of prepare_corpus.
Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

B, SECONDS, TARGET = 64, 5.0, 16000
RATES = (48000, 44100)
HBM_COPY_BYTES_PER_S = 6.29e12


def rows_of(sr):
    rng = np.random.RandomState(sr)
    return (rng.uniform(-0.5, 0.5, (B, int(SECONDS * sr))) * 32767).astype(np.int16)


def _poly_row(job):
    from scipy.signal import resample_poly
    x, up, down, g = job
    return resample_poly(x.astype(np.float64) / 32768.0, up, down, window=g)


def scipy_seconds(x, up, down, g, workers, runs):
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing
    jobs = [(x[b], up, down, g) for b in range(x.shape[0])]
    ts = []
    with ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context('spawn')) as pool:
        list(pool.map(_poly_row, jobs[:workers]))                      # the workers are up and have imported scipy
        for _ in range(runs):
            t0 = time.perf_counter()
            list(pool.map(_poly_row, jobs))
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import resample_ref
    workers = min(16, os.cpu_count() or 1)
    data = {sr: rows_of(sr) for sr in RATES}
    res = {'rows': B, 'seconds_per_row': SECONDS, 'runs': args.runs, 'cpu_workers': workers}
    for sr in RATES:                                                   # before the GPU is initialised
        up, down, half, g = resample_ref.window(sr, TARGET)
        res['scipy_%d_s' % sr] = round(scipy_seconds(data[sr], up, down, g, workers, 5), 4)

    import torch
    import t2v_hip
    from scipy.io.wavfile import write
    from wavio import read_wav
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

    lines = ['%7s %6s %12s %12s %10s %12s %12s %14s %12s' % ('rate', 'input', 'kernel us', 'HBM floor us', 'x floor', 'Gfma/s',
                                                              'call us', 'trim+crop us', 'scipy / call')]
    for sr in RATES:
        up, down, half, taps = t2v_hip.resample_taps(sr, TARGET)
        S = data[sr].shape[1]
        n = [S] * B
        n_out = t2v_hip.resample_length(S, up, down)
        fmas = B * sum((2 * half - (m * down + half) % up) // up + 1 for m in range(n_out))
        x16 = torch.from_numpy(data[sr]).cuda()
        x32 = x16.float() * (1.0 / 32768.0)
        n_dev = torch.tensor(n, dtype=torch.int32, device='cuda')
        t_dev = torch.from_numpy(taps.copy()).cuda()
        y = torch.empty(B, n_out, device='cuda')
        for name, x in (('int16', x16), ('fp32', x32)):
            def launch():
                rc = lib.t2v_resample(t2v_hip._p(x), int(x.dtype == torch.int16), 1.0 / 32768.0, t2v_hip._p(n_dev), S, B,
                                      t2v_hip._p(t_dev), up, down, half, t2v_hip._p(y), n_out, t2v_hip._stream())
                assert rc == 0, rc
            k_us = event_us(launch, 10)
            floor = (x.numel() * x.element_size() + y.numel() * 4) / HBM_COPY_BYTES_PER_S * 1e6
            call = wall_us(lambda: t2v_hip.resample(x, n, sr, TARGET))
            yy, nn = t2v_hip.resample(x, n, sr, TARGET)
            tc = wall_us(lambda: t2v_hip.crop(yy, t2v_hip.trim_bounds(yy, nn), pcm16=True, return_stats=True))
            key = '%d_%s' % (sr, name)
            res.update({'kernel_%s_us' % key: round(k_us, 1), 'hbm_floor_%s_us' % key: round(floor, 2),
                        'call_%s_us' % key: round(call, 1), 'trim_crop_%s_us' % key: round(tc, 1),
                        'gfma_per_s_%s' % key: round(fmas / k_us * 1e-3, 1)})
            lines.append('%7d %6s %12.1f %12.2f %10.1f %12.1f %12.1f %14.1f %12.1f'
                         % (sr, name, k_us, floor, k_us / floor, fmas / k_us * 1e-3, call, tc, res['scipy_%d_s' % sr] * 1e6 / call))
        lines.append('%d Hz: scipy.signal.resample_poly, same window, float64, %d processes: %.3f s for the %d rows'
                     % (sr, workers, res['scipy_%d_s' % sr], B))

    # the rest of prepare_corpus on the 48 kHz rows: files and copies
    sr = RATES[0]
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, '%03d.wav' % b) for b in range(B)]
        for b, p in enumerate(paths):
            write(p, sr, data[sr][b])

        def timed(fn):
            ts = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts)

        res['read_s'] = round(timed(lambda: [read_wav(p) for p in paths]), 4)
        host = np.stack([read_wav(p)[1] for p in paths])
        res['upload_s'] = round(wall_us(lambda: torch.from_numpy(host).cuda()) * 1e-6, 5)
        yy, nn = t2v_hip.resample(torch.from_numpy(host).cuda(), [host.shape[1]] * B, sr, TARGET)
        pcm, counts, _ = t2v_hip.crop(yy, t2v_hip.trim_bounds(yy, nn), pcm16=True, return_stats=True)
        res['download_s'] = round(wall_us(lambda: pcm.cpu()) * 1e-6, 5)
        out = pcm.cpu().numpy()
        res['write_s'] = round(timed(lambda: [write(os.path.join(d, 'o%03d.wav' % b), TARGET, out[b, :counts[b]]) for b in range(B)]), 4)
    lines.append('the %d rows at %d Hz as files: read %.4f s, upload %.5f s, download of the int16 result %.5f s, write %.4f s'
                 % (B, sr, res['read_s'], res['upload_s'], res['download_s'], res['write_s']))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
