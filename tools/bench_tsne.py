#!/usr/bin/env python
"""Cost of the exact t-SNE latent map (t2v_hip.tsne, csrc/tsne.hip) on one GPU.

    python tools/bench_tsne.py [--runs 5] [--out FILE]

For N = 1232, 6496 and 12000 random 32-d latents: device time of `tsne_affinities` and of the 1000-iteration run
(`t2v_tsne_run` on a P computed once), each from a pair of events around one call, median of `runs` after a warm-up call.
Next to each run time, the two floors of DESIGN 7f computed from the shapes: (a) the P stream, 4 N^2 bytes per iteration at
6.3 TB/s, (b) 20 lane-operations per pair at 78.6e12 per second (the fp32 vector rate, one lane-operation per FMA slot), and
the time per iteration.  Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

SIZES = (1232, 6496, 12000)
N_ITER = 1000
HBM_BYTES_PER_S = 6.3e12
LANE_OPS_PER_S = 78.6e12
LANE_OPS_PER_PAIR = 20


def event_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    lib = t2v_hip.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'n_iter': N_ITER}
    lines = ['%6s %14s %22s %12s %12s %12s' % ('N', 'affinities ms', '%d iterations ms' % N_ITER, 'us / iter', 'HBM floor', 'VALU floor')]
    for n in SIZES:
        x = torch.from_numpy(np.random.RandomState(n).standard_normal((n, 32)).astype(np.float32)).cuda()
        aff = event_ms(lambda: t2v_hip.tsne_affinities(x, 30.0), args.runs)
        P = t2v_hip.tsne_affinities(x, 30.0)
        y0 = t2v_hip.tsne_init(n, 0).cuda()
        y = torch.empty_like(y0)
        trace = torch.empty(N_ITER // 50, device='cuda')
        scratch = torch.empty(lib.t2v_tsne_scratch_bytes(n, 32), device='cuda', dtype=torch.uint8)
        p = t2v_hip._p

        def run():
            y.copy_(y0)
            t2v_hip._check(lib.t2v_tsne_run(p(P), p(y), n, N_ITER, t2v_hip.tsne_learning_rate(n), p(trace), p(scratch),
                                            t2v_hip._stream()), 't2v_tsne_run')
        it = event_ms(run, args.runs)
        assert bool(torch.isfinite(y).all())
        hbm_us = 4.0 * n * n / HBM_BYTES_PER_S * 1e6
        valu_us = LANE_OPS_PER_PAIR * float(n) * n / LANE_OPS_PER_S * 1e6
        res['N%d' % n] = {'affinities_ms': round(aff[0], 3), 'run_ms': round(it[0], 2), 'run_ms_min': round(it[1], 2),
                          'run_ms_max': round(it[2], 2), 'us_per_iter': round(it[0] * 1e3 / N_ITER, 2),
                          'hbm_floor_us_per_iter': round(hbm_us, 2), 'valu_floor_us_per_iter': round(valu_us, 2),
                          'final_kl': round(float(trace[-1]), 4)}
        lines.append('%6d %14.3f %22s %12.2f %12.2f %12.2f' % (n, aff[0], '%.2f (%.2f..%.2f)' % it, it[0] * 1e3 / N_ITER, hbm_us,
                                                              valu_us))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
