#!/usr/bin/env python
"""Cost of the latent-space scores (t2v_hip.latent_neighbours, csrc/latent.hip) on one GPU.

    python tools/bench_latent_scores.py [--runs 7] [--out FILE]

For N = M = 1024, 4096 and 16384 random 32-d latents in four classes, leave-one-out, k = 5:
  kernels    device time of one `t2v_latent_neighbours` call (both kernels) on preallocated outputs, from a pair of events
             around `inner` back-to-back calls (inner chosen so that a window lasts about 50 ms), median of `runs` windows after
             a warm-up window;
  wrapper    host clock around `t2v_hip.latent_neighbours` ending in a synchronise: it adds the label check on the host, the
             finiteness check and the allocations;
  cdist+topk the yardstick on the same tensor: `torch.cdist(x, x)` followed by `topk(k + 1, largest=False)`, timed as the
             kernels are.  It yields only the neighbours (no class sums, no rank, ties in no defined order), and the N x N
             distance matrix goes through memory.
Next to the kernel time, its floor from the shapes: 2 D + 14 lane-operations per pair (D subtractions, D fused multiply-adds,
a square root, 8 class accumulators, the rank count, the exclusion and the list's compare) at 78.6e12 per second, the fp32
vector rate.  Prints the table and one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

SIZES = (1024, 4096, 16384)
D, K, CLASSES = 32, 5, 4
LANE_OPS_PER_S = 78.6e12
LANE_OPS_PER_PAIR = 2 * D + 14
WINDOW_MS = 50.0


def event_ms(fn, runs):
    """(median, min, max) device milliseconds of one fn() call, from windows of `inner` calls"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    inner = max(1, int(math.ceil(WINDOW_MS / max(e0.elapsed_time(e1), 1e-3))))
    ts = []
    for w in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:                                   # window 0 warms up
            ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts), inner


def host_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    lib = t2v_hip.load_library()
    p = t2v_hip._p
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'D': D, 'k': K, 'classes': CLASSES}
    lines = ['%6s %26s %10s %12s %24s %26s' % ('N = M', 'kernels ms (min..max)', 'x inner', 'VALU floor', 'wrapper ms (host clock)',
                                               'cdist + topk ms (min..max)')]
    for n in SIZES:
        rs = np.random.RandomState(n)
        lab_host = np.arange(n) % CLASSES
        x = torch.from_numpy((0.5 * rs.standard_normal((CLASSES, D))[lab_host] + rs.standard_normal((n, D))).astype(np.float32)).cuda()
        lab = torch.from_numpy(lab_host.astype(np.int32)).cuda()
        idx = torch.empty(n, K, device='cuda', dtype=torch.int32)
        dist = torch.empty(n, K, device='cuda')
        cs, cc = torch.empty(n, CLASSES, device='cuda'), torch.empty(n, CLASSES, device='cuda', dtype=torch.int32)
        scratch = torch.empty(lib.t2v_latent_scratch_bytes(n, n, CLASSES, K, 0), device='cuda', dtype=torch.uint8)

        def kernels():
            t2v_hip._check(lib.t2v_latent_neighbours(p(x), p(lab), n, D, CLASSES, None, n, None, None, K, 0, p(idx), p(dist), p(cs),
                                                     p(cc), None, p(scratch), t2v_hip._stream()), 't2v_latent_neighbours')

        def yardstick():
            return torch.cdist(x, x).topk(K + 1, dim=1, largest=False)
        kt = event_ms(kernels, args.runs)
        wt = host_ms(lambda: t2v_hip.latent_neighbours(x, lab_host, k=K, n_classes=CLASSES), args.runs)
        yt = event_ms(yardstick, args.runs)
        # the yardstick's neighbours (self dropped) against the kernel's, as a sanity check of both: not a test
        same = float((yardstick()[1][:, 1:].to(torch.int32) == idx).float().mean())
        floor_ms = LANE_OPS_PER_PAIR * float(n) * n / LANE_OPS_PER_S * 1e3
        res['N%d' % n] = {'kernels_ms': round(kt[0], 4), 'kernels_ms_min': round(kt[1], 4), 'kernels_ms_max': round(kt[2], 4),
                          'inner': kt[3], 'valu_floor_ms': round(floor_ms, 4), 'wrapper_ms': round(wt[0], 3),
                          'cdist_topk_ms': round(yt[0], 4), 'cdist_topk_ms_min': round(yt[1], 4), 'cdist_topk_ms_max': round(yt[2], 4),
                          'scratch_mib': round(scratch.numel() / 2.0 ** 20, 2), 'share_of_indices_equal_to_cdist_topk': round(same, 5)}
        lines.append('%6d %26s %10d %12.4f %24s %26s' % (n, '%.4f (%.4f..%.4f)' % kt[:3], kt[3], floor_ms, '%.3f (%.3f..%.3f)' % wt,
                                                         '%.4f (%.4f..%.4f)' % yt[:3]))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
