#!/usr/bin/env python
"""Cost of the DTW mel distance (t2v_hip.mel_dtw, csrc/dtw.hip) next to the decode it scores, on one GPU.

    python tools/bench_dtw.py [--runs 7] [--out FILE]

Times mel_dtw on random log-mels for B = 1, 8, 64 pairs at (Tx, Ty) = (400, 400), (600, 900), (2048, 2048): device time
from a pair of events around `inner` back-to-back calls, median of `runs` such measurements after a warm-up, in us per
call and per pair.  The yardstick, in the same process: `Decoder.inference_batch` decoding one group of 8 utterances for
600 frames (the random-init model of tools/bench_synth_batch.py with a gate that never fires), wall time with a device
synchronisation, median of `runs`.  Prints the table, the ratio "scoring a group of 8 at (600, 900) / decoding it" and
one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SHAPES = ((400, 400), (600, 900), (2048, 2048))
BATCHES = (1, 8, 64)


def dtw_us(B, tx, ty, runs, inner):
    import t2v_hip
    g = torch.Generator().manual_seed(B * 7919 + tx)
    x = (torch.randn(B, 80, tx, generator=g) * 2 - 4).cuda()
    y = (torch.randn(B, 80, ty, generator=g) * 2 - 4).cuda()
    nx, ny = torch.full((B,), tx, dtype=torch.int32), torch.full((B,), ty, dtype=torch.int32)
    t2v_hip.mel_dtw(x, nx, y, ny)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            t2v_hip.mel_dtw(x, nx, y, ny)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    from bench_synth_batch import make_synth, sentences, timed
    t2v_hip.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs}
    lines = ['%-14s %4s %12s %12s' % ('(Tx, Ty)', 'B', 'us / call', 'us / pair')]
    for tx, ty in SHAPES:
        for B in BATCHES:
            us = dtw_us(B, tx, ty, args.runs, 2 if tx > 1000 else 5)
            res['dtw_%dx%d_B%d_us' % (tx, ty, B)] = round(us, 1)
            lines.append('%-14s %4d %12.1f %12.1f' % ('(%d, %d)' % (tx, ty), B, us, us / B))
    with tempfile.TemporaryDirectory() as tmp:
        syn = make_synth(tmp, -1e3)
        dec = syn.model.decoder
        dec.max_decoder_steps = 600
        with torch.no_grad():
            enc = syn.encode_text(sentences(1)[0])
            mem = (enc + syn.style_vector(enc, False, None, (1, 0, 0, 0))).expand(8, -1, -1).contiguous()
            t8, out = timed(lambda: dec.inference_batch(mem, [mem.size(1)] * 8), args.runs)
        assert out[3].tolist() == [600] * 8
    res['decode_B8_600_frames_us'] = round(t8 * 1e6, 1)
    ratio = res['dtw_600x900_B8_us'] / (t8 * 1e6)
    res['dtw_over_decode_B8'] = round(ratio, 5)
    lines.append('inference_batch, 8 utterances x 600 frames: %.1f us' % (t8 * 1e6))
    lines.append('scoring that group at (600, 900): %.1f us = %.2f %% of decoding it' % (res['dtw_600x900_B8_us'], 100 * ratio))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
