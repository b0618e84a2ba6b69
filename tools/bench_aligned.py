#!/usr/bin/env python
"""Cost of the frame-aligned scores (t2v_hip.aligned_scores, csrc/aligned.hip) next to mel_dtw and to the decode they score.

    python tools/bench_aligned.py [--runs 7] [--out FILE]

For B = 1, 8, 64 pairs at (Tx, Ty) = (400, 400), (600, 900), (2048, 2048), on random-walk cepstra and random F0 tracks: the
forward kernel (t2v_cep_dtw_forward: the DTW that stores its decisions), the walk plus the scores (t2v_cep_dtw_walk followed
by t2v_path_scores), the whole aligned_scores call, the two mel_cepstrum calls that feed it, and t2v_hip.mel_dtw on log-mels
of the same lengths in the same process.  Device time from a pair of events around `inner` back-to-back calls, median of
`runs` such measurements after a warm-up, in us per call.  The yardstick is bench_dtw.py's: `Decoder.inference_batch` decoding
one group of 8 utterances for 600 frames, wall time with a device synchronisation.  Prints the table, the share of decoding
that `--aligned` adds for a group of 8 at (600, 900) (cepstra + aligned_scores) and one JSON line."""
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


def event_us(fn, runs, inner):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(ts)


def shape_us(B, tx, ty, runs, inner):
    """us per call of (forward, walk + scores, aligned_scores, the two cepstra, mel_dtw) at one shape"""
    import t2v_hip
    lib = t2v_hip.load_library()
    p, st = t2v_hip._p, t2v_hip._stream
    g = torch.Generator().manual_seed(B * 7919 + tx)
    mx = (torch.randn(B, 80, tx, generator=g) * 2 - 4).cuda()
    my = (torch.randn(B, 80, ty, generator=g) * 2 - 4).cuda()
    cx = (torch.randn(B, 13, tx, generator=g) * 0.3).cumsum(2).cuda()
    cy = (torch.randn(B, 13, ty, generator=g) * 0.3).cumsum(2).cuda()
    fx = (torch.rand(B, tx, generator=g) * 440 + 60).cuda()
    fy = (torch.rand(B, ty, generator=g) * 440 + 60).cuda()
    nx, ny = torch.full((B,), tx, dtype=torch.int32), torch.full((B,), ty, dtype=torch.int32)
    nxd, nyd = nx.cuda(), ny.cuda()
    kmax = tx + ty - 1
    scratch = torch.empty(lib.t2v_cep_dtw_scratch_bytes(B, tx, ty), dtype=torch.uint8).cuda()
    dist, K = torch.empty(B).cuda(), torch.empty(B, dtype=torch.int32).cuda()
    path = torch.empty(B, kmax, 2, dtype=torch.int32).cuda()
    counts, sums = torch.empty(B, 4, dtype=torch.int32).cuda(), torch.empty(B, 8).cuda()

    def fwd():
        t2v_hip._check(lib.t2v_cep_dtw_forward(p(cx), p(nxd), tx, p(cy), p(nyd), ty, B, 13, p(dist), p(scratch), st()), 'forward')

    def back():
        t2v_hip._check(lib.t2v_cep_dtw_walk(p(nxd), tx, p(nyd), ty, B, p(scratch), p(K), p(path), kmax, st()), 'walk')
        t2v_hip._check(lib.t2v_path_scores(p(path), p(K), kmax, p(cx), p(nxd), tx, p(cy), p(nyd), ty, p(fx), tx, p(fy), ty, B, 13,
                                           p(counts), p(sums), st()), 'scores')

    def cep():
        t2v_hip.mel_cepstrum(mx, nx)
        t2v_hip.mel_cepstrum(my, ny)

    return (event_us(fwd, runs, inner), event_us(back, runs, inner),
            event_us(lambda: t2v_hip.aligned_scores(cx, nx, cy, ny, fx, fy), runs, inner), event_us(cep, runs, inner),
            event_us(lambda: t2v_hip.mel_dtw(mx, nx, my, ny), runs, inner))


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
    lines = ['%-14s %4s %12s %14s %14s %12s %12s' % ('(Tx, Ty)', 'B', 'forward us', 'walk+scores us', 'aligned_scores', 'cepstra us',
                                                    'mel_dtw us')]
    for tx, ty in SHAPES:
        for B in BATCHES:
            us = shape_us(B, tx, ty, args.runs, 2 if tx > 1000 else 5)
            for name, v in zip(('fwd', 'back', 'aligned', 'cepstra', 'mel_dtw'), us):
                res['%s_%dx%d_B%d_us' % (name, tx, ty, B)] = round(v, 1)
            lines.append('%-14s %4d %12.1f %14.1f %14.1f %12.1f %12.1f' % (('(%d, %d)' % (tx, ty), B) + us))
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
    added = res['aligned_600x900_B8_us'] + res['cepstra_600x900_B8_us']
    res['aligned_over_decode_B8'] = round(added / (t8 * 1e6), 5)
    res['mel_dtw_over_decode_B8'] = round(res['mel_dtw_600x900_B8_us'] / (t8 * 1e6), 5)
    res['walk_under_forward_everywhere'] = all(res['back_%dx%d_B%d_us' % (tx, ty, B)] < res['fwd_%dx%d_B%d_us' % (tx, ty, B)]
                                               for tx, ty in SHAPES for B in BATCHES)
    lines.append('inference_batch, 8 utterances x 600 frames: %.1f us' % (t8 * 1e6))
    lines.append('--aligned for that group at (600, 900): cepstra + aligned_scores = %.1f us = %.2f %% of decoding it (mel_dtw: %.2f %%)'
                 % (added, 100 * added / (t8 * 1e6), 100 * res['mel_dtw_over_decode_B8']))
    lines.append('walk + scores under the forward kernel at every shape: %s' % res['walk_under_forward_everywhere'])
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
