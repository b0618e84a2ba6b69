#!/usr/bin/env python
"""Cost of the monotonic alignment search (t2v_hip.mas, csrc/durations.hip) next to the alignment statistics and a device copy
of the same tensor, and next to the decode call that feeds it, on one GPU.

    python tools/bench_durations.py [--runs 9] [--out profiles/durations_bench.txt]

Two shapes, every row at its full length: (8, 800, 555) and (64, 800, 555), koemo's longest text.  The rows are the softmax
rows with a ridge that walks the text of tools/bench_alignment.py.  Per shape, in one run and alternating: k_mas through the C
entry point with buffers allocated once (device events around `inner` back-to-back calls, the median of `runs` such
measurements after a warm-up), `t2v_hip.alignment_stats`' two kernels the same way, `alignments.clone()` the same way, and the
whole Python call of mas with host lists of lengths (wall time with a device synchronisation).  The search is a chain of N
dependent steps per row and a walk back of N dependent loads, so its time is set by N and not by the bytes; no target is set,
the ratios are the ones measured here.  A second run of k_mas with every row at 1 symbol (`one-symbol us`) keeps the N barriers
of the forward pass and the N dependent loads of the walk back and drops the column work: the share of the serial skeleton.
The yardstick of evaluate(durations=True): Decoder.inference_batch on 8 memories of 200 positions of a random-init model that
never stops (600 frames; wall time, median) against the whole Python call of mas on the alignments it returns.
Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SHAPES = ((8, 800, 555), (64, 800, 555))


def mas_only(lib, t2v_hip, A, n, L, max_step=1):
    """a closure that launches k_mas on buffers allocated here"""
    B, N, T_in = A.shape
    path = torch.empty(B, N, device='cuda', dtype=torch.int32)
    dur = torch.empty(B, T_in, device='cuda', dtype=torch.int32)
    sta = torch.empty(B, T_in, device='cuda', dtype=torch.int32)
    score = torch.empty(B, device='cuda')
    scratch = torch.empty(lib.t2v_mas_scratch_bytes(B, N, T_in), device='cuda', dtype=torch.uint8)
    p = t2v_hip._p

    def run():
        rc = lib.t2v_mas(p(A), A.stride(0), A.stride(1), p(n), p(L), B, N, T_in, max_step, p(path), N, p(dur), p(sta), T_in,
                         p(score), p(scratch), t2v_hip._stream())
        assert rc == 0, rc
    return run, scratch.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import bench_alignment as BA
    import hparams as HP
    import t2v_hip
    import train as TR
    lib = t2v_hip.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs}
    lines = ['%16s %10s %10s %12s %12s %10s %10s %12s %12s' % ('shape', 'MB read', 'mas us', 'align us', 'clone us', 'x align',
                                                                'x clone', 'one-symbol us', 'call us')]
    for B, N, T_in in SHAPES:
        A = BA.ridge_batch(B, N, T_in, B)
        n_list, L_list = [N] * B, [T_in] * B
        n = torch.tensor(n_list, dtype=torch.int32).cuda()
        L = torch.tensor(L_list, dtype=torch.int32).cuda()
        one = torch.ones(B, dtype=torch.int32).cuda()
        run, scratch_bytes = mas_only(lib, t2v_hip, A, n, L)
        walk, _ = mas_only(lib, t2v_hip, A, n, one)                  # one cell per frame: the barriers and the walk back remain
        align, _ = BA.kernels_only(lib, t2v_hip, A, n, L)
        m_us, a_us, c_us, w_us = BA.event_us([run, align, lambda: A.clone(), walk], args.runs, 20)
        call = BA.wall_us(lambda: t2v_hip.mas(A, n_list, L_list), args.runs)
        mb = A.numel() * 4 / 1e6
        tag = 'B%d_N%d_T%d' % (B, N, T_in)
        res.update({tag + '_mas_us': round(m_us, 2), tag + '_alignment_stats_us': round(a_us, 2), tag + '_clone_us': round(c_us, 2),
                    tag + '_mas_over_alignment_stats': round(m_us / a_us, 3), tag + '_mas_over_clone': round(m_us / c_us, 3),
                    tag + '_one_symbol_us': round(w_us, 2), tag + '_call_wall_us': round(call, 1),
                    tag + '_us_per_frame': round(m_us / N, 4), tag + '_scratch_MB': round(scratch_bytes / 1e6, 3)})
        lines.append('%16s %10.2f %10.2f %12.2f %12.2f %10.3f %10.3f %12.2f %12.1f'
                     % ((B, N, T_in), mb, m_us, a_us, c_us, m_us / a_us, m_us / c_us, w_us, call))
        del A, run, walk, align

    # the yardstick: the decode call that makes a group's alignments against the search through those alignments
    hp = HP.create_hparams()
    hp.sampling_rate, hp.max_decoder_steps = 16000, 600
    torch.manual_seed(hp.seed)
    dec = TR.load_model(hp).eval().decoder
    dec.gate_threshold = 1.0                                        # a random-init gate never reaches it: 600 frames per row
    g = torch.Generator().manual_seed(2)
    mem = (torch.randn(8, 200, 512, generator=g) * 0.5).cuda()
    lens = [200] * 8
    with torch.no_grad():
        dec_us = BA.wall_us(lambda: dec.inference_batch(mem, lens), max(5, args.runs // 2))
        _, _, al, n_frames = dec.inference_batch(mem, lens)
    n8 = n_frames.tolist()
    mas_us = BA.wall_us(lambda: t2v_hip.mas(al, n8, lens), args.runs)
    al_us = BA.wall_us(lambda: t2v_hip.alignment_stats(al, n8, lens), args.runs)
    res.update(decode_B8_wall_us=round(dec_us, 1), decode_B8_frames=n8, mas_of_its_output_wall_us=round(mas_us, 1),
               alignment_stats_of_its_output_wall_us=round(al_us, 1), mas_over_decode_B8=round(mas_us / dec_us, 6))
    lines.append('Decoder.inference_batch, 8 memories of 200 positions, %d..%d frames: %.1f us (wall)' % (min(n8), max(n8), dec_us))
    lines.append('mas of the alignments it returns %s: %.1f us (wall) = %.3f %% of the decode call (alignment_stats: %.1f us)'
                 % (tuple(al.shape), mas_us, 100 * mas_us / dec_us, al_us))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
