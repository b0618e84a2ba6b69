#!/usr/bin/env python
"""Cost of the attention alignment statistics (t2v_hip.alignment_stats, csrc/align.hip) next to a device copy of the same
tensor and next to the decode call that feeds it, on one GPU.

    python tools/bench_alignment.py [--runs 9] [--out FILE]

Two shapes, every row at its full length so that the kernels read every byte a copy reads: (8, 600, 200), a group of
Synthesizer.evaluate at max_decoder_steps, and (64, 800, 555), a validation batch at koemo's longest text.  The rows are
softmax rows with a ridge that walks the text.  Per shape, in one run and alternating: the two kernels through the C entry
point with buffers allocated once (device events around `inner` back-to-back calls, median of `runs` such measurements after
a warm-up), `alignments.clone()` measured the same way, and the whole Python call with host lists of lengths (wall time with
a device synchronisation: allocations, the copy of the lengths and the launches).  The kernels read A once, so the copy,
which reads it once and writes it once, is the yardstick; the ratio is the one measured here, no target is set.
The yardstick of evaluate(alignment=True), in the same process: Decoder.inference_batch on 8 memories of 200 positions of a
random-init model that never stops (600 frames; wall time with a synchronisation, median of `runs`) against the whole Python
call on the alignments it returns.
Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

SHAPES = ((8, 600, 200), (64, 800, 555))


def ridge_batch(B, N, T_in, seed):
    """(B, N, T_in) float32 softmax rows on the device: unit Gaussian logits plus a ridge of height 6 walking the text"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    logits = torch.randn(B, N, T_in, device='cuda', generator=g)
    centre = torch.linspace(0, T_in - 1, N, device='cuda')[None, :, None]
    j = torch.arange(T_in, device='cuda', dtype=torch.float32)[None, None, :]
    return torch.softmax(logits + 6.0 * torch.exp(-0.5 * ((j - centre) / 1.5) ** 2), dim=2).contiguous()


def event_us(fns, runs, inner):
    """median device time per call of each function of `fns`, measured alternately"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return [statistics.median(t) for t in ts]


def wall_us(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def kernels_only(lib, t2v_hip, A, n, L):
    """a closure that launches the two kernels on buffers allocated here"""
    B, N, T_in = A.shape
    path = torch.empty(B, N, device='cuda', dtype=torch.int32)
    mass = torch.empty(B, T_in, device='cuda')
    focus = torch.empty(B, device='cuda')
    stats = torch.empty(B, 8, device='cuda', dtype=torch.int32)
    scratch = torch.empty(lib.t2v_alignment_scratch_bytes(B, N, T_in), device='cuda', dtype=torch.uint8)
    p = t2v_hip._p

    def run():
        rc = lib.t2v_alignment_stats(p(A), A.stride(0), A.stride(1), p(n), p(L), B, N, T_in, 3, 0.5, p(path), N, p(mass), T_in,
                                     p(focus), p(stats), p(scratch), t2v_hip._stream())
        assert rc == 0, rc
    return run, scratch.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import hparams as HP
    import t2v_hip
    import train as TR
    lib = t2v_hip.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'frames_per_workgroup': t2v_hip.ALIGN_FRAMES}
    lines = ['%16s %10s %12s %12s %10s %12s %12s' % ('shape', 'MB read', 'kernels us', 'clone us', 'x clone', 'GB/s read', 'call us')]
    for B, N, T_in in SHAPES:
        A = ridge_batch(B, N, T_in, B)
        n_list, L_list = [N] * B, [T_in] * B
        n = torch.tensor(n_list, dtype=torch.int32).cuda()
        L = torch.tensor(L_list, dtype=torch.int32).cuda()
        run, scratch_bytes = kernels_only(lib, t2v_hip, A, n, L)
        inner = 1000 if A.numel() < (1 << 22) else 100
        k_us, c_us = event_us([run, lambda: A.clone()], args.runs, inner)
        call = wall_us(lambda: t2v_hip.alignment_stats(A, n_list, L_list), args.runs)
        mb = A.numel() * 4 / 1e6
        tag = 'B%d_N%d_T%d' % (B, N, T_in)
        res.update({tag + '_kernels_us': round(k_us, 2), tag + '_clone_us': round(c_us, 2), tag + '_kernels_over_clone': round(k_us / c_us, 3),
                    tag + '_read_GBps': round(mb * 1e-3 / (k_us * 1e-6), 1), tag + '_call_wall_us': round(call, 1),
                    tag + '_scratch_MB': round(scratch_bytes / 1e6, 3)})
        lines.append('%16s %10.2f %12.2f %12.2f %10.3f %12.1f %12.1f' % ((B, N, T_in), mb, k_us, c_us, k_us / c_us,
                                                                         mb * 1e-3 / (k_us * 1e-6), call))
        del A, run

    # the yardstick: the decode call that makes a group's alignments against the statistics of those alignments
    hp = HP.create_hparams()
    hp.sampling_rate, hp.max_decoder_steps = 16000, 600
    torch.manual_seed(hp.seed)
    dec = TR.load_model(hp).eval().decoder
    dec.gate_threshold = 1.0                                        # a random-init gate never reaches it: 600 frames per row
    g = torch.Generator().manual_seed(2)
    mem = (torch.randn(8, 200, 512, generator=g) * 0.5).cuda()
    lens = [200] * 8
    with torch.no_grad():
        dec_us = wall_us(lambda: dec.inference_batch(mem, lens), max(5, args.runs // 2))
        _, _, al, n_frames = dec.inference_batch(mem, lens)
    n8 = n_frames.tolist()
    al_us = wall_us(lambda: t2v_hip.alignment_stats(al, n8, lens), args.runs)
    res.update(decode_B8_wall_us=round(dec_us, 1), decode_B8_frames=n8, alignment_of_its_output_wall_us=round(al_us, 1),
               alignment_over_decode_B8=round(al_us / dec_us, 6))
    lines.append('Decoder.inference_batch, 8 memories of 200 positions, %d..%d frames: %.1f us (wall)' % (min(n8), max(n8), dec_us))
    lines.append('alignment_stats of the alignments it returns %s: %.1f us (wall) = %.3f %% of the decode call'
                 % (tuple(al.shape), al_us, 100 * al_us / dec_us))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
