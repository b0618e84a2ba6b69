#!/usr/bin/env python
"""The phase start from magnitudes (t2v_hip.spsi_phase, vocoder 'spsi') on one GPU: what it costs and what it keeps.

    python tools/bench_phase_init.py [--runs 20] [--warmup 3] [--out FILE]

(a) the two kernels alone (k_spsi_scan + k_spsi_assign, one t2v_hip.spsi_phase call on magnitudes that are on the device) at
    (B, T) = (1, 600) and (8, 600): the median over `runs` event-timed calls after warm-up.
(b) the whole vocoder call, GriffinLimVocoder.batch on device mels, for 'griffin_lim', 'griffin_lim_fast' and 'spsi' in one
    process: host wall-clock around a call that ends in a device synchronise, so the np.random draw and the copy of the drawn
    phases to the device are inside for the first two; and the draw alone (host, no device work) beside them.
(c) does pitch survive mel -> vocoder?  DESIGN 7g's 16 five-harmonic tones (tools/bench_f0.py, 91-383 Hz, 2 s) and the eight
    low tones of DESIGN 7r (70-160 Hz, amplitudes 1 / k) through the mel front end, the vocoder and t2v_hip.f0: per tone the
    voiced share of the resynthesis (8 frames dropped at each end) and the shift of its median F0 in semitones, for
    'griffin_lim_fast', 'spsi', and init='spsi' followed by 4, 16 and 60 fast iterations; np.random.seed(1) before each.
Prints the tables and one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

LOW_TONES = (70.0, 80.0, 91.0, 100.0, 110.0, 125.0, 139.0, 160.0)
EDGE = 8


def wall_ms(fn, runs, warmup):
    """median host wall-clock of fn() + synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def low_tones(seconds=2.0):
    """(y (8, S) device batch of five-harmonic tones with amplitudes 1 / k scaled by 0.15, sample counts, frequencies)"""
    S = int(seconds * 16000)
    t = torch.arange(S, device='cuda', dtype=torch.float64)[None] / 16000.0
    f = torch.tensor(LOW_TONES, device='cuda', dtype=torch.float64)[:, None]
    y = sum(torch.sin(2 * math.pi * k * f * t) / k for k in range(1, 6))
    return (0.15 * y).float().contiguous(), [S] * len(LOW_TONES), list(LOW_TONES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    from bench_f0 import tones, voiced_median
    from bench_vocoder import time_ms
    from hparams import create_hparams
    from synthesizer import VOCODERS, GriffinLimVocoder, Synthesizer
    syn = Synthesizer(create_hparams())
    taco = syn.stft
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs}
    lines = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for B, T in ((1, 600), (8, 600)):
        tag = 'B%d_T%d' % (B, T)
        mag = torch.rand(B, 513, T, device='cuda', generator=g)
        mel = torch.log(torch.clamp(taco.mel_basis.cuda() @ mag, min=1e-5))
        lengths = [T] * B
        res[tag + '_spsi_kernels_ms'] = round(time_ms(lambda: t2v_hip.spsi_phase(mag), args.runs, args.warmup), 4)
        t0 = time.perf_counter()
        for _ in range(5):
            for b in range(B):
                np.angle(np.exp(2j * np.pi * np.random.rand(1, 513, T)))
        res[tag + '_host_draw_ms'] = round(1e3 * (time.perf_counter() - t0) / 5, 3)
        for name in VOCODERS:
            voc = GriffinLimVocoder.named(name, taco)
            res['%s_vocoder_%s_wall_ms' % (tag, name)] = round(wall_ms(lambda: voc.batch(mel, lengths), args.runs, args.warmup), 3)
        lines.append('%s: spsi_phase (two kernels, event-timed) %.4f ms; the host draw of the random start %.3f ms; whole vocoder '
                     'call, host wall-clock: %s' % (tag, res[tag + '_spsi_kernels_ms'], res[tag + '_host_draw_ms'], ', '.join(
                         '%s %.3f ms' % (name, res['%s_vocoder_%s_wall_ms' % (tag, name)]) for name in VOCODERS)))

    combos = [('griffin_lim_fast', lambda: GriffinLimVocoder.named('griffin_lim_fast', taco)),
              ('spsi', lambda: GriffinLimVocoder.named('spsi', taco))]
    for n in (4, 16, 60):
        combos.append(('spsi+fgl%d' % n, lambda n=n: GriffinLimVocoder(taco, n_iters=n, momentum=0.99, inversion='nnls', init='spsi')))
    for title, (yt, nt, freqs) in (('7g', tones([32000] * 16, 3, 90.0, 420.0)), ('low', low_tones())):
        direct = t2v_hip.f0(yt, nt)
        with torch.no_grad():
            mel_t, frames_t = syn._mels_of(yt, nt)
        table = {}
        for name, make in combos:
            np.random.seed(1)
            with torch.no_grad():
                back = make().batch(mel_t, frames_t)
            resyn = t2v_hip.f0(torch.stack(back), [w.numel() for w in back])
            for b in range(len(freqs)):
                d, r = direct[b, EDGE:direct.size(1) - EDGE], resyn[b, EDGE:resyn.size(1) - EDGE]
                m_d, m_r = voiced_median(d), voiced_median(r)
                shift = 12 * math.log2(m_r / m_d) if m_r == m_r and m_d == m_d else float('nan')
                table[(name, b)] = (float((r > 0).float().mean()), shift)
        lines.append('%s tones: voiced share and median shift in semitones' % title)
        lines.append('%8s |' % 'tone Hz' + '|'.join(' %20s ' % name for name, _ in combos))
        for b in sorted(range(len(freqs)), key=lambda i: freqs[i]):
            lines.append('%8.1f |' % freqs[b] + '|'.join('      %6.2f  %+8.3f ' % table[(name, b)] for name, _ in combos))
        for name, _ in combos:
            v = [table[(name, b)] for b in range(len(freqs))]
            fin = [abs(s) for _, s in v if math.isfinite(s)]
            key = '%s_%s' % (title, name)
            res[key + '_voiced_share_mean'] = round(sum(x for x, _ in v) / len(v), 4)
            res[key + '_tones_over_half_voiced'] = sum(1 for x, _ in v if x >= 0.5)
            res[key + '_abs_shift_st_mean'] = round(sum(fin) / max(len(fin), 1), 4)
            res[key + '_abs_shift_st_max'] = round(max(fin), 4) if fin else None
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
