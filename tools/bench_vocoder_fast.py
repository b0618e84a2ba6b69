#!/usr/bin/env python
"""The vocoder-quality options against the defaults on one GPU: timings, and whether pitch survives mel -> vocoder.

    python tools/bench_vocoder_fast.py [--runs 20] [--warmup 3] [--out FILE]

Timings, at the batches tools/bench_vocoder.py uses ((B, T) = (1, 600) and (8, 600), 60 Griffin-Lim iterations), each the
median over `runs` event-timed calls after warm-up, old against new in the same process:
  the inversion alone      TacotronSTFT.mel_to_magnitude, method 'pinv' against 'nnls' (100 steps);
  the whole vocoder call   mel_to_magnitude + audio_processing.griffin_lim with the initial angles already on the device (the
                           host RNG is not timed): pinv + momentum 0 against nnls + momentum 0.99.
The pitch-survival experiment of DESIGN 7g with all four combinations (pinv / nnls x momentum 0 / 0.99): the 16 five-harmonic
tones of tools/bench_f0.py (91-383 Hz, 2 s), 60 iterations, np.random.seed(1) before every combination; per tone the voiced
share of the resynthesis and the shift of its median F0 in semitones.  Prints the table and one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

COMBOS = (('pinv', 0.0), ('pinv', 0.99), ('nnls', 0.0), ('nnls', 0.99))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import t2v_hip
    from audio_processing import griffin_lim
    from bench_f0 import tones, voiced_median
    from bench_vocoder import time_ms
    from hparams import create_hparams
    from synthesizer import GriffinLimVocoder, Synthesizer
    syn = Synthesizer(create_hparams())
    taco = syn.stft
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs}
    lines = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for B, T in ((1, 600), (8, 600)):
        mag = torch.rand(B, 513, T, device='cuda', generator=g)
        mel = torch.log(torch.clamp(taco.mel_basis.cuda() @ mag, min=1e-5))
        angles = (torch.rand(B, 513, T, device='cuda', generator=g) * 2 - 1) * 3.14159265
        tag = 'B%d_T%d' % (B, T)
        res[tag + '_pinv_ms'] = round(time_ms(lambda: taco.mel_to_magnitude(mel), args.runs, args.warmup), 4)
        res[tag + '_nnls100_ms'] = round(time_ms(lambda: taco.mel_to_magnitude(mel, method='nnls', n_iters=100), args.runs, args.warmup), 4)
        res[tag + '_vocoder_pinv_gl60_ms'] = round(time_ms(
            lambda: griffin_lim(taco.mel_to_magnitude(mel), taco.stft_fn, 60, angles=angles), args.runs, args.warmup), 4)
        res[tag + '_vocoder_nnls_fgl60_ms'] = round(time_ms(
            lambda: griffin_lim(taco.mel_to_magnitude(mel, method='nnls', n_iters=100), taco.stft_fn, 60, angles=angles, momentum=0.99),
            args.runs, args.warmup), 4)
        res[tag + '_gl60_ms'] = round(time_ms(lambda: griffin_lim(mag, taco.stft_fn, 60, angles=angles), args.runs, args.warmup), 4)
        res[tag + '_fgl60_ms'] = round(time_ms(lambda: griffin_lim(mag, taco.stft_fn, 60, angles=angles, momentum=0.99), args.runs, args.warmup), 4)
        lines.append('%s: inversion pinv %.4f ms, nnls(100) %.4f ms; Griffin-Lim 60: plain %.4f ms, momentum 0.99 %.4f ms; whole call: '
                     'old %.4f ms, new %.4f ms' % (tag, res[tag + '_pinv_ms'], res[tag + '_nnls100_ms'], res[tag + '_gl60_ms'],
                                                   res[tag + '_fgl60_ms'], res[tag + '_vocoder_pinv_gl60_ms'], res[tag + '_vocoder_nnls_fgl60_ms']))

    # does pitch survive mel -> vocoder?  (DESIGN 7g's experiment, four ways)
    yt, nt, freqs = tones([32000] * 16, 3, 90.0, 420.0)
    direct = t2v_hip.f0(yt, nt)
    with torch.no_grad():
        mel_t, frames_t = syn._mels_of(yt, nt)
    table = {}
    for inv, mom in COMBOS:
        voc = GriffinLimVocoder(taco, n_iters=60, momentum=mom, inversion=inv)
        np.random.seed(1)
        with torch.no_grad():
            back = voc.batch(mel_t, frames_t)
        resyn = t2v_hip.f0(torch.stack(back), [w.numel() for w in back])
        for b, f in enumerate(freqs):
            m_d, m_r = voiced_median(direct[b]), voiced_median(resyn[b])
            shift = 12 * math.log2(m_r / m_d) if m_r == m_r and m_d == m_d else float('nan')
            table[(inv, mom, b)] = (float((resyn[b] > 0).float().mean()), shift)
    lines.append('%8s |' % 'tone Hz' + '|'.join(' %s m=%.2f voiced  shift st ' % c for c in COMBOS))
    for b in sorted(range(len(freqs)), key=lambda i: freqs[i]):
        lines.append('%8.1f |' % freqs[b] + '|'.join('      %11.2f  %+8.3f ' % table[c + (b,)] for c in COMBOS))
    for inv, mom in COMBOS:
        v = [table[(inv, mom, b)] for b in range(len(freqs))]
        fin = [abs(s) for _, s in v if math.isfinite(s)]
        key = '%s_m%02d' % (inv, round(100 * mom))
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
