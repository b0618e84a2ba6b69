#!/usr/bin/env python
"""Cost of the voice-quality kernel (t2v_hip.voice_quality, csrc/voice.hip) next to the pitch tracker's, and what the vocoder
leg of evaluate(voice=True) does to the descriptors, on one GPU.

    python tools/bench_voice.py [--runs 7] [--out FILE]

Times voice_quality and f0 on the 8, 64 and 1232 synthetic waveforms of tools/bench_f0.py (koemo-like lengths, harmonic tones
plus a little noise, one zero-padded batch): device time from a pair of events around `inner` back-to-back calls, median of
`runs` such measurements after a warm-up, next to the time to read every sample once at the 6.29 TB/s copy rate.
Whether the descriptors survive mel -> Griffin-Lim: the 16 harmonic tones of bench_f0.py (90-420 Hz, 2 s) through
mel_spectrogram and the vocoder; the shift of the median alpha_db, hammarberg_db, slope_db_khz and cpp_db over the counted
frames is the noise floor of alpha_shift_db and cpp_shift_db.
Prints the table and one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

COPY_BYTES_PER_S = 6.29e12
PLANES = ('alpha_db', 'hammarberg_db', 'slope_db_khz', 'cpp_db')


def medians(vq, n):
    """per row, the median of each of PLANES over the counted frames"""
    import t2v_hip
    frames = [k // 256 + 1 for k in n]
    keep = t2v_hip.voice_counted(vq.level_db, frames)
    return [{k: float(getattr(vq, k)[b][keep[b]].median()) for k in PLANES} for b in range(len(n))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    from bench_f0 import BATCHES, event_us, tones
    from bench_refenc_batch import koemo_lengths
    from hparams import create_hparams
    from synthesizer import GriffinLimVocoder, Synthesizer
    t2v_hip.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs}
    lines = ['%6s %10s %10s %12s %12s %12s %12s %10s' % ('B', 'seconds', 'frames', 'voice us', 'f0 us', 'voice / f0', 'floor us',
                                                         'x floor')]
    all_lengths = koemo_lengths(max(BATCHES))
    for B in BATCHES:
        y, n, _ = tones(all_lengths[:B], B)
        frames = sum(k // 256 + 1 for k in n)
        inner = 3 if B > 100 else 10
        us = event_us(lambda: t2v_hip.voice_quality(y, n), args.runs, inner)
        f0_us = event_us(lambda: t2v_hip.f0(y, n), args.runs, inner)
        floor = 4.0 * sum(n) / COPY_BYTES_PER_S * 1e6
        res.update({'voice_B%d_us' % B: round(us, 1), 'f0_B%d_us' % B: round(f0_us, 1), 'voice_B%d_frames' % B: frames,
                    'voice_B%d_floor_us' % B: round(floor, 2)})
        lines.append('%6d %10.1f %10d %12.1f %12.1f %12.2f %12.2f %10.1f' % (B, sum(n) / 16000.0, frames, us, f0_us, us / f0_us, floor,
                                                                             us / floor))
        del y

    # do the descriptors survive mel -> Griffin-Lim?
    syn = Synthesizer(create_hparams())
    voc = GriffinLimVocoder(syn.stft)
    yt, nt, freqs = tones([32000] * 16, 3, 90.0, 420.0)
    with torch.no_grad():
        mel_t, frames_t = syn._mels_of(yt, nt)
        np.random.seed(1)
        back = voc.batch(mel_t, frames_t)
    direct = medians(t2v_hip.voice_quality(yt, nt), nt)
    n_back = [w.numel() for w in back]
    resyn = medians(t2v_hip.voice_quality(torch.stack(back), n_back), n_back)
    for b, f in enumerate(freqs):
        lines.append('tone %6.1f Hz: ' % f + ', '.join('%s %+.2f -> %+.2f' % (k, direct[b][k], resyn[b][k]) for k in PLANES))
    for k in PLANES:
        d = [resyn[b][k] - direct[b][k] for b in range(len(freqs))]
        res['resynthesis_%s_shift_mean' % k] = round(float(np.mean(d)), 3)
        res['resynthesis_%s_shift_abs_max' % k] = round(float(np.max(np.abs(d))), 3)
        lines.append('%s after mel -> Griffin-Lim: mean shift %+.3f, mean |shift| %.3f, max |shift| %.3f over %d tones'
                     % (k, np.mean(d), np.mean(np.abs(d)), np.max(np.abs(d)), len(d)))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
