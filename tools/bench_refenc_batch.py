#!/usr/bin/env python
"""The centroid pass of Synthesizer.load, sequential against ragged batches, on one GPU.

    python tools/bench_refenc_batch.py [--n 1232] [--runs 3] [--batch_sizes 16,64] [--out FILE]

N synthetic 16 kHz int16 wavs with koemo-like lengths (log-normal around 3 s, 1..8 s, fixed seed) go through a seeded
random-init model.  Timed, each the median of `runs` passes over all N wavs after one warm-up pass:
  * read   : reading the N wavs (load_wav_to_torch), nothing else;
  * seq    : the B = 1 loop `load()` ran before the ragged path: vae_gst(load_mel(path)) and a host copy of z per wav;
  * bs<k>  : Synthesizer.latents(paths, batch_size=k) and one host copy of z;
each of seq / bs<k> twice: from disk (what load() does) and with the wavs already in memory (the GPU part: the front end,
the reference encoder and the copies, without file reading).  Prints the table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))


def koemo_lengths(n, seed=0, sr=16000):
    rng = np.random.RandomState(seed)
    sec = np.clip(np.exp(rng.normal(np.log(3.0), 0.35, size=n)), 1.0, 8.0)
    return (sec * sr).astype(np.int64)


def write_wavs(d, lengths, sr=16000):
    from scipy.io.wavfile import write
    rng = np.random.RandomState(1)
    paths = []
    for i, N in enumerate(lengths):
        t = np.arange(N) / sr
        x = 4000 * np.sin(2 * np.pi * rng.uniform(80, 400) * t) + 1500 * rng.randn(N)
        p = os.path.join(d, 'u%04d.wav' % i)
        write(p, sr, np.clip(x, -32768, 32767).astype(np.int16))
        paths.append(p)
    return paths


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


class in_memory(object):
    """synthesizer's wav reads served from a dict filled beforehand (the GPU part of a pass)"""

    def __init__(self, paths):
        import synthesizer as S
        self.S = S
        self.audio = {p: S.load_wav_to_torch(p) for p in paths}

    def __enter__(self):
        self.saved = self.S.load_wav_to_torch, self.S.wav_num_samples
        self.S.load_wav_to_torch = lambda p: self.audio[p]
        self.S.wav_num_samples = lambda p: self.audio[p][0].numel()

    def __exit__(self, *exc):
        self.S.load_wav_to_torch, self.S.wav_num_samples = self.saved


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=1232, help="wavs (the reference's default filelist has 1 232)")
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--batch_sizes', default='16,64')
    ap.add_argument('--out', default=None, help="also write the JSON line here")
    args = ap.parse_args(argv)
    import hparams as HP
    import train as TR
    from synthesizer import Synthesizer
    from utils import load_wav_to_torch
    hp = HP.create_hparams()
    hp.sampling_rate, hp.max_decoder_steps = 16000, 600
    torch.manual_seed(hp.seed)
    lengths = koemo_lengths(args.n)
    res = dict(n=args.n, seconds_mean=float(lengths.mean() / 16000), frames_max=int(lengths.max() // 256 + 1))
    with tempfile.TemporaryDirectory() as d:
        paths = write_wavs(d, lengths)
        ck = os.path.join(d, 'ck')
        torch.save({'iteration': 1, 'state_dict': TR.load_model(hp).state_dict(), 'optimizer': {}, 'learning_rate': 1e-3}, ck)
        syn = Synthesizer(hp).load_checkpoint(ck)

        def seq():
            with torch.no_grad():
                return np.concatenate([syn.model.vae_gst(syn.load_mel(p))[3].cpu().numpy() for p in paths])

        def batched(k):
            return lambda: syn.latents(paths, k)[3].cpu().numpy()

        res['read_s'] = timed(lambda: [load_wav_to_torch(p) for p in paths], args.runs)
        legs = [('seq', seq)] + [('bs%d' % int(k), batched(int(k))) for k in args.batch_sizes.split(',')]
        mem = in_memory(paths)
        for name, fn in legs:
            res[name + '_s'] = timed(fn, args.runs)
            with mem:
                res[name + '_gpu_s'] = timed(fn, args.runs)
        z_seq, z_bat = seq(), batched(64)()
        res['max_abs_dz'] = float(np.abs(z_seq - z_bat).max())
    print('%-6s %12s %14s' % ('', 'from disk s', 'wavs in memory s'))
    for name, _ in legs:
        print('%-6s %12.3f %14.3f   (%.2f ms per wav in memory)' % (name, res[name + '_s'], res[name + '_gpu_s'],
                                                                    1e3 * res[name + '_gpu_s'] / args.n))
    print('read   %12.3f' % res['read_s'])
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
