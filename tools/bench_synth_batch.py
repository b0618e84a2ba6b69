#!/usr/bin/env python
"""Batched vs sequential text-to-speech throughput on one GPU.

    python tools/bench_synth_batch.py [--n 32] [--runs 3] [--out FILE]

N sentences from tests/golden/koemo_sentences.txt.gz (every 200th line) go through a seeded random-init model (dropout
on, as at inference) whose gate bias is shifted so that the sentences stop at different frames within max_decoder_steps
(600).  Timed, each the median of `runs` passes over all N sentences after one warm-up pass:
  * sequential `Synthesizer.synthesize()` calls, and `synthesize_batch` with batch sizes 4 and 8,
  * mel only (no output file), and with the Griffin-Lim vocoder (60 iterations, one wav per sentence),
  * the decode loop alone: 8 utterances of one length decoded 400 frames as one B = 8 group on the launch-per-stage loop
    against 8 x B = 1 on the persistent kernel (us per decoded frame).
Prints the table and one JSON line; the recommended batch size is the fastest mel-only configuration."""
import argparse
import gzip
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


def sentences(n):
    with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'koemo_sentences.txt.gz'), 'rt', encoding='utf-8') as f:
        lines = [l.strip() for l in f if l.strip()]
    return lines[::200][:n]


def make_synth(tmp, gate_shift=0.0, vocoder=None):
    import hparams as HP
    import train as TR
    from synthesizer import Synthesizer
    hp = HP.create_hparams()
    hp.sampling_rate, hp.max_decoder_steps = 16000, 600
    torch.manual_seed(hp.seed)
    model = TR.load_model(hp)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd['decoder.gate_layer.linear_layer.bias'] += gate_shift
    ck = os.path.join(tmp, 'ck')
    torch.save({'iteration': 1, 'state_dict': sd, 'optimizer': {}, 'learning_rate': 1e-3}, ck)
    fl = os.path.join(tmp, 'refs_test.txt')
    g = torch.Generator().manual_seed(5)
    np.savez(Synthesizer.centroid_cache_path(ck, fl), zs=(torch.randn(8, hp.z_latent_dim, generator=g) * 0.3).numpy(),
             emotions=np.arange(8) % 4)
    return Synthesizer(hp).load(ck, vocoder=vocoder, filelist_path=fl)


def pick_gate_shift(texts, tmp):
    """a bias shift under which about half the sentences stop before frame 300 and most before 600 (the gate row does not
    feed back into the decode, so a shift moves every frame's logit by the same amount)"""
    syn = make_synth(tmp)
    dec = syn.model.decoder
    dec.gate_threshold = 1.0
    peaks = []
    with torch.no_grad():
        for t in texts:
            enc = syn.encode_text(t)
            _, gate, _ = dec.inference(enc + syn.style_vector(enc, False, None, (1, 0, 0, 0)))
            g = gate[0, :, 0].cpu()
            peaks.append(float(g[:300].max()))
    return -float(np.median(peaks))


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import t2v_hip
    t2v_hip.load_library()
    texts = sentences(args.n)
    lines, res = [], {'n_sentences': len(texts), 'device': torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        shift = pick_gate_shift(texts, tmp)
        res['gate_bias_shift'] = round(shift, 4)
        for voc in (None, 'griffin_lim'):
            syn = make_synth(tmp, shift, voc)
            paths = [os.path.join(tmp, '%d.wav' % i) for i in range(len(texts))] if voc else None

            def seq():
                return [syn.synthesize(t, None if paths is None else paths[i])[0].size(2) for i, t in enumerate(texts)]

            def bat(bs):
                def run():
                    n = []
                    for i0 in range(0, len(texts), bs):
                        outs = syn.synthesize_batch(texts[i0:i0 + bs], None if paths is None else paths[i0:i0 + bs])
                        n += [o[0].size(2) for o in outs]
                    return n
                return run
            tag = 'gl' if voc else 'mel'
            for name, fn in (('seq', seq), ('b4', bat(4)), ('b8', bat(8))):
                with torch.no_grad():
                    dt, frames = timed(fn, args.runs)
                res['%s_%s_utt_per_s' % (tag, name)] = round(len(texts) / dt, 2)
                res['%s_%s_frames_per_s' % (tag, name)] = round(sum(frames) / dt, 1)
                lines.append('%-4s %-4s %8.3f s  %7.2f utt/s  %9.1f frames/s' % (tag, name, dt, len(texts) / dt, sum(frames) / dt))
            res['frames'] = frames
        # the decode loop alone, fixed 400 frames: one B = 8 launch-per-stage group vs 8 x B = 1 persistent
        syn = make_synth(tmp, -1e3)
        dec = syn.model.decoder
        dec.max_decoder_steps = 400
        with torch.no_grad():
            enc = syn.encode_text(texts[0])
            mem = (enc + syn.style_vector(enc, False, None, (1, 0, 0, 0))).expand(8, -1, -1).contiguous()
            L = [mem.size(1)] * 8
            t8, _ = timed(lambda: dec.inference_batch(mem, L, persistent=False), args.runs)
            t1, _ = timed(lambda: [dec.inference(mem[b:b + 1]) for b in range(8)], args.runs)
        res['decode_B8_per_stage_us_per_frame'] = round(t8 / 400 * 1e6, 2)
        res['decode_8xB1_persistent_us_per_frame'] = round(t1 / 400 * 1e6, 2)
        lines.append('decode, 400 frames x 8 utterances: B=8 launch-per-stage %.2f us/frame, 8 x B=1 persistent %.2f us/frame'
                     % (t8 / 400 * 1e6, t1 / 400 * 1e6))
    best = max(('seq', 'b4', 'b8'), key=lambda k: res['mel_%s_utt_per_s' % k])
    res['recommended_batch_size'] = {'seq': 1, 'b4': 4, 'b8': 8}[best]
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
