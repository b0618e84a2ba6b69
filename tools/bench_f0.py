#!/usr/bin/env python
"""Cost of the YIN pitch tracker (t2v_hip.f0, csrc/f0.hip) next to the vocoder run that feeds it, on one GPU.

    python tools/bench_f0.py [--runs 7] [--out FILE]

Times f0 on 8, 64 and 1232 synthetic waveforms of koemo-like lengths (tools/bench_refenc_batch.py's log-normal set, mean
3.2 s; harmonic tones of 80-400 Hz plus a little noise, one zero-padded batch): device time from a pair of events around
`inner` back-to-back calls, median of `runs` such measurements after a warm-up, next to the VALU floor of the shape
(frames x 256 new samples x tau_max lags x 2 lane-operations at 256 CUs x 4 SIMDs x 16 lanes x 2 (packed) x 2.4 GHz) and
to the fp64 numpy reference (tests/yin_ref.py) on one 1.5 s and one 3.2 s waveform on this machine's CPU.
The yardstick of evaluate(prosody=True), in the same process: GriffinLimVocoder.batch on the mels of a group of 8 such
waveforms (wall time with a device synchronisation, median of `runs`) against f0 on the 8 waveforms it returns.
Whether pitch survives mel -> Griffin-Lim: 16 harmonic tones of known F0 (90-420 Hz, 2 s) through mel_spectrogram and the
vocoder; the error of the resynthesis' median F0 in semitones is the noise floor of f0_shift_st.
Prints the table and one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BATCHES = (8, 64, 1232)
LANE_OPS_PER_S = 256 * 4 * 16 * 2 * 2.4e9          # packed fp32 VALU operations per second, whole chip


def tones(lengths, seed, lo=80.0, hi=400.0):
    """(y (B, max) zero-padded device batch of five-harmonic tones plus noise of sigma 0.003, lengths, frequencies)"""
    g = torch.Generator().manual_seed(seed)
    B, S = len(lengths), int(max(lengths))
    freq = (lo + (hi - lo) * torch.rand(B, generator=g)).cuda()
    t = torch.arange(S, device='cuda', dtype=torch.float64)[None] / 16000.0
    y = torch.zeros(B, S, device='cuda', dtype=torch.float64)
    for k in range(1, 6):
        y += 0.6 ** (k - 1) * torch.sin(2 * math.pi * k * freq[:, None].double() * t + k)
    torch.manual_seed(seed)
    y = (0.15 * y).float() + 0.003 * torch.randn(B, S, device='cuda')
    n = torch.tensor([int(v) for v in lengths])
    y[torch.arange(S, device='cuda')[None] >= n.cuda()[:, None]] = 0.0
    return y.contiguous(), n.tolist(), freq.cpu().tolist()


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


def voiced_median(track):
    v = track[track > 0]
    return float(v.median()) if v.numel() else float('nan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be >= 5 (the median of fewer runs is not a measurement)")
    import t2v_hip
    import yin_ref
    from bench_refenc_batch import koemo_lengths
    from hparams import create_hparams
    from synthesizer import GriffinLimVocoder, Synthesizer
    t2v_hip.load_library()
    tau_min, tau_max = t2v_hip.f0_lags()
    res = {'device': torch.cuda.get_device_name(0), 'runs': args.runs, 'tau_min': tau_min, 'tau_max': tau_max}
    lines = ['%6s %10s %10s %12s %12s %12s %10s' % ('B', 'seconds', 'frames', 'us / call', 'us / wav', 'floor us', 'x floor')]
    all_lengths = koemo_lengths(max(BATCHES))
    for B in BATCHES:
        y, n, _ = tones(all_lengths[:B], B)
        frames = sum(k // 256 + 1 for k in n)
        us = event_us(lambda: t2v_hip.f0(y, n), args.runs, 3 if B > 100 else 10)
        floor = frames * 256.0 * tau_max * 2 / LANE_OPS_PER_S * 1e6
        res['f0_B%d_us' % B], res['f0_B%d_frames' % B], res['f0_B%d_floor_us' % B] = round(us, 1), frames, round(floor, 2)
        lines.append('%6d %10.1f %10d %12.1f %12.2f %12.2f %10.1f' % (B, sum(n) / 16000.0, frames, us, us / B, floor, us / floor))
        del y
    for sec in (1.5, 3.2):
        x = yin_ref.glide_signal(int(sec * 16000), 0)
        t0 = time.perf_counter()
        yin_ref.yin(x)
        dt = time.perf_counter() - t0
        res['numpy_fp64_%.1fs_wav_s' % sec] = round(dt, 4)
        lines.append('fp64 numpy reference, one %.1f s waveform on the CPU: %.3f s' % (sec, dt))

    # the yardstick: the Griffin-Lim call that makes a group's waveforms against the pitch tracks of those waveforms
    syn = Synthesizer(create_hparams())
    voc = GriffinLimVocoder(syn.stft)
    y8, n8, _ = tones(all_lengths[:8], 8)
    with torch.no_grad():
        mels, frames8 = syn._mels_of(y8, n8)
        np.random.seed(0)
        gl_us = wall_us(lambda: voc.batch(mels, frames8), args.runs)
        wavs = voc.batch(mels, frames8)
    y_syn = torch.zeros(8, max(w.numel() for w in wavs), device='cuda')
    for b, w in enumerate(wavs):
        y_syn[b, :w.numel()] = w
    n_syn = [w.numel() for w in wavs]
    f0_us = event_us(lambda: t2v_hip.f0(y_syn, n_syn), args.runs, 10)
    f0_wall = wall_us(lambda: t2v_hip.f0(y_syn, n_syn), args.runs)
    res.update(griffin_lim_B8_us=round(gl_us, 1), f0_of_its_output_B8_us=round(f0_us, 1), f0_of_its_output_B8_wall_us=round(f0_wall, 1),
               f0_over_griffin_lim_B8=round(f0_wall / gl_us, 5))
    lines.append('GriffinLimVocoder.batch, 8 mels of %d..%d frames: %.1f us (wall)' % (min(frames8), max(frames8), gl_us))
    lines.append('f0 of the 8 waveforms it returns: %.1f us (events), %.1f us (wall) = %.2f %% of the vocoder call'
                 % (f0_us, f0_wall, 100 * f0_wall / gl_us))

    # does pitch survive mel -> Griffin-Lim?
    yt, nt, freqs = tones([32000] * 16, 3, 90.0, 420.0)
    with torch.no_grad():
        mel_t, frames_t = syn._mels_of(yt, nt)
        np.random.seed(1)
        back = voc.batch(mel_t, frames_t)
    direct = t2v_hip.f0(yt, nt)
    resyn = t2v_hip.f0(torch.stack(back), [w.numel() for w in back])
    err_true, err_direct = [], []
    for b, f in enumerate(freqs):
        m_d, m_r = voiced_median(direct[b]), voiced_median(resyn[b])
        err_true.append(12 * math.log2(m_r / f))
        err_direct.append(12 * math.log2(m_r / m_d))
        lines.append('tone %6.1f Hz: tracked %7.2f Hz, after mel -> Griffin-Lim %7.2f Hz (%+.4f st), voiced %.2f -> %.2f'
                     % (f, m_d, m_r, err_direct[-1], float((direct[b] > 0).float().mean()), float((resyn[b] > 0).float().mean())))
    finite = [abs(e) for e in err_direct if math.isfinite(e)]
    res.update(resynthesis_tones=len(freqs), resynthesis_tones_tracked=len(finite),
               resynthesis_median_f0_err_st_mean=round(sum(finite) / max(len(finite), 1), 5),
               resynthesis_median_f0_err_st_max=round(max(finite) if finite else float('nan'), 5),
               resynthesis_vs_true_err_st_max=round(max(abs(e) for e in err_true if math.isfinite(e)) if finite else float('nan'), 5))
    lines.append('median-F0 error of the resynthesis: mean |e| %.4f st, max |e| %.4f st over %d of %d tones'
                 % (res['resynthesis_median_f0_err_st_mean'], res['resynthesis_median_f0_err_st_max'], len(finite), len(freqs)))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
