#!/usr/bin/env python
"""What the attention window of the free-running decode costs (Decoder.attention_window).

    python tools/bench_attention_window.py [--runs 5] [--reps 10] [--frames 400] [--legs none/1,3] [--pkg DIR] [--label TEXT] [--out FILE]

Two workloads on a seeded random-init decoder, the gate never firing, Prenet dropout on as at inference:
  * persistent:  B = 1, T_in = 200, `frames` frames as one persistent launch (Decoder.inference);
  * per-stage:   the B = 8, T_in = 84 group of lengths 84 80 71 66 50 37 20 5 on the launch-per-stage loop
                 (Decoder.inference_batch(persistent=False), one chunk).
The legs (window None and window (1, 3) by default) alternate in one process; a sample is `reps` decodes in a row, and a leg's
figure is the median of `runs` samples after one warm-up sample, with the smallest and largest sample next to it: their
distance is the run-to-run spread a difference has to be read against.  Per decoded frame the tool prints
  * device: the time between two device events around the decode loop's own launches (InferenceSession.run_persistent / .run);
  * wall:   the host clock around the whole call, ending in a device synchronise (session set-up, arenas and copies included).
--legs none measures window None alone and never touches Decoder.attention_window, and --pkg DIR imports the package from
another checkout (its library built): together they time a commit from before the window existed on the same machine."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = (84, 80, 71, 66, 50, 37, 20, 5)


def parse_legs(text):
    legs = []
    for part in text.split('/'):
        part = part.strip().lower()
        if part == 'none':
            legs.append(None)
        else:
            back, ahead = (int(x) for x in part.split(','))
            legs.append((back, ahead))
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help="decodes per timed sample")
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--legs', default='none/1,3', help="'/' separated: none or BACK,AHEAD")
    ap.add_argument('--pkg', default=os.path.join(ROOT, 'tacotron2-vae_amd'), help="package directory to import")
    ap.add_argument('--label', default='this commit', help="what --pkg holds, for the output")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    legs = parse_legs(args.legs)
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    import hparams as HP
    import model as M
    import t2v_hip
    assert torch.cuda.is_available(), "bench_attention_window needs a GPU"
    t2v_hip.load_library()
    hp = HP.create_hparams("max_decoder_steps=%d" % args.frames)
    torch.manual_seed(hp.seed)
    dec = M.Decoder(hp).cuda().eval()
    dec.gate_threshold = 1.0                                     # the gate never fires: every decode runs `frames` frames
    g = torch.Generator().manual_seed(11)
    mem1 = (torch.randn(1, 200, 512, generator=g) * 0.5).cuda()
    mem8 = (torch.randn(8, 84, 512, generator=g) * 0.5).cuda()

    # device events around the decode loop's own launches
    spans = []
    for attr in ('run_persistent', 'run'):
        def timed(self, *a, _f=getattr(t2v_hip.InferenceSession, attr), **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _f(self, *a, **kw)
            e1.record()
            spans.append((e0, e1))
            return r
        setattr(t2v_hip.InferenceSession, attr, timed)

    def persistent():
        mel = dec.inference(mem1)[0]
        assert mel.size(2) == args.frames
        assert dec._sess.persistent_supported() and not dec._sess.persistent_timed_out()

    def per_stage():
        n = dec.inference_batch(mem8, GROUP, chunk=args.frames, persistent=False)[3]
        assert n.tolist() == [args.frames] * 8

    def sample(fn):
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        dev = sum(e0.elapsed_time(e1) for e0, e1 in spans) * 1e-3
        assert len(spans) == args.reps, len(spans)
        per = 1e6 / (args.reps * args.frames)
        return dev * per, wall * per

    def set_leg(w):
        if w is not None or hasattr(dec, 'attention_window'):
            dec.attention_window = w

    res = {'device': torch.cuda.get_device_name(0), 'frames': args.frames, 'runs': args.runs, 'reps': args.reps,
           'package': args.label}
    lines = ['%s, %s: %d runs of %d decodes of %d frames per leg' % (args.label, res['device'], args.runs, args.reps, args.frames)]
    with torch.no_grad():
        for name, fn in (('persistent B=1 T_in=200', persistent), ('per-stage B=8 T_in=84', per_stage)):
            got = {repr(w): [] for w in legs}
            for w in legs:                                        # warm-up sample of every leg
                set_leg(w)
                sample(fn)
            for _ in range(args.runs):
                for w in legs:                                    # the legs alternate
                    set_leg(w)
                    got[repr(w)].append(sample(fn))
            for w in legs:
                dev, wall = [s[0] for s in got[repr(w)]], [s[1] for s in got[repr(w)]]
                key = '%s window %s' % (name, 'None' if w is None else '%d,%d' % w)
                res[key] = {'device_us_per_frame': [round(statistics.median(dev), 3), round(min(dev), 3), round(max(dev), 3)],
                            'wall_us_per_frame': [round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3)]}
                lines.append('%-24s window %-6s device %8.3f us/frame (min %8.3f max %8.3f)   wall %8.3f us/frame (min %8.3f max %8.3f)'
                             % (name, 'None' if w is None else '%d,%d' % w, statistics.median(dev), min(dev), max(dev),
                                statistics.median(wall), min(wall), max(wall)))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
