#!/usr/bin/env python
"""What decoding along a duration plan costs (Decoder.inference(plan=, n_plan=)).

    python tools/bench_attention_plan.py [--runs 5] [--reps 10] [--frames 400] [--legs none/w1,3/p1,3] [--pkg DIR] [--label TEXT] [--out FILE]

The two workloads of tools/bench_attention_window.py on a seeded random-init decoder, the gate never firing, Prenet dropout on as
at inference:
  * persistent:  B = 1, T_in = 200, `frames` frames as one persistent launch (Decoder.inference);
  * per-stage:   the B = 8, T_in = 84 group of lengths 84 80 71 66 50 37 20 5 on the launch-per-stage loop
                 (Decoder.inference_batch(persistent=False), one chunk).
Legs: `none` (no constraint), `wB,A` (Decoder.attention_window = (B, A)) and `pB,A` (a plan that walks each item's text at an
even pace over the `frames` frames, plan_window = (B, A), plan_stop = 'gate').  They alternate in one process; a sample is `reps`
decodes in a row, and a leg's figure is the median of `runs` samples after one warm-up sample, with the smallest and largest
sample next to it: their distance is the run-to-run spread a difference has to be read against.  Per decoded frame the tool
prints
  * device: the time between two device events around the decode loop's own launches (InferenceSession.run_persistent / .run);
  * wall:   the host clock around the whole call, ending in a device synchronise (session set-up, the check of the plan, arenas
            and copies included).
--legs none/w1,3 never touches the plan arguments, and --pkg DIR imports the package from another checkout (its library built):
together they time a commit from before the plan existed on the same machine.
With a `p` leg the tool also times the length regulator (t2v_hip.duration_plan) at 8 rows of 555 symbols and a plan of `frames`
frames, device events around the call, against the decode it precedes."""
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
            legs.append(('none', None))
        else:
            back, ahead = (int(x) for x in part[1:].split(','))
            if part[0] not in 'wp':
                raise SystemExit("a leg is none, wBACK,AHEAD or pBACK,AHEAD, got %r" % part)
            legs.append(('window' if part[0] == 'w' else 'plan', (back, ahead)))
    return legs


def leg_name(leg):
    return 'none' if leg[1] is None else '%s %d,%d' % (leg[0], leg[1][0], leg[1][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10, help="decodes per timed sample")
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--legs', default='none/w1,3/p1,3', help="'/' separated: none, wBACK,AHEAD or pBACK,AHEAD")
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
    assert torch.cuda.is_available(), "bench_attention_plan needs a GPU"
    t2v_hip.load_library()
    hp = HP.create_hparams("max_decoder_steps=%d" % args.frames)
    torch.manual_seed(hp.seed)
    dec = M.Decoder(hp).cuda().eval()
    dec.gate_threshold = 1.0                                     # the gate never fires: every decode runs `frames` frames
    g = torch.Generator().manual_seed(11)
    mem1 = (torch.randn(1, 200, 512, generator=g) * 0.5).cuda()
    mem8 = (torch.randn(8, 84, 512, generator=g) * 0.5).cuda()

    def even_plan(lens):
        """every item's symbols at an even pace over the frames, through the length regulator"""
        dur = torch.zeros(len(lens), max(lens))
        for b, n in enumerate(lens):
            dur[b, :n] = args.frames / n
        return t2v_hip.duration_plan(dur.cuda(), list(lens), args.frames)

    plans = {}
    if any(kind == 'plan' for kind, _ in legs):
        plans = {'persistent': even_plan((200,)), 'per_stage': even_plan(GROUP)}
        assert plans['persistent'].n_plan.tolist() == [args.frames] and plans['per_stage'].n_plan.tolist() == [args.frames] * 8

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

    def plan_kw(leg, which):
        if leg[0] != 'plan':
            return {}
        return dict(plan=plans[which].plan, n_plan=plans[which].n_plan, plan_window=leg[1], plan_stop='gate')

    def persistent(leg):
        mel = dec.inference(mem1, **plan_kw(leg, 'persistent'))[0]
        assert mel.size(2) == args.frames
        assert dec._sess.persistent_supported() and not dec._sess.persistent_timed_out()

    def per_stage(leg):
        n = dec.inference_batch(mem8, GROUP, chunk=args.frames, persistent=False, **plan_kw(leg, 'per_stage'))[3]
        assert n.tolist() == [args.frames] * 8

    def sample(fn, leg):
        del spans[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn(leg)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        dev = sum(e0.elapsed_time(e1) for e0, e1 in spans) * 1e-3
        assert len(spans) == args.reps, len(spans)
        per = 1e6 / (args.reps * args.frames)
        return dev * per, wall * per

    def set_leg(leg):
        w = leg[1] if leg[0] == 'window' else None
        if w is not None or hasattr(dec, 'attention_window'):
            dec.attention_window = w

    res = {'device': torch.cuda.get_device_name(0), 'frames': args.frames, 'runs': args.runs, 'reps': args.reps,
           'package': args.label}
    lines = ['%s, %s: %d runs of %d decodes of %d frames per leg' % (args.label, res['device'], args.runs, args.reps, args.frames)]
    with torch.no_grad():
        for name, fn in (('persistent B=1 T_in=200', persistent), ('per-stage B=8 T_in=84', per_stage)):
            got = {leg_name(leg): [] for leg in legs}
            for leg in legs:                                      # warm-up sample of every leg
                set_leg(leg)
                sample(fn, leg)
            for _ in range(args.runs):
                for leg in legs:                                  # the legs alternate
                    set_leg(leg)
                    got[leg_name(leg)].append(sample(fn, leg))
            for leg in legs:
                dev, wall = [s[0] for s in got[leg_name(leg)]], [s[1] for s in got[leg_name(leg)]]
                res['%s %s' % (name, leg_name(leg))] = {
                    'device_us_per_frame': [round(statistics.median(dev), 3), round(min(dev), 3), round(max(dev), 3)],
                    'wall_us_per_frame': [round(statistics.median(wall), 3), round(min(wall), 3), round(max(wall), 3)]}
                lines.append('%-24s %-11s device %8.3f us/frame (min %8.3f max %8.3f)   wall %8.3f us/frame (min %8.3f max %8.3f)'
                             % (name, leg_name(leg), statistics.median(dev), min(dev), max(dev),
                                statistics.median(wall), min(wall), max(wall)))
        if plans:
            # the length regulator at 8 rows of 555 symbols, and the planned decode of 8 such texts it would precede
            lens = [555, 540, 500, 431, 377, 290, 120, 33]
            dur = torch.zeros(8, 555)
            for b, n in enumerate(lens):
                dur[b, :n] = args.frames / n
            dur = dur.cuda()
            rate = torch.full((8, 555), 1.0).cuda()
            L = torch.tensor(lens, dtype=torch.int32).cuda()
            for _ in range(3):
                t2v_hip.duration_plan(dur, L, args.frames, rate=rate)
            us = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    lib_call = t2v_hip.duration_plan(dur, L, args.frames, rate=rate)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / args.reps)
            assert lib_call.n_plan.tolist() == [args.frames] * 8
            mem555 = (torch.randn(8, 555, 512, generator=g) * 0.5).cuda()
            pl = t2v_hip.duration_plan(dur, L, args.frames, rate=rate)
            leg = ('plan', (1, 3))
            set_leg(leg)
            dec_us = []
            for i in range(3):
                del spans[:]
                n = dec.inference_batch(mem555, lens, chunk=args.frames, plan=pl.plan, n_plan=pl.n_plan, plan_window=(1, 3),
                                        plan_stop='gate')[3]
                torch.cuda.synchronize()
                assert n.tolist() == [args.frames] * 8
                dec_us.append(sum(e0.elapsed_time(e1) for e0, e1 in spans) * 1e3)
            res['duration_plan 8x555'] = {'us_per_call': [round(statistics.median(us), 2), round(min(us), 2), round(max(us), 2)],
                                          'decode_us': round(min(dec_us[1:]), 1)}
            lines.append('duration_plan (8, 555) symbols -> %d frames, per-symbol rate: %8.2f us per call with its read-back of n_plan '
                         '(min %8.2f max %8.2f); the planned decode of those 8 texts: %10.1f us (%.4f %%)'
                         % (args.frames, statistics.median(us), min(us), max(us), min(dec_us[1:]),
                            100 * statistics.median(us) / min(dec_us[1:])))
    text = '\n'.join(lines) + '\n' + json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
