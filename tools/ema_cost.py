"""What the weight average (hparams.ema_decay > 0) costs a training step: bench.py's headline workload, timed by bench.py's own
run_workload, with ema_decay added to the hparams the engine is built from.  One JSON line.

    python tools/ema_cost.py --ema 0.9999 --steps 200 --warmup 20
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ema_cost.py --ema 0.9999 --steps 30 --warmup 5
        (kernel time of k_clip_adam<true> / k_clip_adam<false> in OUT/*/*_kernel_stats.csv; a run of its own: tracing slows the host)

One configuration per process (a third engine in one process replays its graph on other queues): alternate
`--ema 0` and `--ema 0.9999` runs from the shell to see the spread.  profiles/ema_cost.txt was made this way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tacotron2-vae_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ema', type=float, default=0.9999, help='hparams.ema_decay (0 = off)')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--settle', type=int, default=40)
    ap.add_argument('--no-graph', action='store_true')
    args = ap.parse_args()
    import bench
    import hparams as HP
    import t2v_hip
    t2v_hip.load_library()
    create = HP.create_hparams
    HP.create_hparams = lambda spec=None, verbose=False: create((spec + ',' if spec else '') + 'ema_decay=%r' % args.ema, verbose)
    engine, res = bench.run_workload(args, 1, 0, False, False, args.steps, args.warmup, not args.no_graph)
    opt = engine.optimizer
    print(json.dumps({'ema_decay': args.ema, 'ema_arena': opt.ema is not None, 'ms_per_step': res['ms_per_step'],
                      'value': res['value'], 'steps': args.steps, 'warmup': args.warmup, 'step_mode': res['step_mode'],
                      'arena_floats': opt.numel, 'final_loss': res['final_loss']}))


if __name__ == '__main__':
    main()
