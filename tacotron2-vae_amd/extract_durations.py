"""Durations export: how long every symbol of every utterance of a filelist lasts, by forced alignment with the model itself.

    python extract_durations.py --load_path CKPT --filelist_path F --out D.npz [--weights raw|ema] [--max_step S] [--min_logp X]
                                [--batch_size N] [--hparams ...]

Filelist rows are `path|text|speaker|emotion`.  The model runs teacher-forced on each recording and the best monotonic path
through its attention alignments (`Synthesizer.durations`, `t2v_hip.mas`, csrc/durations.hip: steps of at most --max_step
symbols per frame, 1 by default) segments the recording into the text's own symbols: no outside aligner.  What a
non-autoregressive student is trained on, and a check of the corpus.

D.npz holds, row i for filelist row i: offsets (N + 1,) int64 into the ragged arrays; durations, starts and text_ids (offsets[-1],)
int32, the row's values at [offsets[i], offsets[i + 1]) (durations in frames, summing to n_frames[i]; starts the first frame
of each symbol; text_ids the symbol ids the text maps to); n_frames and n_symbols (N,) int32; align_logp (N,) float32, the mean
log attention weight along the path; paths (N,) str and max_step.  A row whose text has more symbols than its frames can reach
has no path: its durations and starts are all -1 and its align_logp is NaN; such rows are printed.

--min_logp X prints the rows whose align_logp lies below X as transcript suspects: a transcript that does not match its audio
has no path of high weight.  It has no default: no trained checkpoint exists here, so no threshold could be calibrated, and
a random-init model gives about -ln(symbols) everywhere; look at the distribution of align_logp of a trained model first
(DESIGN 7u).  Without it nothing is flagged; the values are in the file either way.
--weights ema aligns with the averaged weights of the checkpoint ('ema_state_dict', hparams.ema_decay > 0 in training).
"""
import argparse

import numpy as np

DEFAULT_BATCH_SIZE = 8
DEFAULT_MAX_STEP = 1


def build_arg_parser():
    p = argparse.ArgumentParser(description="filelist -> frames per symbol of every utterance by forced alignment (.npz)")
    p.add_argument('--load_path', required=True, help="checkpoint written by train.py")
    p.add_argument('--filelist_path', required=True, help="rows path|text|speaker|emotion")
    p.add_argument('--out', required=True, help="output .npz")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="rows per search call (the model runs one row at a time)")
    p.add_argument('--max_step', type=int, default=DEFAULT_MAX_STEP, metavar='S',
                   help="symbols the path may advance per frame, 1..3 (above 1 a symbol may be skipped and gets duration 0)")
    p.add_argument('--min_logp', type=float, default=None, metavar='X',
                   help="print the rows whose mean log weight along the path lies below X as transcript suspects (no default: "
                        "no threshold has been calibrated on a trained model)")
    p.add_argument('--hparams', default='', help="comma separated name=value overrides")
    from wavio import add_wav_arguments
    add_wav_arguments(p)
    from synthesizer import add_weights_argument
    add_weights_argument(p)
    return p


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if not 1 <= args.max_step <= 3:
        raise SystemExit("--max_step must be in 1..3")
    if args.min_logp is not None and not args.min_logp < 0.0:
        raise SystemExit("--min_logp is a mean log-probability: it must be a number below 0")
    return args


def pack(results, text_ids, paths, max_step):
    """the arrays of D.npz from `Synthesizer.durations` results, the rows' symbol ids and their paths"""
    counts = [r['n_symbols'] for r in results]
    offsets = np.zeros(len(results) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    durations = np.full(int(offsets[-1]), -1, dtype=np.int32)
    starts = np.full(int(offsets[-1]), -1, dtype=np.int32)
    ids = np.zeros(int(offsets[-1]), dtype=np.int32)
    for i, (r, q) in enumerate(zip(results, text_ids)):
        if len(q) != r['n_symbols']:
            raise ValueError("row %d: %d symbol ids for %d symbols" % (i, len(q), r['n_symbols']))
        ids[offsets[i]:offsets[i + 1]] = q
        if r['durations'] is not None:
            durations[offsets[i]:offsets[i + 1]] = r['durations']
            starts[offsets[i]:offsets[i + 1]] = r['starts']
    logp = np.array([np.nan if r['align_logp'] is None else r['align_logp'] for r in results], dtype=np.float32)
    return dict(offsets=offsets, durations=durations, starts=starts, text_ids=ids,
                n_frames=np.array([r['n_frames'] for r in results], dtype=np.int32), n_symbols=np.array(counts, dtype=np.int32),
                align_logp=logp, paths=np.array(paths), max_step=np.int32(max_step))


def suspects(align_logp, min_logp):
    """indices of the rows whose align_logp lies below min_logp (a NaN, a row without a path, is not one of them)"""
    return [i for i, v in enumerate(align_logp) if v < min_logp]


def main(argv=None):
    args = parse_args(argv)
    from evaluate import read_rows
    from hparams import create_hparams
    from synthesizer import Synthesizer, weights_option
    from text import text_to_sequence
    from wavio import wav_options
    hp = create_hparams()
    hp.sampling_rate = 16000                 # the reference's Synthesizer() overrides, as synthesizer.py's command line
    hp.max_decoder_steps = 600
    if args.hparams:
        hp.parse(args.hparams)
    syn = Synthesizer(hp, **wav_options(args)).load_checkpoint(args.load_path, **weights_option(args))
    rows = read_rows(args.filelist_path)
    results = syn.durations(rows, args.batch_size, args.max_step)
    out = pack(results, [text_to_sequence(r[1], ['korean_cleaners']) for r in rows], [r[0] for r in rows], args.max_step)
    np.savez(args.out, **out)
    for i, r in enumerate(results):
        if r['durations'] is None:
            print("no path: %s (%d symbols, %d frames)" % (rows[i][0], r['n_symbols'], r['n_frames']))
    if args.min_logp is not None:
        for i in suspects(out['align_logp'].tolist(), args.min_logp):
            print("transcript suspect: %s align_logp %.4f" % (rows[i][0], out['align_logp'][i]))
    print("%s: %d utterances" % (args.out, len(rows)))


if __name__ == "__main__":
    main()
