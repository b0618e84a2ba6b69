"""Score a checkpoint by free-running synthesis: every utterance of a filelist is synthesised from its text and compared
with its own recording by mel-spectral distortion with dynamic time warping (`Synthesizer.evaluate`, csrc/dtw.hip).

    python evaluate.py --load_path CKPT --filelist_path F --out OUT.json
                       [--batch_size N] [--condition ref|emotion] [--limit N] [--hparams ...]

Filelist rows are `path|text|speaker|emotion`.  --condition ref (default) takes the style from the row's own recording
(copy synthesis); --condition emotion takes the centroid of the row's emotion label (built from the filelist, or read from
its cache next to the checkpoint).  OUT.json holds {"summary": evaluation.summarize(rows), "rows": [...]}, row i for
filelist row i: path, dtw, n_frames, n_ref_frames, hit_max, emotion."""
import argparse
import json

DEFAULT_BATCH_SIZE = 8
CONDITIONS = ('ref', 'emotion')


def build_arg_parser():
    p = argparse.ArgumentParser(description="filelist -> DTW mel distance of free-running synthesis per utterance (.json)")
    p.add_argument('--load_path', required=True, help="checkpoint written by train.py")
    p.add_argument('--filelist_path', required=True, help="rows path|text|speaker|emotion")
    p.add_argument('--out', required=True, help="output .json")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="rows per synthesize_batch / mel_dtw call")
    p.add_argument('--condition', choices=CONDITIONS, default='ref', help="style from the row's recording or its emotion centroid")
    p.add_argument('--limit', type=int, default=None, help="score only the first N rows")
    p.add_argument('--hparams', default='', help="comma separated name=value overrides")
    return p


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if args.limit is not None and args.limit < 1:
        raise SystemExit("--limit must be >= 1")
    return args


def read_rows(path, limit=None):
    """the rows (audio_path, text, speaker, emotion id) of a filelist, in order; the paths and labels through
    extract_latents.read_filelist, so both commands take the same files"""
    from extract_latents import read_filelist
    paths, emotions = read_filelist(path)
    rows = []
    with open(path, encoding='utf-8') as f:
        for line in f:
            if line.strip():
                _, text, speaker, _ = line.strip().split("|")
                rows.append((paths[len(rows)], text, speaker, int(emotions[len(rows)])))
    return rows if limit is None else rows[:limit]


def main(argv=None):
    args = parse_args(argv)
    from evaluation import summarize
    from hparams import create_hparams
    from synthesizer import Synthesizer
    hp = create_hparams()
    hp.sampling_rate = 16000                 # the reference's Synthesizer() overrides, as synthesizer.py's command line
    hp.max_decoder_steps = 600
    if args.hparams:
        hp.parse(args.hparams)
    syn = Synthesizer(hp)
    if args.condition == 'emotion':
        syn.load(args.load_path, filelist_path=args.filelist_path)
    else:
        syn.load_checkpoint(args.load_path)
    rows = read_rows(args.filelist_path, args.limit)
    records = syn.evaluate(rows, args.batch_size, args.condition)
    summary = summarize(records)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump({'summary': summary, 'rows': [dict(r, path=row[0]) for r, row in zip(records, rows)]}, f, indent=1)
    print(json.dumps(summary, indent=1))
    print("%s: %d utterances" % (args.out, len(records)))


if __name__ == "__main__":
    main()
