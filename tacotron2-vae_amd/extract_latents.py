"""Latent export: prosody, mu, logvar and z of every utterance of a filelist, for the plots of the reference README's
"Visualization" section: the scatter of two latent dimensions is the reader's to draw from OUT.npz, the t-SNE map is
latent_map.py's (or --tsne here).

    python extract_latents.py --load_path CKPT --filelist_path F --out OUT.npz [--batch_size N] [--hparams ...] [--tsne [KEY]]
                              [--weights raw|ema]
                              [--scores [KEY]] [--probe OUT.json [--probe_formant ST,...] [--probe_preserve_formants]]

Filelist rows are `path|text|speaker|emotion`.  OUT.npz holds, row i for filelist row i: prosody (N, E), mus, logvars,
zs (N, z_latent_dim), emotions (N,) int and paths (N,) str.  The wavs run through `Synthesizer.latents`: sorted by
length, in ragged batches of at most --batch_size, each row what model.vae_gst(load_mel(path)) gives for the wav alone.  --tsne [mus|zs|prosody] adds tsne (N, 2), the
map of that array by latent_map.compute_map with its defaults, and tsne_kl; without it the file is what it always was.
--scores [mus|zs] adds scores, the dict of latent_report.py (leave-one-out kNN accuracy, silhouette, active units, KL per
dimension) for that array as a JSON string; without it the file is what it always was.
--probe OUT.json also writes the latent probe (`Synthesizer.latent_probe` with its defaults): how far mu moves when
a clip's pitch, tempo or level alone is changed, against the distance between the emotions' centroids; OUT.npz is not
changed by it.  --probe_formant ST,... adds entries of kind 'formant', the spectral envelope alone moved by those semitones,
and --probe_preserve_formants makes the pitch entries move F0 alone: the plain pitch shift moves the formants
too, so only with it does the table tell pitch from timbre.  Both need --probe.
--weights ema encodes with the averaged weights of the checkpoint ('ema_state_dict', hparams.ema_decay > 0 in training).
"""
import argparse

import numpy as np

DEFAULT_BATCH_SIZE = 64


def build_arg_parser():
    p = argparse.ArgumentParser(description="filelist -> prosody / mu / logvar / z of every utterance (.npz)")
    p.add_argument('--load_path', required=True, help="checkpoint written by train.py")
    p.add_argument('--filelist_path', required=True, help="rows path|text|speaker|emotion")
    p.add_argument('--out', required=True, help="output .npz")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="wavs per ragged vae_gst call")
    p.add_argument('--hparams', default='', help="comma separated name=value overrides")
    p.add_argument('--tsne', nargs='?', const='mus', default=None, choices=('mus', 'zs', 'prosody'),
                   help="also store the t-SNE map of this array (default mus) as tsne, tsne_kl")
    p.add_argument('--scores', nargs='?', const='mus', default=None, choices=('mus', 'zs'),
                   help="also store the latent_report.py scores of this array (default mus) as a JSON string under scores")
    p.add_argument('--probe', default=None, metavar='OUT.json',
                   help="also write the latent probe: mean and median move of mu under single pitch, tempo and level changes")
    p.add_argument('--probe_formant', default=[], type=_semitone_list, metavar='ST,...',
                   help="with --probe: also shift the formants alone by these semitones (each in -12..12), entries of kind 'formant'")
    p.add_argument('--probe_preserve_formants', action='store_true',
                   help="with --probe: the pitch entries keep the formants in place (F0 alone)")
    from wavio import add_wav_arguments
    add_wav_arguments(p)
    from synthesizer import add_weights_argument
    add_weights_argument(p)
    return p


def _semitone_list(text):
    try:
        values = [float(x) for x in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a comma separated list of numbers" % (text,))
    if not values or any(not -12.0 <= v <= 12.0 for v in values):
        raise argparse.ArgumentTypeError("semitones must lie in -12..12, got %r" % (text,))
    return values


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if (args.probe_formant or args.probe_preserve_formants) and not args.probe:
        raise SystemExit("--probe_formant / --probe_preserve_formants change the latent probe: give --probe")
    return args


def read_filelist(path):
    """(paths, emotion ids) of the rows `path|text|speaker|emotion`"""
    paths, emotions = [], []
    with open(path, encoding='utf-8') as f:
        for line in f:
            if not line.strip():
                continue
            audio_path, _, _, emotion = line.strip().split("|")
            paths.append(audio_path)
            emotions.append(int(emotion))
    return paths, np.array(emotions, dtype=np.int64)


def main(argv=None):
    args = parse_args(argv)
    from hparams import create_hparams
    from synthesizer import Synthesizer, weights_option
    hp = create_hparams()
    hp.sampling_rate = 16000                 # the reference's Synthesizer() overrides, as synthesizer.py's command line
    hp.max_decoder_steps = 600
    if args.hparams:
        hp.parse(args.hparams)
    from wavio import wav_options
    syn = Synthesizer(hp, **wav_options(args)).load_checkpoint(args.load_path, **weights_option(args))
    paths, emotions = read_filelist(args.filelist_path)
    prosody, mu, logvar, z = (t.cpu().numpy() for t in syn.latents(paths, args.batch_size))
    out = dict(prosody=prosody, mus=mu, logvars=logvar, zs=z, emotions=emotions, paths=np.array(paths))
    if args.tsne:
        import latent_map
        latent_map.check_perplexity(latent_map.DEFAULT_PERPLEXITY, len(paths))
        points, trace = latent_map.compute_map(out[args.tsne])
        out.update(tsne=points, tsne_kl=trace[-1])
    if args.scores:
        import json
        from latent_scores import corpus_report
        out.update(scores=json.dumps(corpus_report(out[args.scores], emotions, mu, logvar)))
    np.savez(args.out, **out)
    if args.probe:
        import json
        probe = syn.latent_probe(paths, emotions.tolist(), batch_size=args.batch_size, formant=args.probe_formant,
                                 preserve_formants=args.probe_preserve_formants)
        with open(args.probe, 'w', encoding='utf-8') as f:
            json.dump(probe, f, indent=1)
        for r in probe['perturbations']:
            print("%s %+g: mean |dmu| %.4g (%s of the scale)" % (r['kind'], r['value'], r['mean'],
                                                                "n/a" if r['mean_rel'] is None else "%.3f" % r['mean_rel']))
    print("%s: %d utterances" % (args.out, len(paths)))


if __name__ == "__main__":
    main()
