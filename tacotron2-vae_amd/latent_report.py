"""Score the latent space of a checkpoint from recorded latents: do the emotions separate, and does the latent still matter?

    python latent_report.py --latents OUT.npz [--key mus|zs] [--k 5] --out REPORT.json

OUT.npz is what extract_latents.py wrote (mus, logvars, zs, emotions).  REPORT.json holds n, k, knn_accuracy (leave-one-out:
every utterance is classified by the vote of its k nearest other utterances, `t2v_hip.latent_neighbours`, csrc/latent.hip),
confusion (rows: the label, columns: the vote), silhouette_mean (scikit-learn's definition), by_emotion {name: n, knn_accuracy,
silhouette_mean}, active_units (latent dimensions whose mu has a variance above 0.01 over the corpus), kl_per_dim and kl_total
(the corpus mean of the KL term per dimension, and their sum).  Active units and KL always come from mus and logvars, whatever
--key is.  `prosody` is a linear map of z and is not offered as a key.  A posterior collapse shows as few active units, a KL
near 0 and a kNN accuracy near chance; the numbers compare checkpoints, precisions and KL-annealing schedules where the t-SNE
picture of latent_map.py only shows one."""
import argparse
import json

import numpy as np

KEYS = ('mus', 'zs')
DEFAULT_K = 5
MAX_K = 32                               # t2v_hip.LATENT_MAX_K


def build_arg_parser():
    p = argparse.ArgumentParser(description="recorded latents (.npz of extract_latents.py) -> kNN accuracy, silhouette, "
                                            "active units and KL per dimension (.json)")
    p.add_argument('--latents', required=True, help=".npz written by extract_latents.py")
    p.add_argument('--key', choices=KEYS, default='mus', help="the array whose neighbourhoods are scored")
    p.add_argument('--k', type=int, default=DEFAULT_K, help="neighbours of the vote (lowered to N - 1 for a smaller corpus)")
    p.add_argument('--out', required=True, help="output .json")
    return p


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if not 1 <= args.k <= MAX_K:
        raise SystemExit("--k must be in 1..%d" % MAX_K)
    return args


def main(argv=None):
    args = parse_args(argv)
    from latent_scores import corpus_report, summary_lines
    with np.load(args.latents) as f:
        missing = [name for name in (args.key, 'mus', 'logvars', 'emotions') if name not in f.files]
        if missing:
            raise SystemExit("%s holds no %s (is it an extract_latents.py file?)" % (args.latents, ', '.join(missing)))
        values, mus, logvars, emotions = f[args.key], f['mus'], f['logvars'], f['emotions']
    rep = corpus_report(values, emotions, mus, logvars, args.k)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(rep, f, indent=1)
    for line in summary_lines(rep):
        print(line)
    return rep


if __name__ == "__main__":
    main()
