"""Latent map: exact t-SNE of the latents that extract_latents.py wrote, the second figure of the reference README's
"Visualization" section (tsne.png): does the latent space separate neu / sad / ang / hap?

    python latent_map.py --latents OUT.npz [--key mus|zs|prosody] [--perplexity 30] [--n_iter 1000] [--seed 0]
                         --out MAP.npz [--png MAP.png]

MAP.npz holds map (N, 2), kl (the KL divergence of the final map), kl_trace (after 50, 100, ..., n_iter iterations) and the
emotions and paths of OUT.npz.  The map is computed on the GPU by `t2v_hip.tsne` (all pairs, no approximation; scikit-learn's
schedule for method='exact', init='random', random_state=seed, without its early stop); a run repeats to the bit.  --png
draws the README's figure: r / b / g / y for neu / sad / ang / hap, alpha 0.5, grid, legend.
"""
import argparse

import numpy as np

KEYS = ('mus', 'zs', 'prosody')
DEFAULT_KEY = 'mus'
DEFAULT_PERPLEXITY = 30.0
DEFAULT_N_ITER = 1000
COLOURS = (('r', 'neu'), ('b', 'sad'), ('g', 'ang'), ('y', 'hap'))      # label ids 0..3, the README's colours


def build_arg_parser():
    p = argparse.ArgumentParser(description="latents (.npz of extract_latents.py) -> 2-d t-SNE map (.npz, optional .png)")
    p.add_argument('--latents', required=True, help=".npz written by extract_latents.py")
    p.add_argument('--key', default=DEFAULT_KEY, choices=KEYS, help="which array of it to map")
    p.add_argument('--perplexity', type=float, default=DEFAULT_PERPLEXITY)
    p.add_argument('--n_iter', type=int, default=DEFAULT_N_ITER)
    p.add_argument('--seed', type=int, default=0, help="numpy RandomState seed of the initial map")
    p.add_argument('--out', required=True, help="output .npz")
    p.add_argument('--png', default=None, help="also draw the map, coloured by emotion")
    return p


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if not args.perplexity > 0:
        raise SystemExit("--perplexity must be > 0")
    if args.n_iter < 1:
        raise SystemExit("--n_iter must be >= 1")
    return args


def check_perplexity(perplexity, n):
    if not 3.0 * perplexity < n:
        raise SystemExit("--perplexity %g needs more than %d points (3 * perplexity < N), the file has %d"
                         % (perplexity, int(3 * perplexity), n))


def compute_map(x, perplexity=DEFAULT_PERPLEXITY, n_iter=DEFAULT_N_ITER, seed=0):
    """(map (N, 2), kl_trace) as numpy arrays of the rows of x (N, D), on cuda:0"""
    import torch
    import t2v_hip
    x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    y, trace = t2v_hip.tsne(x, perplexity=perplexity, n_iter=n_iter, seed=seed, return_trace=True)
    return y.cpu().numpy(), trace.cpu().numpy()


def plot_map(points, emotions, path):
    """the README's tsne figure; False (nothing written) without matplotlib"""
    from logger import _plots
    plt = _plots()
    if plt is None:
        return False
    points, emotions = np.asarray(points), np.asarray(emotions)
    fig, ax = plt.subplots(figsize=(12, 12))
    for i, (c, label) in enumerate(COLOURS):
        ax.scatter(points[emotions == i, 0], points[emotions == i, 1], c=c, label=label, alpha=0.5)
    ax.grid(True)
    ax.legend(loc='upper left')
    fig.savefig(path)
    plt.close(fig)
    return True


def main(argv=None):
    args = parse_args(argv)
    with np.load(args.latents) as f:
        x, emotions, paths = f[args.key], f['emotions'], f['paths']
    check_perplexity(args.perplexity, len(x))
    points, trace = compute_map(x, args.perplexity, args.n_iter, args.seed)
    np.savez(args.out, map=points, kl=trace[-1], kl_trace=trace, emotions=emotions, paths=paths)
    print("%s: %d points of %s, KL %.4f" % (args.out, len(points), args.key, trace[-1]))
    if args.png:
        if plot_map(points, emotions, args.png):
            print(args.png)
        else:
            print("%s not written: matplotlib is not installed" % args.png)


if __name__ == "__main__":
    main()
