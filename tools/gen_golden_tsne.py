#!/usr/bin/env python
"""Write tests/golden/tsne.npz by running scikit-learn's exact t-SNE on a small synthetic set (test infrastructure).

    python tools/gen_golden_tsne.py [--out DIR]

Needs scikit-learn (the fixture was written with 1.7.2); nothing else in the project imports it.  Only numbers are
stored: the tests compare them with tests/tsne_ref.py, a numpy restatement, and with the HIP kernels.

Dataset: 600 points in 32 dimensions, four unit Gaussian clusters around centres drawn from N(0, I), seed 1234, label i % 4.
Stored:
    X (600, 32) f32, labels, perplexity
    init (600, 2) f32         scikit-learn's init='random' for random_state 0: 1e-4 * RandomState(0).standard_normal
    spread (600, 2) f32       a second map, 10 * RandomState(1).standard_normal
    p_i, p_j, p_val           _joint_probabilities(squared distances, 30) at 4096 sampled pairs i != j (RandomState(2))
    p_row_sums (600,) f64     row sums of the full matrix
    kl_init, grad_init, kl_spread, grad_spread, and the same with _x12   _kl_divergence at those maps with P and 12 P
    final_kl (5,)             kl_divergence_ of TSNE(method='exact', init='random', random_state=s), s = 0..4
    final_n_iter (5,)         their n_iter_ (scikit-learn may stop early; the HIP run never does)
    exact_seconds (5,)        wall time of each fit on this machine, threads as the environment sets them
    sklearn_version
"""
import argparse
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, SEED, PERPLEXITY, N_PAIRS = 600, 32, 1234, 30.0, 4096


def dataset():
    rs = np.random.RandomState(SEED)
    labels = np.arange(N) % 4
    centres = rs.standard_normal((4, D))
    return (centres[labels] + rs.standard_normal((N, D))).astype(np.float32), labels.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    import sklearn
    from scipy.spatial.distance import squareform
    from sklearn.manifold import TSNE
    from sklearn.manifold import _t_sne
    from sklearn.metrics import pairwise_distances

    X, labels = dataset()
    init = (1e-4 * np.random.RandomState(0).standard_normal(size=(N, 2))).astype(np.float32)
    spread = (10 * np.random.RandomState(1).standard_normal(size=(N, 2))).astype(np.float32)
    dist = pairwise_distances(X, metric='euclidean', squared=True)
    P = _t_sne._joint_probabilities(dist, PERPLEXITY, 0)          # condensed, float64
    Pd = squareform(P)
    rs = np.random.RandomState(2)
    p_i = rs.randint(0, N, size=N_PAIRS)
    p_j = (p_i + rs.randint(1, N, size=N_PAIRS)) % N
    out = dict(X=X, labels=labels, perplexity=np.float64(PERPLEXITY), init=init, spread=spread,
               p_i=p_i.astype(np.int16), p_j=p_j.astype(np.int16), p_val=Pd[p_i, p_j].astype(np.float32),
               p_row_sums=Pd.sum(axis=1), sklearn_version=np.array(sklearn.__version__))
    for name, y in (('init', init), ('spread', spread)):
        for tag, ex in (('', 1.0), ('_x12', 12.0)):
            kl, grad = _t_sne._kl_divergence(y.ravel().copy(), P * ex, 1, N, 2)
            out['kl_%s%s' % (name, tag)] = np.float64(kl)
            out['grad_%s%s' % (name, tag)] = grad.reshape(N, 2).astype(np.float32)
    final_kl, final_n_iter, secs = [], [], []
    for s in range(5):
        t0 = time.time()
        m = TSNE(n_components=2, perplexity=PERPLEXITY, method='exact', init='random', random_state=s).fit(X)
        secs.append(time.time() - t0)
        final_kl.append(m.kl_divergence_)
        final_n_iter.append(m.n_iter_)
        print('random_state %d: kl %.6f after %d iterations, %.1f s' % (s, final_kl[-1], final_n_iter[-1], secs[-1]))
    out.update(final_kl=np.array(final_kl), final_n_iter=np.array(final_n_iter), exact_seconds=np.array(secs))
    path = os.path.join(args.out, 'tsne.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
