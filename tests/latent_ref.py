"""The contract of t2v_hip.latent_neighbours (include/t2vae.h, csrc/latent.hip) restated in numpy, for the CPU and GPU tests.
Every function takes a dtype: float64 is the reference, float32 the yardstick that says what single precision costs on the
same formulas.

    d2(i, j)     sum_c (q_ic - r_jc)^2 from the differences, column by column in ascending c
    order        references sorted by (d2, index) ascending: a stable argsort of d2
    exclusion    reference exclude[i] leaves query i's neighbours, class sums and class counts (by index, never by distance)
    rank         the number of references, excluded or not, that sort strictly before reference target[i]; -1 without one
    class_sum    per class, the sum of sqrt(d2) over the non-excluded references; class_cnt their count
    silhouette   scikit-learn's silhouette_samples, restated from its definition (scikit-learn is not a dependency)
"""
import collections

import numpy as np

Neighbours = collections.namedtuple('Neighbours', 'idx dist class_sum class_cnt rank d2')


def sq_distances(q, r, dtype=np.float64):
    q, r = np.asarray(q, dtype=dtype), np.asarray(r, dtype=dtype)
    d = np.zeros((len(q), len(r)), dtype=dtype)
    for c in range(q.shape[1]):                 # column by column: no (M, N, D) array, and ascending c
        df = q[:, c, None] - r[None, :, c]
        d += df * df
    return d


def neighbours(refs, labels, queries=None, k=5, n_classes=4, exclude=None, target=None, dtype=np.float64):
    """what latent_neighbours returns, as numpy arrays, plus the (M, N) squared distances"""
    refs = np.asarray(refs)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(refs)
    if queries is None:
        queries = refs
        if exclude is None:
            exclude = np.arange(n)
    m = len(queries)
    exclude = np.full(m, -1, dtype=np.int64) if exclude is None else np.asarray(exclude, dtype=np.int64)
    target = np.full(m, -1, dtype=np.int64) if target is None else np.asarray(target, dtype=np.int64)
    d2 = sq_distances(queries, refs, dtype)
    order = np.argsort(d2, axis=1, kind='stable')              # (d2, index): stable keeps the lower index first
    pos = np.empty_like(order)
    pos[np.arange(m)[:, None], order] = np.arange(n)[None, :]
    rank = np.where(target >= 0, pos[np.arange(m), np.maximum(target, 0)], -1).astype(np.int64)
    keep = np.ones((m, n), dtype=bool)
    has = exclude >= 0
    keep[np.nonzero(has)[0], exclude[has]] = False
    idx = np.empty((m, k), dtype=np.int64)
    for i in range(m):
        row = order[i]
        idx[i] = row[keep[i, row]][:k]
    dist = np.sqrt(d2)
    class_sum = np.zeros((m, n_classes), dtype=dtype)
    class_cnt = np.zeros((m, n_classes), dtype=np.int64)
    for c in range(n_classes):
        sel = keep & (labels == c)[None, :]
        class_sum[:, c] = np.where(sel, dist, dtype(0)).sum(axis=1, dtype=dtype)
        class_cnt[:, c] = sel.sum(axis=1)
    return Neighbours(idx, np.take_along_axis(dist, idx, 1), class_sum, class_cnt, rank, d2)


def _spaced(first, gap):
    lo, hi = first[:, :-1], first[:, 1:]
    return ((hi - lo) > gap * hi).all(axis=1)


def decided(d2, exclude, k, gap=1e-5):
    """(M,) bool: the query's first k + 1 non-excluded fp64 Euclidean distances have consecutive relative gaps above `gap`, so
    single precision cannot reorder them and the k neighbour indices are decided.  Two equal distances count as undecided."""
    m, n = d2.shape
    d = np.sqrt(np.array(d2, dtype=np.float64))
    if exclude is not None:
        ex = np.asarray(exclude)
        has = ex >= 0
        d[np.nonzero(has)[0], ex[has]] = np.inf
    first = np.sort(d, axis=1)[:, :min(k + 1, n)]
    return _spaced(first[:, np.isfinite(first).all(axis=0)], gap)


def rank_decided(d2, target, gap=1e-5):
    """(M,) bool: no other reference lies within a relative `gap` of the target's Euclidean distance (True without a target)"""
    d = np.sqrt(np.array(d2, dtype=np.float64))
    out = np.ones(len(d), dtype=bool)
    for i in np.nonzero(np.asarray(target) >= 0)[0]:
        dt = d[i, target[i]]
        near = np.abs(d[i] - dt) <= gap * np.maximum(d[i], dt)
        near[target[i]] = False
        out[i] = not near.any()
    return out


def knn_vote(idx, labels, n_classes):
    """majority vote of each row's neighbours; a tie in votes goes to the tied class whose member comes first in the row"""
    labels = np.asarray(labels)
    out = np.empty(len(idx), dtype=np.int64)
    for i, row in enumerate(np.asarray(idx)):
        votes = np.bincount(labels[row], minlength=n_classes)
        tied = set(np.nonzero(votes == votes.max())[0].tolist())
        out[i] = next(int(labels[j]) for j in row if int(labels[j]) in tied)
    return out


def silhouette_direct(x, labels):
    """silhouette_samples of scikit-learn from its definition, O(N^2) in fp64: a = mean distance to the other members of the
    own cluster, b = the smallest mean distance to another cluster, s = (b - a) / max(a, b); 0 for a singleton cluster"""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    dist = np.sqrt(sq_distances(x, x))
    classes = np.unique(labels)
    s = np.zeros(len(x))
    for i in range(len(x)):
        own = labels == labels[i]
        if own.sum() == 1:
            continue
        a = dist[i, own].sum() / (own.sum() - 1)
        others = [dist[i, labels == c].mean() for c in classes if c != labels[i]]
        if not others:
            s[i] = np.nan
            continue
        b = min(others)
        s[i] = (b - a) / max(a, b)
    return s
