"""fp64 numpy restatement of the alignment statistics (include/t2vae.h, csrc/align.hip): the fp32 values as they are, argmax
by np.argmax (first occurrence), every sum in fp64.  Also the seeded inputs of the GPU tests: softmax rows with a monotone
ridge, built on the host."""
import numpy as np

STATS = ('furthest', 'p_last', 'n_back', 'n_jump', 'longest_stall', 'n_uncovered', 'longest_gap')


def _longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def align(A, n, L, max_jump=3, cover_min=0.5):
    """A: (N, T_in) float32 of one row; only A[:n, :L] is looked at.  Returns path (n,) int64, mass (L,) fp64, focus (fp64),
    stats (the seven integers in STATS order), col_margin (L,) = |mass_j - cover_min| and margin = its minimum: a threshold
    count is defined only where the margin exceeds the error of the mass it is compared with."""
    A = np.asarray(A)
    assert A.dtype == np.float32 and A.ndim == 2 and 1 <= n <= A.shape[0] and 1 <= L <= A.shape[1]
    a = A[:n, :L].astype(np.float64)
    path = np.argmax(A[:n, :L], axis=1).astype(np.int64)
    mass = a.sum(axis=0)
    focus = a[np.arange(n), path].sum() / n
    d = np.diff(path)
    unc = mass < cover_min
    stats = [int(path.max()), int(path[-1]), int((d < 0).sum()), int((d > max_jump).sum()), 1 + _longest_run(d == 0),
             int(unc.sum()), _longest_run(unc)]
    col_margin = np.abs(mass - cover_min)
    return {'path': path, 'mass': mass, 'focus': float(focus), 'stats': stats, 'col_margin': col_margin,
            'margin': float(col_margin.min())}


def sum_bound(n, value):
    """the worst-case error of an fp32 sum of n non-negative terms in any order, plus one rounding for a division:
    n 2^-24 value"""
    return n * 2.0 ** -24 * value


def ridge_row(n, L, seed, sharp=6.0, width=1.5):
    """(n, L) float32 softmax rows: unit Gaussian logits plus a ridge of height `sharp` and width `width` positions whose
    centre walks from the first text position to the last over the n frames"""
    rs = np.random.RandomState(seed)
    logits = rs.randn(n, L)
    centre = np.linspace(0.0, L - 1.0, n) if n > 1 else np.zeros(1)
    j = np.arange(L)[None, :]
    logits = logits + sharp * np.exp(-0.5 * ((j - centre[:, None]) / width) ** 2)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def decided_row(n, L, seed, max_jump=3, cover_min=0.5):
    """(row, reference) of the first seed of seed, seed + 1000, ... whose every column mass is further from cover_min than
    the bound on the error of an fp32 sum of it: the seed is changed, the comparison is never skipped"""
    for k in range(50):
        row = ridge_row(n, L, seed + 1000 * k)
        ref = align(row, n, L, max_jump, cover_min)
        if (ref['col_margin'] > 2 * sum_bound(n, ref['mass'])).all():
            return row, ref
    raise AssertionError("no seed gives decided threshold counts for n = %d, L = %d" % (n, L))
