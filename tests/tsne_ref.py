"""Exact t-SNE restated in numpy, for the CPU and GPU tests of t2v_hip.tsne (csrc/tsne.hip).  Every function takes a
dtype: float64 is the reference, float32 the yardstick that says what single precision costs on the same formulas.

    distances      d_ij = sum_c (x_ic - x_jc)^2, from the differences
    conditional    p_j|i = exp(-d_ij beta_i) / sum_k exp(-d_ik beta_i), p_i|i = 0; beta_i by binary search: 100 steps at
                   most, |H_i - log(perplexity)| <= 1e-5 ends it, beta doubles / halves while a bound is infinite, a sum
                   that vanished is replaced by 1e-8
    joint          P = (p + p^T) / max(sum(p + p^T), eps), floored at eps = 2^-52, diagonal 0
    kl_and_grad    w_ij = 1 / (1 + |y_i - y_j|^2), Q = max(w / sum_{k != l} w_kl, eps), P' = ex P,
                   kl = sum_{i != j} P' log(max(P', eps) / Q), grad_i = 4 sum_j (P'_ij - Q_ij) w_ij (y_i - y_j)
    descend        gains += 0.2 where update * grad < 0, *= 0.8 elsewhere, floor 0.01; update = momentum * update -
                   lr * gains * grad; 250 iterations at exaggeration 12 and momentum 0.5, then 1 and 0.8; no early stop
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
EXAG_ITERS = 250
EXAG = 12.0
KL_EVERY = 50


def distances(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    d = np.zeros((len(x), len(x)), dtype=dtype)
    for c in range(x.shape[1]):                 # column by column: no (N, N, D) array
        df = x[:, c, None] - x[None, :, c]
        d += df * df
    return d


def conditional(d, perplexity, dtype=np.float64, steps=100, tol=1e-5):
    """(p (N, N), beta (N,)) of the rows of squared distances d"""
    d = np.asarray(d, dtype=dtype)
    n = len(d)
    off = ~np.eye(n, dtype=bool)
    target = dtype(np.log(perplexity))
    beta = np.ones(n, dtype=dtype)
    lo = np.full(n, -np.inf, dtype=dtype)
    hi = np.full(n, np.inf, dtype=dtype)
    p = np.zeros((n, n), dtype=dtype)
    todo = np.arange(n)
    for _ in range(steps):
        b = beta[todo]
        e = np.exp(-d[todo] * b[:, None]) * off[todo]
        s = e.sum(axis=1, dtype=dtype)
        s[s == 0] = dtype(1e-8)
        e = e / s[:, None]
        h = np.log(s) + b * (d[todo] * e).sum(axis=1, dtype=dtype)
        p[todo] = e
        diff = h - target
        go = np.abs(diff) > tol
        up = go & (diff > 0)
        dn = go & ~(diff > 0)
        r = todo[up]
        lo[r] = beta[r]
        beta[r] = np.where(np.isinf(hi[r]), beta[r] * 2, (beta[r] + hi[r]) / 2)
        r = todo[dn]
        hi[r] = beta[r]
        beta[r] = np.where(np.isinf(lo[r]), beta[r] / 2, (beta[r] + lo[r]) / 2)
        todo = todo[go]
        if not len(todo):
            break
    # beta of the rows that never met the tolerance was moved once more after their last evaluation: p is what counts
    return p, beta


def joint(p, dtype=np.float64):
    p = np.asarray(p, dtype=dtype)
    s = p + p.T
    out = np.maximum(s / max(s.sum(dtype=dtype), EPS), dtype(EPS))
    np.fill_diagonal(out, 0)
    return out.astype(dtype)


def affinities(x, perplexity, dtype=np.float64):
    return joint(conditional(distances(x, dtype), perplexity, dtype)[0], dtype)


def kl_and_grad(P, y, exaggeration=1.0, dtype=np.float64):
    """(kl, grad (N, 2)) at the map y; P is symmetric with a zero diagonal"""
    P = np.asarray(P, dtype=dtype) * dtype(exaggeration)
    y = np.asarray(y, dtype=dtype)
    n = len(y)
    off = ~np.eye(n, dtype=bool)
    dx = y[:, None, 0] - y[None, :, 0]
    dy = y[:, None, 1] - y[None, :, 1]
    w = dtype(1) / (dtype(1) + dx * dx + dy * dy)
    w[~off] = 0
    Q = np.maximum(w / w.sum(dtype=dtype), dtype(EPS))
    kl = (P[off] * np.log(np.maximum(P[off], dtype(EPS)) / Q[off])).sum(dtype=dtype)
    f = (P - Q * off) * w
    grad = dtype(4) * np.stack([(f * dx).sum(axis=1, dtype=dtype), (f * dy).sum(axis=1, dtype=dtype)], axis=1)
    return dtype(kl), grad.astype(dtype)


def learning_rate(n):
    return max(n / EXAG / 4.0, 50.0)


def descend(P, y0, n_iter, lr=None, dtype=np.float64):
    """(map after n_iter updates, kl trace): trace[k] is the objective, with the exaggeration of that iteration, at the map
    after min(50 (k + 1), n_iter) updates"""
    y = np.array(y0, dtype=dtype)
    lr = dtype(learning_rate(len(y)) if lr is None else lr)
    upd = np.zeros_like(y)
    gains = np.ones_like(y)
    trace = []
    for it in range(n_iter + 1):
        exag = it < EXAG_ITERS
        kl, g = kl_and_grad(P, y, EXAG if exag else 1.0, dtype)
        if it > 0 and (it == n_iter or it % KL_EVERY == 0):
            trace.append(float(kl))
        if it == n_iter:
            break
        inc = upd * g < 0
        gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
        upd = dtype(0.5 if exag else 0.8) * upd - lr * (gains * g)
        y = y + upd
    return y, np.array(trace)


def init(n, seed=0):
    return (1e-4 * np.random.RandomState(seed).standard_normal(size=(n, 2))).astype(np.float32)


def knn_label_agreement(pts, labels, k=5):
    """share of the k nearest neighbours (Euclidean, self excluded) that carry the point's own label, averaged"""
    pts = np.asarray(pts, dtype=np.float64)
    labels = np.asarray(labels)
    d = distances(pts)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind='stable')[:, :k]
    return float((labels[nn] == labels[:, None]).mean())
