"""fp64 numpy restatement of the frame-aligned scores (include/t2vae.h, csrc/aligned.hip): the mel cepstrum, the DTW that
keeps its decisions and walks them back, the counts and sums along a given path, and the derived values."""
import math

import numpy as np

NCEP = 13
MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)


def cepstrum_table():
    """(13, 80) fp64: row k - 1 holds sqrt(2 / 80) cos(pi k (n + 1/2) / 80), k = 1..13"""
    k = np.arange(1, NCEP + 1, dtype=np.float64)[:, None]
    n = np.arange(80, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / 80.0) * np.cos(np.pi * k * (n + 0.5) / 80.0)


def cepstrum(mel, table=None):
    """c_1 .. c_13 of a log-mel (80, T) -> (13, T) in fp64, and sum_n |w m| (13, T), the scale of a dot product's rounding
    error; table: another (13, 80) table, e.g. the fp32-rounded one the kernel reads"""
    w = cepstrum_table() if table is None else np.asarray(table, np.float64)
    m = np.asarray(mel, np.float64)
    return w @ m, np.abs(w) @ np.abs(m)


def local_costs(x, y):
    """d(i, j) = ||x_i - y_j||_2 from the differences, (Tx, Ty) fp64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.sqrt(sum((x[c][:, None] - y[c][None, :]) ** 2 for c in range(x.shape[0])))


def dtw_path(x, y):
    """(dist, path) of x (C, Tx) and y (C, Ty): symmetric2 without a band, D(0,0) = 2 d, ties to the diagonal, then (i-1, j),
    then (i, j-1); one numpy operation per anti-diagonal, the decisions kept and walked back from (Tx-1, Ty-1).
    dist = D(Tx-1, Ty-1) / (Tx + Ty); path (K, 2) int64 from (0, 0) to (Tx-1, Ty-1)."""
    d = local_costs(x, y)
    tx, ty = d.shape
    D = np.full((tx + 1, ty + 1), np.inf)
    D[0, 0] = 0.0                                        # the virtual corner that makes D(0,0) = 2 d(0,0)
    frm = np.zeros((tx, ty), dtype=np.int8)
    for k in range(tx + ty - 1):
        i = np.arange(max(0, k - ty + 1), min(tx, k + 1))
        j = k - i
        diag, up, left = D[i, j] + 2 * d[i, j], D[i, j + 1] + d[i, j], D[i + 1, j] + d[i, j]
        best, f = diag.copy(), np.zeros(len(i), dtype=np.int8)
        m = up < best
        best[m], f[m] = up[m], 1
        m = left < best
        best[m], f[m] = left[m], 2
        D[i + 1, j + 1] = best
        frm[i, j] = f
    i, j = tx - 1, ty - 1
    pts = [(i, j)]
    while (i, j) != (0, 0):
        f = frm[i, j]
        i, j = i - (f != 2), j - (f != 1)
        pts.append((i, j))
    return D[tx, ty] / (tx + ty), np.asarray(pts[::-1], dtype=np.int64)


def path_is_valid(path, tx, ty):
    """starts at (0, 0), ends at (tx-1, ty-1), steps only from {(1,1), (1,0), (0,1)}"""
    p = np.asarray(path, dtype=np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or len(p) < 1 or tuple(p[0]) != (0, 0) or tuple(p[-1]) != (tx - 1, ty - 1):
        return False
    st = np.diff(p, axis=0)
    return bool(((st >= 0) & (st <= 1)).all() and (st.sum(axis=1) >= 1).all())


def path_cost(x, y, path):
    """the symmetric2 cost of a path in fp64, over (Tx + Ty): 2 d at the start and on diagonal steps, d on the others"""
    d = local_costs(x, y)
    p = np.asarray(path, dtype=np.int64)
    w = np.concatenate([[2], np.diff(p, axis=0).sum(axis=1)])
    return float((w * d[p[:, 0], p[:, 1]]).sum() / (d.shape[0] + d.shape[1]))


def path_scores(x, y, path, fx=None, fy=None):
    """the counts and sums of t2v_path_scores along `path` in fp64, and for each sum the sum of its terms' magnitudes (the
    scale of its rounding error) with what else the tests' bounds need: sum |dx|, sum |dy|, the largest |log2 f| and the
    distance of the nearest both-voiced point from the gross-error threshold.  fx, fy: F0 per frame in Hz, 0 unvoiced; None: unvoiced everywhere.
    Returns (counts dict, sums dict, scales dict)."""
    d = local_costs(x, y)
    tx, ty = d.shape
    p = np.asarray(path, dtype=np.int64)
    i, j = p[:, 0], p[:, 1]
    a = np.zeros(tx) if fx is None else np.asarray(fx, np.float64)[:tx]
    c = np.zeros(ty) if fy is None else np.asarray(fy, np.float64)[:ty]
    a, c = a[i], c[j]
    va, vc = a > 0, c > 0
    both = va & vc
    a, c = a[both], c[both]
    counts = {'n_points': len(p), 'n_both': int(both.sum()), 'n_vde': int((va != vc).sum()),
              'n_gpe': int((np.abs(a - c) > 0.2 * c).sum())}
    e = 1200.0 * np.log2(a / c)
    lx, ly = np.log2(a), np.log2(c)
    dx, dy = (lx - lx.mean(), ly - ly.mean()) if len(a) else (lx, ly)
    w = np.abs(i / max(tx - 1, 1) - j / max(ty - 1, 1))
    dp = d[i, j]
    sums = {'sum_d': dp.sum(), 'sum_e': e.sum(), 'sum_e2': (e * e).sum(), 's_xx': (dx * dx).sum(), 's_yy': (dy * dy).sum(),
            's_xy': (dx * dy).sum(), 'sum_warp': w.sum()}
    scales = {'sum_d': dp.sum(), 'sum_e': np.abs(e).sum(), 'sum_e2': (e * e).sum(), 's_xx': (dx * dx).sum(),
              's_yy': (dy * dy).sum(), 's_xy': np.abs(dx * dy).sum(), 'sum_warp': w.sum(),
              'abs_dx': np.abs(dx).sum(), 'abs_dy': np.abs(dy).sum(),
              'l_max': max(np.abs(lx).max(), np.abs(ly).max()) if len(a) else 0.0,
              # how near a both-voiced point comes to the 20 % threshold, in units of fy (inf without such points)
              'gpe_margin': (np.abs(np.abs(a - c) - 0.2 * c) / c).min() if len(a) else np.inf}
    return counts, {k: float(v) for k, v in sums.items()}, {k: float(v) for k, v in scales.items()}


def derived(counts, sums, f0=True):
    """the derived values with their None rules (evaluation.aligned_fields restated)"""
    K, nb = counts['n_points'], counts['n_both']
    out = dict.fromkeys(('mcd_db', 'vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_bias_cents', 'lf0_corr', 'warp_dev'))
    out['mcd_db'] = MCD_DB * sums['sum_d'] / K
    out['warp_dev'] = sums['sum_warp'] / K
    if f0:
        out['vde'] = counts['n_vde'] / K
        out['ffe'] = (counts['n_vde'] + counts['n_gpe']) / K
        if nb:
            out['gpe'] = counts['n_gpe'] / nb
            out['lf0_rmse_cents'] = math.sqrt(sums['sum_e2'] / nb)
            out['lf0_bias_cents'] = sums['sum_e'] / nb
            if nb >= 2 and sums['s_xx'] > 0 and sums['s_yy'] > 0:
                out['lf0_corr'] = max(-1.0, min(1.0, sums['s_xy'] / math.sqrt(sums['s_xx'] * sums['s_yy'])))
    return out
