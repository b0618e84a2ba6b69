"""t2v_hip.mel_cepstrum and t2v_hip.aligned_scores (csrc/aligned.hip) against the fp64 restatement in aligned_ref: the
cepstrum, the warping path (valid, and optimal to round-off; equal to the reference's where arithmetic is exact), determinism,
the scores along the kernel's own path, and the errors.

Bounds (derived, not measured; u = 2^-24):
  cepstrum   an 80-term fp32 dot product by fused multiply-add has the first-order bound 80 u sum |w m|; the test allows twice
             that, against the fp64 sum over the fp32 table the kernel reads.
  path       a path that is optimal under fp32 costs exceeds the fp64 optimum by at most (Tx + Ty + 16) 2^-23 of it to first
             order (Tx + Ty additions along a path, 16 for a local cost); the recomputed cost and `dist` are held to twice that.
  sums       thread t adds the points t, t + 256, ... and a tree adds the 256 partial sums: a term passes A = ceil(K / 256) + 8
             additions.  First-order bounds, each allowed twice:
    sum_d    (9 + A) u sum d: a local cost carries 15 u in its sum of squares (the differences, 13 fused multiply-adds), half of
             that and one rounding after the square root.
    sum_warp (1 + A) u sum w + 2 u K: the two quotients lie in [0, 1] and carry u each, which is not relative to their
             difference; the diagonal of an equal-length pair still gives exactly 0.
    sum_e    with e = 1200 log2(fx / fy): the quotient carries u, i.e. u / ln 2 in the logarithm; log2f is taken as good to 2 ulp
             (4 u |log2|), the product by 1200 adds u.  De = 1200 u / ln 2 per point and 5 u |e|, so the sum has
             n_both 1200 u / ln 2 + (5 + A) u sum |e|.
    sum_e2   2 |e| De and the square's own rounding: 2400 u / ln 2 sum |e| + (11 + A) u sum e^2.
    s_xx     the logarithms carry Dl = 4 u max |log2 f|; the mean's error moves every centred value alike and cancels to first
             order (the centred values sum to 0), so 2 Dl sum |dx| + (2 + A) u sum dx^2; s_yy alike, and
    s_xy     Dl (sum |dx| + sum |dy|) + (2 + A) u sum |dx dy|.
  The gross-error count is exact when no both-voiced point lies within 4 u fy of the 20 % threshold (|fx - fy| and 0.2f fy
  carry under u fy together); the test asserts that of its inputs."""
import math

import numpy as np
import pytest
import torch

import aligned_ref as AR

pytestmark = pytest.mark.gpu

# one row; a thread's 8 rows minus and plus one; a wave's edge (64 threads = 512 rows is covered by 600); all threads; the maximum
CASES = [(1, 1), (1, 7), (7, 1), (8, 9), (9, 8), (37, 5), (63, 64), (64, 65), (257, 1025), (600, 913), (2041, 2047), (2048, 2048)]
U = 2.0 ** -24
SUMS = ('sum_d', 'sum_e', 'sum_e2', 's_xx', 's_yy', 's_xy', 'sum_warp')


def _path_tol(tx, ty):
    return (tx + ty + 16) * 2.0 ** -22


def _padded(rows, width, fill=float('nan')):
    """(B, C, width) float32 from a list of (C, T_b) arrays, `fill` past each length"""
    out = torch.full((len(rows), rows[0].shape[0], width), fill)
    for b, r in enumerate(rows):
        out[b, :, :r.shape[1]] = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32))
    return out


def _speechlike(seed):
    """per case X a random walk over time and Y a resampled copy of X plus noise, fp32 values"""
    rs = np.random.RandomState(seed)
    xs, ys = [], []
    for tx, ty in CASES:
        x = np.cumsum(rs.randn(13, tx) * 0.3, axis=1)
        y = x[:, np.round(np.linspace(0, tx - 1, ty)).astype(int)] + 0.1 * rs.randn(13, ty)
        xs.append(x.astype(np.float32))
        ys.append(y.astype(np.float32))
    return xs, ys


def _tracks(seed):
    """per case fx 60-500 Hz and fy = fx (resampled to Ty) * U(0.7, 1.4), about 30 % unvoiced on each side, fp32 values"""
    rs = np.random.RandomState(seed)
    fxs, fys = [], []
    for tx, ty in CASES:
        fx = rs.uniform(60.0, 500.0, tx)
        fy = fx[np.round(np.linspace(0, tx - 1, ty)).astype(int)] * rs.uniform(0.7, 1.4, ty)
        fx[rs.rand(tx) < 0.3] = 0.0
        fy[rs.rand(ty) < 0.3] = 0.0
        fxs.append(fx.astype(np.float32))
        fys.append(fy.astype(np.float32))
    return fxs, fys


@pytest.fixture(scope='module')
def batch():
    import t2v_hip
    assert max(max(c) for c in CASES) == t2v_hip.DTW_MAX_FRAMES        # the supported maximum is among the cases
    xs, ys = _speechlike(1)
    fxs, fys = _tracks(2)
    nx, ny = [c[0] for c in CASES], [c[1] for c in CASES]
    ref = [AR.dtw_path(x, y) for x, y in zip(xs, ys)]
    # a condition on the inputs: along the reference's path no both-voiced point sits on the 20 % threshold
    for b in range(len(CASES)):
        assert AR.path_scores(xs[b], ys[b], ref[b][1], fxs[b], fys[b])[2]['gpe_margin'] > 4 * U, CASES[b]
    return dict(xs=xs, ys=ys, fxs=fxs, fys=fys, nx=nx, ny=ny, ref=ref,
                x=_padded(xs, max(nx)), y=_padded(ys, max(ny) + 3),
                fx=_padded([f[None] for f in fxs], max(nx) + 5)[:, 0].contiguous(),
                fy=_padded([f[None] for f in fys], max(ny))[:, 0].contiguous())


def _run(bt, **kw):
    import t2v_hip
    return t2v_hip.aligned_scores(bt['x'].cuda(), bt['nx'], bt['y'].cuda(), bt['ny'], bt['fx'].cuda(), bt['fy'].cuda(),
                                  return_path=True, **kw)


def _bits(r, b=None):
    """everything a result defines, as bytes (the path only up to each K)"""
    rows = range(r.dist.numel()) if b is None else [b]
    k = r.n_points.cpu().tolist()
    path = r.path.cpu().numpy()
    return [(r.dist[i:i + 1].cpu().numpy().tobytes(), k[i], r.counts[i].cpu().numpy().tobytes(), r.sums[i].cpu().numpy().tobytes(),
             path[i, :k[i]].tobytes()) for i in rows]


def test_cepstrum_matches_fp64():
    """|c - ref| <= 2 * 80 u sum |w m| per value, ref the fp64 sum over the kernel's fp32 table; 0 past each length; a row alone
    gives the batch's bits"""
    import t2v_hip
    lengths = [1, 255, 256, 257, 700]
    g = torch.Generator().manual_seed(3)
    m = torch.full((len(lengths), 80, 703), float('nan'))
    for b, n in enumerate(lengths):
        m[b, :, :n] = torch.randn(80, n, generator=g) * 2 - 4
    c = t2v_hip.mel_cepstrum(m.cuda(), lengths)
    assert c.shape == (len(lengths), 13, 703)
    c = c.cpu()
    worst = 0.0
    for b, n in enumerate(lengths):
        ref, scale = AR.cepstrum(m[b, :, :n].numpy(), t2v_hip.cepstrum_table())
        err = np.abs(c[b, :, :n].double().numpy() - ref)
        worst = max(worst, float((err / (2 * 80 * U * scale)).max()))
        assert (err <= 2 * 80 * U * scale).all(), (n, float((err / scale).max()))
        assert (c[b, :, n:] == 0).all()
        # the fp32 table itself costs one more rounding against the formula in fp64
        full = AR.cepstrum(m[b, :, :n].numpy())[0]
        assert (np.abs(c[b, :, :n].double().numpy() - full) <= 2 * 81 * U * scale).all()
        alone = t2v_hip.mel_cepstrum(m[b:b + 1, :, :n].contiguous().cuda(), torch.tensor([n]).cuda()).cpu()
        assert alone.numpy().tobytes() == c[b:b + 1, :, :n].contiguous().numpy().tobytes(), n
    print("cepstrum: worst error over its bound %.3f" % worst)


def test_path_is_valid_and_optimal_to_round_off(batch):
    r = _run(batch)
    k = r.n_points.cpu().tolist()
    dist = r.dist.cpu().double().numpy()
    path = r.path.cpu().numpy()
    assert r.path.shape == (len(CASES), max(tx + ty - 1 for tx, ty in CASES), 2) and r.path.dtype == torch.int32
    for b, (tx, ty) in enumerate(CASES):
        ref_dist, ref_path = batch['ref'][b]
        p = path[b, :k[b]]
        assert max(tx, ty) <= k[b] <= tx + ty - 1, (tx, ty, k[b])
        assert AR.path_is_valid(p, tx, ty), (tx, ty)                                             # (a)
        cost = AR.path_cost(batch['xs'][b], batch['ys'][b], p)
        agree = len(set(map(tuple, p.tolist())) & set(map(tuple, ref_path.tolist()))) / len(ref_path)
        print("(%d, %d): K %d (ref %d), %.4f of the reference's points, cost excess %.3g, dist rel err %.3g, bound %.3g"
              % (tx, ty, k[b], len(ref_path), agree, cost / ref_dist - 1, abs(dist[b] - ref_dist) / ref_dist, _path_tol(tx, ty)))
        assert cost <= ref_dist * (1 + _path_tol(tx, ty)), (tx, ty, cost, ref_dist)              # (b)
        assert abs(dist[b] - ref_dist) <= ref_dist * _path_tol(tx, ty), (tx, ty, dist[b], ref_dist)      # (c)


@pytest.fixture(scope='module')
def exact():
    """cepstra with one non-zero coefficient holding integers 0..7: every cost and every sum is exact in fp32 and in fp64, and
    ties are everywhere"""
    rs = np.random.RandomState(5)
    xs, ys = [], []
    for b, (tx, ty) in enumerate(CASES):
        x, y = np.zeros((13, tx), np.float32), np.zeros((13, ty), np.float32)
        x[b % 13], y[b % 13] = rs.randint(0, 8, tx), rs.randint(0, 8, ty)
        xs.append(x)
        ys.append(y)
    return xs, ys, [AR.dtw_path(x, y) for x, y in zip(xs, ys)]


def test_exact_inputs_give_the_reference_path(exact):
    import t2v_hip
    xs, ys, ref = exact
    nx, ny = [c[0] for c in CASES], [c[1] for c in CASES]
    r = t2v_hip.aligned_scores(_padded(xs, max(nx) + 1).cuda(), nx, _padded(ys, max(ny)).cuda(), ny, return_path=True)
    k = r.n_points.cpu().tolist()
    path = r.path.cpu().numpy()
    for b, (tx, ty) in enumerate(CASES):
        ref_dist, ref_path = ref[b]
        assert k[b] == len(ref_path), (tx, ty, k[b], len(ref_path))
        assert np.array_equal(path[b, :k[b]], ref_path), (tx, ty)
        assert abs(float(r.dist[b]) - ref_dist) <= ref_dist * U, (tx, ty)         # D is exact; one rounding in the division
        sums = AR.path_scores(xs[b], ys[b], ref_path)[1]
        assert float(r.sum_d[b]) == sums['sum_d'], (tx, ty)                          # small integers: exact in any order
        assert r.counts[b].cpu().tolist() == [len(ref_path), 0, 0, 0]


def test_all_zero_inputs_go_diagonal_first():
    import t2v_hip
    pairs = [(3, 5), (5, 3), (9, 9), (17, 40), (300, 70)]
    nx, ny = [p[0] for p in pairs], [p[1] for p in pairs]
    r = t2v_hip.aligned_scores(torch.zeros(len(pairs), 13, max(nx)).cuda(), nx, torch.zeros(len(pairs), 13, max(ny)).cuda(), ny,
                               return_path=True)
    k = r.n_points.cpu().tolist()
    path = r.path.cpu().numpy()
    assert path[0, :k[0]].tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    for b, (tx, ty) in enumerate(pairs):
        # the diagonal from the end as far as it goes, then along the edge to (0, 0)
        i, j = np.arange(tx - 1, -1, -1), np.arange(ty - 1, -1, -1)
        m = min(tx, ty)
        want = list(zip(i[:m], j[:m])) + [(a, 0) for a in i[m:]] + [(0, c) for c in j[m:]]
        assert k[b] == max(tx, ty) and [tuple(q) for q in path[b, :k[b]].tolist()] == want[::-1], (tx, ty)
    assert (r.dist.cpu() == 0).all() and (r.sum_d.cpu() == 0).all()


def test_second_call_and_pairs_alone_give_the_same_bits(batch):
    import t2v_hip
    first = _run(batch)
    bits = _bits(first)
    assert _bits(_run(batch)) == bits
    for b, (tx, ty) in enumerate(CASES):
        # alone, cut to its own length: other strides, no padding at all
        a = t2v_hip.aligned_scores(batch['x'][b:b + 1, :, :tx].contiguous().cuda(), [tx], batch['y'][b:b + 1, :, :ty].contiguous().cuda(),
                                   [ty], batch['fx'][b:b + 1, :tx].contiguous().cuda(), batch['fy'][b:b + 1, :ty].contiguous().cuda(),
                                   return_path=True)
        assert _bits(a) == bits[b:b + 1], (tx, ty)


def test_group_split_gives_the_same_bits(monkeypatch):
    import t2v_hip
    nx, ny = [600, 3, 520, 77, 513, 1, 64, 300], [40, 600, 513, 90, 1, 1, 700, 300]
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(8, 13, 600, generator=g).cumsum(2).cuda(), torch.randn(8, 13, 700, generator=g).cumsum(2).cuda()
    fx, fy = (torch.rand(8, 600, generator=g) * 400 + 60).cuda(), (torch.rand(8, 700, generator=g) * 400 + 60).cuda()
    whole = _bits(t2v_hip.aligned_scores(x, nx, y, ny, fx, fy, return_path=True))
    lib = t2v_hip.load_library()
    per_pair = lib.t2v_cep_dtw_scratch_bytes(1, 600, 700)
    assert per_pair == (700 + 599 // 8) * 512
    calls = []
    real = lib.t2v_cep_dtw_path
    monkeypatch.setattr(t2v_hip, 'CEP_DTW_SCRATCH_CAP', 3 * per_pair)      # groups of 3, 3, 2

    class Spy(object):
        def __getattr__(self, name):
            return getattr(lib, name)

        def t2v_cep_dtw_path(self, *a):
            calls.append(a[6])
            return real(*a)

    monkeypatch.setattr(t2v_hip, '_lib', Spy())
    split = _bits(t2v_hip.aligned_scores(x, nx, y, ny, fx, fy, return_path=True))
    assert calls == [3, 3, 2]
    assert split == whole


def _sum_bounds(counts, scales):
    """the first-order bounds of the module docstring, doubled"""
    K, nb = counts['n_points'], counts['n_both']
    A = math.ceil(K / 256) + 8
    De = 1200.0 * U / math.log(2.0)
    Dl = 4 * U * scales['l_max']
    first = {'sum_d': (9 + A) * U * scales['sum_d'],
             'sum_warp': (1 + A) * U * scales['sum_warp'] + 2 * U * K,
             'sum_e': nb * De + (5 + A) * U * scales['sum_e'],
             'sum_e2': 2 * De * scales['sum_e'] + (11 + A) * U * scales['sum_e2'],
             's_xx': 2 * Dl * scales['abs_dx'] + (2 + A) * U * scales['s_xx'],
             's_yy': 2 * Dl * scales['abs_dy'] + (2 + A) * U * scales['s_yy'],
             's_xy': Dl * (scales['abs_dx'] + scales['abs_dy']) + (2 + A) * U * scales['s_xy']}
    return {k: 2 * v for k, v in first.items()}


def test_scores_along_the_kernels_own_path(batch):
    """counts exact, sums within the module docstring's bounds, against fp64 along the path the kernel returned"""
    import t2v_hip
    r = _run(batch)
    assert tuple(r.counts.shape) == (len(CASES), 4) and tuple(r.sums.shape) == (len(CASES), 8)
    k = r.n_points.cpu().tolist()
    path, counts, sums = r.path.cpu().numpy(), r.counts.cpu().tolist(), r.sums.cpu().double().numpy()
    worst = {}
    for b, (tx, ty) in enumerate(CASES):
        want_c, want_s, scales = AR.path_scores(batch['xs'][b], batch['ys'][b], path[b, :k[b]], batch['fxs'][b], batch['fys'][b])
        assert scales['gpe_margin'] > 4 * U, (tx, ty)                      # the inputs' condition, on this path too
        assert counts[b] == [want_c[n] for n in t2v_hip.ALIGNED_COUNTS], (tx, ty, counts[b], want_c)
        bound = _sum_bounds(want_c, scales)
        for n in SUMS:
            err = abs(sums[b, t2v_hip.ALIGNED_SUMS.index(n)] - want_s[n])
            if bound[n] > 0:
                worst[n] = max(worst.get(n, 0.0), err / bound[n])
            assert err <= bound[n], (tx, ty, n, sums[b, t2v_hip.ALIGNED_SUMS.index(n)], want_s[n], bound[n])
        assert sums[b, 7] == 0.0
    print("worst error over its bound: " + ", ".join("%s %.3f" % (n, worst.get(n, 0.0)) for n in SUMS))
    # the attributes are the columns, and the derived values follow
    from evaluation import aligned_fields
    assert torch.equal(r.n_gpe, r.counts[:, 3]) and torch.equal(r.sum_warp, r.sums[:, 6]) and torch.equal(r.n_points, r.counts[:, 0])
    b = CASES.index((600, 913))
    got = aligned_fields(counts[b], sums[b])                                # host arithmetic alone: fp64 on the kernel's numbers
    want = AR.derived(dict(zip(t2v_hip.ALIGNED_COUNTS, counts[b])), dict(zip(t2v_hip.ALIGNED_SUMS, sums[b].tolist())))
    assert all(v is not None for v in want.values())
    assert all(got[key] == pytest.approx(want[key], rel=1e-12) for key in want), (got, want)


def test_missing_tracks_are_unvoiced_everywhere(batch):
    import t2v_hip
    x, y = batch['x'].cuda(), batch['y'].cuda()
    both = _run(batch)
    none = t2v_hip.aligned_scores(x, batch['nx'], y, batch['ny'])
    assert none.path is None
    assert none.counts[:, 1:].cpu().eq(0).all() and torch.equal(none.counts[:, 0], both.counts[:, 0])
    assert none.sums[:, 1:6].cpu().eq(0).all() and torch.equal(none.sum_d, both.sum_d) and torch.equal(none.sum_warp, both.sum_warp)
    one = t2v_hip.aligned_scores(x, batch['nx'], y, batch['ny'], f0y=batch['fy'].cuda())
    voiced = [int((f > 0).sum()) for f in batch['fys']]
    assert one.n_both.cpu().eq(0).all() and one.n_gpe.cpu().eq(0).all()
    assert all(v >= n for v, n in zip(one.n_vde.cpu().tolist(), voiced))          # every voiced frame of y is on the path


def test_length_containers_agree():
    import t2v_hip
    nx, ny = [40, 17, 3], [9, 55, 64]
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(3, 13, 48, generator=g).cuda(), torch.randn(3, 13, 64, generator=g).cuda()
    a = _bits(t2v_hip.aligned_scores(x, nx, y, ny, return_path=True))
    b = _bits(t2v_hip.aligned_scores(x, torch.tensor(nx), y, torch.tensor(ny, dtype=torch.int32), return_path=True))
    c = _bits(t2v_hip.aligned_scores(x, torch.tensor(nx).cuda(), y, torch.tensor(ny, dtype=torch.int32).cuda(), return_path=True))
    assert a == b == c


def test_errors_leave_the_library_usable():
    import t2v_hip
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(2, 13, 24, generator=g).cuda(), torch.randn(2, 13, 30, generator=g).cuda()
    good = _bits(t2v_hip.aligned_scores(x, [20, 20], y, [30, 30], return_path=True))
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x, [0, 20], y, [30, 30])                         # length 0
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x, [20, 20], y, [30, 31])                        # length > stride
    big = torch.zeros(1, 13, t2v_hip.DTW_MAX_FRAMES + 1).cuda()
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(big, [t2v_hip.DTW_MAX_FRAMES + 1], y[:1], [30])  # length > maximum
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x[:, :12].contiguous(), [20, 20], y[:, :12].contiguous(), [30, 30])     # n_cep != 13
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x, [20, 20], y[:1], [30])                        # mismatched B
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x, [20], y, [30, 30])                            # mismatched B in the lengths
    with pytest.raises(ValueError):
        t2v_hip.aligned_scores(x, [20, 20], y, [30, 30], f0x=torch.zeros(2, 19).cuda())        # a track shorter than its rows
    with pytest.raises(ValueError):
        t2v_hip.mel_cepstrum(torch.zeros(2, 79, 8).cuda(), [8, 8])              # n_mel != 80
    with pytest.raises(ValueError):
        t2v_hip.mel_cepstrum(torch.zeros(2, 80, 8).cuda(), [8, 9])              # length > stride
    # the C entries themselves refuse other dimensions (T2V_ERR_DIMS) and null pointers (T2V_ERR_ARG)
    lib = t2v_hip.load_library()
    p, st = t2v_hip._p, t2v_hip._stream
    n20, n30 = torch.tensor([20, 20], dtype=torch.int32).cuda(), torch.tensor([30, 30], dtype=torch.int32).cuda()
    scratch = torch.empty(lib.t2v_cep_dtw_scratch_bytes(2, 24, 30), dtype=torch.uint8).cuda()
    dist, K, path = torch.empty(2).cuda(), torch.empty(2, dtype=torch.int32).cuda(), torch.empty(2, 49, 2, dtype=torch.int32).cuda()
    counts, sums = torch.empty(2, 4, dtype=torch.int32).cuda(), torch.empty(2, 8).cuda()
    args = [p(x), p(n20), 24, p(y), p(n30), 30, 2, 13, p(dist), p(K), p(path), 49, p(scratch), st()]
    assert lib.t2v_cep_dtw_path(*(args[:7] + [12] + args[8:])) == -1
    assert lib.t2v_cep_dtw_path(*(args[:10] + [None] + args[11:])) == -2
    assert lib.t2v_cep_dtw_path(*(args[:6] + [0] + args[7:])) == -2
    assert lib.t2v_path_scores(p(path), p(K), 49, p(x), p(n20), 24, p(y), p(n30), 30, None, 1, None, 1, 2, 12, p(counts), p(sums), st()) == -1
    assert lib.t2v_path_scores(p(path), None, 49, p(x), p(n20), 24, p(y), p(n30), 30, None, 1, None, 1, 2, 13, p(counts), p(sums), st()) == -2
    m, out = torch.zeros(2, 80, 8).cuda(), torch.empty(2, 13, 8).cuda()
    n8, tab = torch.tensor([8, 8], dtype=torch.int32).cuda(), t2v_hip.cepstrum_table(m.device)
    assert lib.t2v_mel_cepstrum(p(m), p(n8), 8, 2, 79, 13, p(tab), p(out), 8, st()) == -1
    assert lib.t2v_mel_cepstrum(p(m), p(n8), 8, 2, 80, 12, p(tab), p(out), 8, st()) == -1
    assert lib.t2v_mel_cepstrum(p(m), p(n8), 8, 2, 80, 13, None, p(out), 8, st()) == -2
    assert lib.t2v_cep_dtw_scratch_bytes(0, 24, 30) == 0 and lib.t2v_cep_dtw_scratch_bytes(1, 2048, 2048) == (2048 + 255) * 512
    # a pair whose device length got past the host is refused by the kernels' early return: NaN, K = 0, and its neighbour is whole
    bad = torch.tensor([0, 20], dtype=torch.int32).cuda()
    assert lib.t2v_cep_dtw_path(*(args[:1] + [p(bad)] + args[2:])) == 0
    assert lib.t2v_path_scores(p(path), p(K), 49, p(x), p(bad), 24, p(y), p(n30), 30, None, 1, None, 1, 2, 13, p(counts), p(sums), st()) == 0
    assert math.isnan(float(dist[0])) and K.cpu().tolist()[0] == 0 and K.cpu().tolist()[1] == good[1][1]
    assert counts[0].cpu().tolist() == [0, 0, 0, 0] and torch.isnan(sums[0]).all()
    assert dist[1:].cpu().numpy().tobytes() == good[1][0] and path[1, :good[1][1]].cpu().numpy().tobytes() == good[1][4]
    assert counts[1].cpu().numpy().tobytes() == good[1][2] and sums[1].cpu().numpy().tobytes() == good[1][3]
    # the maximum is longer than a long stride allows: a long stride alone is fine
    ok = t2v_hip.aligned_scores(big, [5], y[:1], [30])
    assert torch.isfinite(ok.dist).all() and ok.n_points.cpu().tolist()[0] >= 30
    assert _bits(t2v_hip.aligned_scores(x, [20, 20], y, [30, 30], return_path=True)) == good
    t2v_hip.check_async_errors()
