"""t2v_hip.latent_neighbours (csrc/latent.hip) against tests/latent_ref.py in fp64, with the same formulas run in fp32 numpy
as the yardstick of what single precision costs; exact ties on an integer grid, the edges of every limit, independence of the
slice length and of padding, and the refusals.

Error rule of the value tests (that of tests/test_tsne_gpu.py): kernel error <= 4 x max(error of the fp32 restatement, one
fp32 rounding), both relative to the array's maximum.  Index rule: nn_idx must equal the reference's for every query whose
first k + 1 fp64 distances have consecutive relative gaps above 1e-5 (about 30 x the fp32 error of a 32-term distance); the
share of queries that rule leaves out is asserted <= 5 %.  rank is compared exactly on the kept queries and within 1 on the
others.  Cluster scale 0.5 puts the fp64 leave-one-out kNN accuracy at 0.84 / 0.85 / 0.84 for the three self-mode cases, so
the confusion matrix is not trivial."""
import numpy as np
import pytest
import torch

import latent_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 4.0
ULP = 2.0 ** -24
GAP = 1e-5
SCALE = 0.5
SELF_CASES = [(601, 5), (130, 16), (1100, 5)]


def _clusters(n, seed=77, d=32, scale=SCALE):
    """rows scale * centres[i % 4] + noise, labels i % 4 (the construction of test_tsne_gpu._with_duplicates)"""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((4, d))
    return (scale * centres[np.arange(n) % 4] + rs.standard_normal((n, d))).astype(np.float32), np.arange(n) % 4


def _clear_targets(queries, refs, target):
    """the targets moved on (index + 1, + 2, ...) until no other reference lies within a relative 1e-5 of the target's fp64
    distance: which references sort before such a target does not hang on an fp32 rounding, so rank has one right answer"""
    d2 = R.sq_distances(queries, refs)
    target = np.array(target)
    for i in np.nonzero(target >= 0)[0]:
        one = np.full(len(target), -1)
        for step in range(len(refs)):
            one[i] = (target[i] + step) % len(refs)
            if R.rank_decided(d2[i:i + 1], one[i:i + 1], GAP)[0]:
                break
        target[i] = one[i]
    return target


def _self_case(n, k):
    X, lab = _clusters(n)
    target = (np.arange(n) * 7 + 3) % n
    target[::3] = -1
    return dict(refs=X, labels=lab, queries=None, k=k, n_classes=4, exclude=None, target=_clear_targets(X, X, target))


def _cross_case():
    """257 queries against 601 references; query 4j is reference (37 j) % 601 plus noise and excludes / targets it, query
    4j + 2 is a fresh cluster point that excludes / targets an arbitrary reference, the odd queries have neither"""
    X, lab = _clusters(601)
    m = 257
    rs = np.random.RandomState(78)
    Q, _ = _clusters(m, seed=79)
    ex = np.full(m, -1, dtype=np.int64)
    near = np.arange(0, m, 4)
    ex[near] = (37 * (near // 4)) % 601
    Q[near] = X[ex[near]] + 0.8 * rs.standard_normal((len(near), 32)).astype(np.float32)
    far = np.arange(2, m, 4)
    ex[far] = rs.randint(0, 601, size=len(far))
    ex = _clear_targets(Q, X, ex)
    return dict(refs=X, labels=lab, queries=Q, k=5, n_classes=4, exclude=ex, target=ex.copy())


_REFS = {}


def _reference(name):
    """(case, fp64 reference, fp32 restatement), computed once per case and shared"""
    if name not in _REFS:
        case = _cross_case() if name == 'cross' else _self_case(*name)
        _REFS[name] = (case, R.neighbours(**case), R.neighbours(dtype=np.float32, **case))
    return _REFS[name]


def _run(case, **kw):
    import t2v_hip
    args = dict(case, **kw)
    refs = torch.from_numpy(args.pop('refs')).cuda()
    queries = args.pop('queries')
    queries = None if queries is None else torch.from_numpy(queries).cuda()
    r = t2v_hip.latent_neighbours(refs, args.pop('labels'), queries, **args)
    m = len(case['refs']) if queries is None else len(queries)
    assert r.idx.shape == (m, case['k']) and r.idx.dtype == torch.int32 and r.dist.shape == (m, case['k'])
    assert r.class_sum.shape == (m, case['n_classes']) and r.class_cnt.dtype == torch.int32 and r.rank.shape == (m,)
    return type(r)(*(t.cpu().numpy() for t in r))


def _err(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _excluded(case):
    m = len(case['refs']) if case['queries'] is None else len(case['queries'])
    if case['exclude'] is not None:
        return np.asarray(case['exclude'])
    return np.arange(m) if case['queries'] is None else np.full(m, -1)


@pytest.mark.parametrize("name", SELF_CASES + ['cross'], ids=lambda v: str(v))
def test_values_against_fp64(name):
    case, ref, yard = _reference(name)
    got = _run(case)
    k, ex = case['k'], _excluded(case)
    m = len(got.idx)
    if name != 'cross':
        acc = float((R.knn_vote(ref.idx, case['labels'], 4) == case['labels']).mean())
        print("%s: fp64 leave-one-out kNN accuracy %.4f" % (name, acc))
        assert 0.5 < acc < 0.95
    # distances and class sums: the tsne error rule
    for what, a, y, r in (('nn_dist', got.dist, yard.dist, ref.dist), ('class_sum', got.class_sum, yard.class_sum, ref.class_sum)):
        e_k, e_y = _err(a, r), _err(y, r)
        print("%s %s: error / max kernel %.3g, fp32 numpy %.3g" % (name, what, e_k, e_y))
        assert e_k <= MARGIN * max(e_y, ULP), (what, e_k, e_y)
    assert np.array_equal(got.class_cnt, ref.class_cnt)
    # the indices: distinct, never the excluded one, and the fp64 distance at each of them is the reported one
    srt = np.sort(got.idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all() and (got.idx >= 0).all() and (got.idx < len(case['refs'])).all()
    assert (got.idx != ex[:, None]).all()
    at = np.sqrt(np.take_along_axis(ref.d2, got.idx.astype(np.int64), 1))
    e_at = _err(got.dist, at)
    print("%s: reported distance against the fp64 distance at the reported index: %.3g" % (name, e_at))
    assert e_at <= MARGIN * max(_err(yard.dist, ref.dist), ULP)
    # index rule
    kept = R.decided(ref.d2, ex, k, GAP)
    left_out = 1.0 - kept.mean()
    print("%s: the index rule leaves out %.2f %% of %d queries" % (name, 100 * left_out, m))
    assert left_out <= 0.05
    assert np.array_equal(got.idx[kept], ref.idx[kept])
    # rank rule
    has = case['target'] >= 0
    assert R.rank_decided(ref.d2, case['target'], GAP).all()          # _clear_targets saw to it
    assert np.array_equal(got.rank[kept], ref.rank[kept])
    assert (np.abs(got.rank[~kept] - ref.rank[~kept]) <= 1).all()
    assert (got.rank[~has] == -1).all() and has.any() and (ref.rank[has] > k).any()


def _grid():
    rs = np.random.RandomState(5)
    X = rs.randint(-2, 3, size=(257, 6)).astype(np.float32)
    X[100:120] = X[3]
    return X, np.arange(257) % 3


def test_integer_grid_is_exact():
    """every squared distance is a small integer, exact in fp32: ties everywhere, and nothing may be left out"""
    X, lab = _grid()
    target = (np.arange(257) * 5 + 1) % 257
    case = dict(refs=X, labels=lab, queries=None, k=5, n_classes=3, exclude=None, target=target)
    ref = R.neighbours(**case)
    srt = np.sort(np.where(np.eye(257, dtype=bool), np.inf, ref.d2), axis=1)
    tied = float((srt[:, 4] == srt[:, 5]).mean())
    print("integer grid: %.0f %% of the rows have a tie across the k boundary" % (100 * tied))
    assert tied > 0.3
    got = _run(case)
    assert np.array_equal(got.idx, ref.idx)
    assert np.array_equal(got.class_cnt, ref.class_cnt)
    assert np.array_equal(got.rank, ref.rank)
    exact = np.sqrt(np.take_along_axis(ref.d2, ref.idx, 1))
    assert (np.abs(got.dist.astype(np.float64) - exact) <= ULP * exact).all()
    assert _err(got.class_sum, ref.class_sum) <= MARGIN * max(_err(R.neighbours(dtype=np.float32, **case).class_sum,
                                                                   ref.class_sum), ULP)
    for c in range(100, 120):
        assert got.idx[c, 0] == 3 and got.dist[c, 0] == 0.0
    assert got.idx[3, 0] == 100 and got.dist[3, 0] == 0.0
    # the same rows as queries against themselves, nothing excluded: every row finds itself or its lowest copy first
    cross = _run(dict(case, queries=X, target=None))
    assert np.array_equal(cross.idx, R.neighbours(**dict(case, queries=X, target=None)).idx)
    assert cross.idx[100, 0] == 3 and (cross.rank == -1).all()


EDGES = {
    'list_fills_last': dict(n=7, d=32, k=6, c=4),
    'two_dimensions': dict(n=131, d=2, k=5, c=4),
    'twelve_dimensions': dict(n=131, d=12, k=5, c=4),
    'sixty_four_dimensions_k32': dict(n=200, d=64, k=32, c=4),
    'one_class': dict(n=67, d=32, k=5, c=1),
    'eight_classes': dict(n=150, d=32, k=5, c=8),
    'k32_of_40': dict(n=40, d=32, k=32, c=4),
    'two_queries': dict(n=300, d=32, k=5, c=4, m=2),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edges(name):
    from latent_scores import silhouette
    e = EDGES[name]
    n, d, k, c = e['n'], e['d'], e['k'], e['c']
    X, _ = _clusters(n, seed=81, d=d)
    lab = np.arange(n) % c
    if name == 'eight_classes':
        lab = np.arange(n) % 6                      # class 7 stays empty,
        lab[11] = 6                                 # and class 6 has one member
    queries = target = exclude = None
    if 'm' in e:
        queries = _clusters(e['m'], seed=82, d=d)[0]
        exclude, target = np.array([5, -1]), np.array([-1, 299])
    case = dict(refs=X, labels=lab, queries=queries, k=k, n_classes=c, exclude=exclude, target=target)
    ref, yard = R.neighbours(**case), R.neighbours(dtype=np.float32, **case)
    got = _run(case)
    kept = R.decided(ref.d2, _excluded(case), k, GAP)
    assert kept.mean() >= 0.9 and (target is None or R.rank_decided(ref.d2, target, GAP).all())
    assert np.array_equal(got.idx[kept], ref.idx[kept])
    assert np.array_equal(got.class_cnt, ref.class_cnt) and np.array_equal(got.rank, ref.rank)
    assert _err(got.dist, ref.dist) <= MARGIN * max(_err(yard.dist, ref.dist), ULP)
    assert _err(got.class_sum, ref.class_sum) <= MARGIN * max(_err(yard.class_sum, ref.class_sum), ULP)
    if queries is None:
        s, want = silhouette(got.class_sum, got.class_cnt, lab), R.silhouette_direct(X, lab)
        if name == 'one_class':
            assert np.isnan(s).all() and np.isnan(want).all()
        else:
            assert np.allclose(s, want, rtol=0, atol=1e-5)
        if name == 'eight_classes':
            assert s[11] == 0.0 and (got.class_cnt[:, 7] == 0).all() and got.class_cnt[11, 6] == 0


def _raw_call(lib, t2v_hip, X, lab, k, c, guard, slice_rows, fill):
    """the C entry on outputs of M + guard rows filled with a sentinel, and on inputs with NaN rows past N"""
    n, d = X.shape
    refs = torch.full((n + guard, d), float('nan'), device='cuda')
    refs[:n] = torch.from_numpy(X).cuda()
    labels = torch.full((n + guard,), 99, device='cuda', dtype=torch.int32)
    labels[:n] = torch.from_numpy(lab.astype(np.int32)).cuda()
    outs = [torch.full((n + guard, k), fill, device='cuda', dtype=torch.int32), torch.full((n + guard, k), float(fill), device='cuda'),
            torch.full((n + guard, c), float(fill), device='cuda'), torch.full((n + guard, c), fill, device='cuda', dtype=torch.int32),
            torch.full((n + guard,), fill, device='cuda', dtype=torch.int32)]
    scratch = torch.empty(lib.t2v_latent_scratch_bytes(n, n, c, k, slice_rows), device='cuda', dtype=torch.uint8)
    p = t2v_hip._p
    rc = lib.t2v_latent_neighbours(p(refs), p(labels), n, d, c, None, n, None, None, k, slice_rows, *[p(o) for o in outs],
                                   p(scratch), t2v_hip._stream())
    assert rc == 0, lib.t2v_last_error()
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def test_independent_of_the_split_and_of_padding():
    import t2v_hip
    lib = t2v_hip.load_library()
    case, ref, _ = _reference((1100, 5))
    X, lab, n = case['refs'], case['labels'], 1100
    a = _raw_call(lib, t2v_hip, X, lab, 5, 4, 3, 0, -7)
    b = _raw_call(lib, t2v_hip, X, lab, 5, 4, 3, 0, -7)
    for x, y in zip(a, b):
        assert torch.equal(x[:n], y[:n])                                 # equal inputs, equal bits
        assert bool((x[n:] == -7).all()) and bool((y[n:] == -7).all())   # the sentinels past row M
    assert np.array_equal(a[3][:n].numpy(), ref.class_cnt) and bool((a[4][:n] == -1).all())
    # a slice per tile, slices of four tiles, one slice: other launches, the same bits
    for rows in (128, 512, 1152):
        c = _raw_call(lib, t2v_hip, X, lab, 5, 4, 3, rows, -7)
        for x, y in zip(a, c):
            assert torch.equal(x, y), rows
    w = _run(case, slice_rows=256)
    assert np.array_equal(w.idx, a[0][:n].numpy()) and np.array_equal(w.class_sum, a[2][:n].numpy())


def test_refusals():
    import t2v_hip
    X, lab = _clusters(40)
    x = torch.from_numpy(X).cuda()
    f = t2v_hip.latent_neighbours
    bad = [
        (dict(refs=x[:1], labels=lab[:1]), 'refs'),
        (dict(refs=torch.zeros(16385, 2, device='cuda'), labels=np.zeros(16385, dtype=np.int64)), 'refs'),
        (dict(refs=x, labels=lab, queries=x[:1], k=5), 'queries'),
        (dict(refs=x[:, :1], labels=lab), 'dimensions'),
        (dict(refs=torch.zeros(40, 65, device='cuda'), labels=lab), 'dimensions'),
        (dict(refs=x, labels=lab, queries=x[:, :8]), 'dimensions'),
        (dict(refs=x, labels=lab * 0, n_classes=0), 'n_classes'),
        (dict(refs=x, labels=lab, n_classes=9), 'n_classes'),
        (dict(refs=x, labels=lab, k=0), 'k 0'),
        (dict(refs=x, labels=lab, k=33), 'k 33'),
        (dict(refs=x[:20], labels=lab[:20], k=20), 'k 20'),                      # leave-one-out: 19 to choose from
        (dict(refs=x[:20], labels=lab[:20], queries=x, k=21), 'k 21'),           # nothing excluded: 20
        (dict(refs=x[:20], labels=lab[:20], queries=x, k=20, exclude=[-1] * 40), 'k 20'),
        (dict(refs=x, labels=np.where(np.arange(40) == 17, 4, lab)), r'labels\[17\] = 4'),
        (dict(refs=x, labels=np.where(np.arange(40) == 2, -1, lab)), r'labels\[2\] = -1'),
        (dict(refs=x, labels=lab[:39]), 'labels'),
        (dict(refs=x, labels=lab.astype(np.float32)), 'labels'),
        (dict(refs=x, labels=lab, exclude=np.where(np.arange(40) == 9, 40, -1)), r'exclude\[9\] = 40'),
        (dict(refs=x, labels=lab, target=np.where(np.arange(40) == 39, -2, 0)), r'target\[39\] = -2'),
        (dict(refs=x, labels=lab, queries=x[:3], target=[0, 1]), 'target'),
        (dict(refs=x, labels=lab, slice_rows=100), 'slice_rows'),
        (dict(refs=x.double(), labels=lab), 'refs'),
        (dict(refs=torch.where(torch.arange(40, device='cuda')[:, None] == 4, float('nan'), x), labels=lab), 'finite'),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            f(**kw)
    with pytest.raises(t2v_hip.T2VHipError):
        f(torch.from_numpy(X), lab)
    with pytest.raises(t2v_hip.T2VHipError):
        f(x, lab, torch.from_numpy(X))
    # the C entry's own limits
    lib, p = t2v_hip.load_library(), t2v_hip._p
    lab_d = torch.from_numpy(lab.astype(np.int32)).cuda()
    oi, od = torch.empty(40, 32, device='cuda', dtype=torch.int32), torch.empty(40, 32, device='cuda')
    cs, cc = torch.empty(40, 8, device='cuda'), torch.empty(40, 8, device='cuda', dtype=torch.int32)
    rk, scratch = torch.empty(40, device='cuda', dtype=torch.int32), torch.empty(1 << 20, device='cuda', dtype=torch.uint8)

    def call(R_=x, L=lab_d, N=40, D=32, Cn=4, Q=None, M=40, ex=None, tg=None, k=5, rows=0, out_i=oi, rank=rk, scr=scratch):
        return lib.t2v_latent_neighbours(p(R_), p(L), N, D, Cn, p(Q), M, p(ex), p(tg), k, rows, p(out_i), p(od), p(cs), p(cc),
                                         p(rank), p(scr), t2v_hip._stream())
    assert call() == 0
    for kw in (dict(N=1), dict(N=16385), dict(Q=x, M=1), dict(Q=x, M=16385), dict(D=1), dict(D=65), dict(Cn=0), dict(Cn=9),
               dict(k=0), dict(k=33)):
        assert call(**kw) == -1, kw                                     # T2V_ERR_DIMS
    for kw in (dict(R_=None), dict(L=None), dict(out_i=None), dict(scr=None), dict(tg=lab_d, rank=None), dict(N=20, k=20),
               dict(N=20, Q=x, k=21), dict(N=20, Q=x, ex=lab_d, k=20), dict(rows=64), dict(rows=-128)):
        assert call(**kw) == -2, kw                                     # T2V_ERR_ARG
    assert call(N=20, Q=x, k=20) == 0 and call(rank=None) == 0
    assert lib.t2v_latent_scratch_bytes(1, 40, 4, 5, 0) == 0 and lib.t2v_latent_scratch_bytes(40, 40, 4, 5, 0) > 0
    torch.cuda.synchronize()
