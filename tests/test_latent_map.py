"""The t-SNE latent map, host side: tests/tsne_ref.py (the fp64 numpy restatement that the GPU tests compare the kernels with)
against numbers recorded from scikit-learn's exact t-SNE (tests/golden/tsne.npz, tools/gen_golden_tsne.py), a full descent of
it on a subset, the latent_map.py / extract_latents.py command lines and the four C entries."""
import os
import re

import numpy as np
import pytest

import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSNE_ENTRIES = ('t2v_tsne_scratch_bytes', 't2v_tsne_affinities', 't2v_tsne_gradient', 't2v_tsne_run')


@pytest.fixture(scope='module')
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, 'tsne.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def ref_p(gold):
    """the restatement's P of the fixture X and, entry by entry, how far a correct P may be from the recorded one.

    The recorded P is scikit-learn's: fp64 arithmetic on squared distances stored in fp32, the result stored in fp32 here.
    Against the restatement (fp64 throughout, distances from the differences) that leaves three terms:
    (1) d_ij carries a relative 2^-24, so ln p_j|i = -beta_i d_ij - ln(sum) moves by at most 2 beta_i d_ij 2^-24;
    (2) the binary search stops at |H - log(perplexity)| <= 1e-5; two correct searches may stop one halving apart (an
        entropy within rounding of the threshold), their entropies then differ by at most 2e-5, and with
        dH/dbeta = -beta Var_i(d) that moves ln p_j|i by at most 2e-5 |d_ij - E_i d| / (beta_i Var_i d);
    (3) the stored value carries 2^-24, doubled for the division by sum(P) against 2N."""
    X = gold['X']
    n = len(X)
    d = R.distances(X)
    p, beta = R.conditional(d, float(gold['perplexity']))
    mean = (p * d).sum(axis=1)
    var = (p * (d - mean[:, None]) ** 2).sum(axis=1)
    rel = 2 * beta[:, None] * d * 2.0 ** -24 + 2e-5 * np.abs(d - mean[:, None]) / (beta * var)[:, None]
    t = p * rel
    P = R.joint(p)
    tol = (t + t.T) / (2 * n) + 2.0 ** -23 * P
    return P, tol


def test_ref_affinities_reproduce_scikit_learn(gold, ref_p):
    P, tol = ref_p
    assert str(gold['sklearn_version']) == '1.7.2'
    i, j = gold['p_i'].astype(int), gold['p_j'].astype(int)
    assert (i != j).all() and len(i) == 4096
    err = np.abs(P[i, j] - gold['p_val'].astype(np.float64))
    print("sampled P: max |err| / tol = %.3g, max relative err %.3g" % ((err / tol[i, j]).max(), (err / P[i, j]).max()))
    assert (err <= tol[i, j]).all()
    assert np.abs(P.sum(axis=1) - gold['p_row_sums']).max() <= tol.sum(axis=1).max()
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    assert abs(P.sum() - 1) < 1e-9


@pytest.mark.parametrize("where", ['init', 'spread'])
@pytest.mark.parametrize("tag, ex", [('', 1.0), ('_x12', 12.0)])
def test_ref_gradient_and_kl_reproduce_scikit_learn(gold, ref_p, where, tag, ex):
    """the gradient and the KL value are linear / smooth in P, so the per-entry bound of P above carries through:
    |d grad_i| <= 4 ex sum_j tol_ij w_ij |y_i - y_j|, |d kl| <= ex sum tol_ij (|log(P'/Q)| + 1); the recorded gradient is
    stored in fp32 (2^-24 of its value), the KL value in fp64"""
    P, tol = ref_p
    y = gold[where].astype(np.float64)
    kl, g = R.kl_and_grad(P, y, ex)
    dx, dy = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
    w = 1 / (1 + dx * dx + dy * dy)
    np.fill_diagonal(w, 0)
    bound = 4 * ex * np.stack([(tol * w * np.abs(dx)).sum(axis=1), (tol * w * np.abs(dy)).sum(axis=1)], axis=1)
    want = gold['grad_%s%s' % (where, tag)].astype(np.float64)
    err = np.abs(g - want)
    print("%s%s: grad max |err| %.3g (max |grad| %.3g), kl %.9g against %.9g" % (where, tag, err.max(), np.abs(want).max(), kl,
                                                                            float(gold['kl_%s%s' % (where, tag)])))
    assert (err <= bound + 2.0 ** -23 * np.abs(want) + 1e-30).all()
    off = ~np.eye(len(y), dtype=bool)
    Q = np.maximum(w / w.sum(), R.EPS)
    kl_bound = ex * (tol[off] * (np.abs(np.log(np.maximum(ex * P[off], R.EPS) / Q[off])) + 1)).sum()
    assert abs(kl - float(gold['kl_%s%s' % (where, tag)])) <= kl_bound + 1e-12


def test_ref_float32_yardstick_is_close_to_float64(gold):
    """the fp32 run of the same formulas is what the GPU tests measure the kernels against: it has to be fp32-close itself"""
    X = gold['X'][:120]
    P64, P32 = R.affinities(X, 10.0), R.affinities(X, 10.0, np.float32)
    assert P32.dtype == np.float32
    big = P64 > 1e-12
    assert (np.abs(P32 - P64)[big] / P64[big]).max() < 1e-2          # a differing stop of the search moves a row by ~1e-4
    k64, g64 = R.kl_and_grad(P64, gold['spread'][:120], 1.0)
    k32, g32 = R.kl_and_grad(P64, gold['spread'][:120], 1.0, np.float32)
    assert g32.dtype == np.float32 and np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max() and abs(k32 - k64) <= 1e-4 * k64


def test_ref_descent_separates_the_clusters(gold):
    n = 150
    X, labels = gold['X'][:n], gold['labels'][:n]
    P = R.affinities(X, float(gold['perplexity']))
    y, trace = R.descend(P, gold['init'][:n], 1000)
    assert len(trace) == 20 and np.isfinite(trace).all() and np.isfinite(y).all()
    assert (np.diff(trace[5:]) <= 0).all()                        # after the exaggeration phase the objective only falls
    in_x, in_map = R.knn_label_agreement(X, labels), R.knn_label_agreement(y, labels)
    print("150 points: KL %.4f, 5-NN label agreement %.3f in X, %.3f in the map" % (trace[-1], in_x, in_map))
    assert in_map >= in_x


def test_ref_duplicates_give_no_nan():
    rs = np.random.RandomState(3)
    X = rs.standard_normal((40, 8)).astype(np.float32)
    X[5:15] = X[5]
    for dtype in (np.float64, np.float32):
        P = R.affinities(X, 5.0, dtype)
        assert np.isfinite(P).all() and np.array_equal(P, P.T)
    P = R.affinities(np.ones((12, 4), dtype=np.float32), 3.0)       # every distance 0: a uniform row
    assert np.isfinite(P).all() and np.allclose(P[0, 1:], 1 / (12 * 11))


def test_init_recipe_matches_the_fixture(gold):
    import t2v_hip
    assert np.array_equal(R.init(600, 0), gold['init'])
    assert np.array_equal(t2v_hip.tsne_init(600, 0).numpy(), gold['init'])
    assert t2v_hip.tsne_learning_rate(600) == R.learning_rate(600) == 50.0
    assert t2v_hip.tsne_learning_rate(12000) == 250.0


# ---------------------------------------------------------------------------------------------- command lines
def test_latent_map_parser_defaults():
    import latent_map as L
    a = L.parse_args(['--latents', 'in.npz', '--out', 'map.npz'])
    assert (a.latents, a.out, a.key, a.perplexity, a.n_iter, a.seed, a.png) == ('in.npz', 'map.npz', 'mus', 30.0, 1000, 0, None)
    a = L.parse_args(['--latents', 'in.npz', '--out', 'map.npz', '--key', 'prosody', '--perplexity', '12.5', '--n_iter', '300',
                      '--seed', '4', '--png', 'm.png'])
    assert (a.key, a.perplexity, a.n_iter, a.seed, a.png) == ('prosody', 12.5, 300, 4, 'm.png')
    for bad in (['--key', 'logvar'], ['--perplexity', '0'], ['--n_iter', '0']):
        with pytest.raises(SystemExit):
            L.parse_args(['--latents', 'in.npz', '--out', 'map.npz'] + bad)
    with pytest.raises(SystemExit):
        L.parse_args(['--latents', 'in.npz'])


def test_latent_map_rejects_a_perplexity_of_a_third_of_the_points(tmp_path):
    import latent_map as L
    src = str(tmp_path / 'lat.npz')
    np.savez(src, mus=np.zeros((90, 32), np.float32), zs=np.zeros((90, 32), np.float32), prosody=np.zeros((90, 512), np.float32),
             emotions=np.zeros(90, np.int64), paths=np.array(['p'] * 90))
    out = str(tmp_path / 'map.npz')
    for perplexity in ('30', '31'):                     # 3 * 30 = N is already outside
        with pytest.raises(SystemExit, match="perplexity"):
            L.main(['--latents', src, '--out', out, '--perplexity', perplexity])
    assert not os.path.exists(out)


def test_extract_latents_keeps_its_command_line():
    import extract_latents as X
    a = X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz'])
    assert (a.load_path, a.filelist_path, a.out, a.batch_size, a.hparams, a.tsne) == ('ck', 'f.txt', 'o.npz', 64, '', None)
    a = X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz', '--batch_size', '8', '--hparams',
                      'z_latent_dim=16'])
    assert a.batch_size == 8 and a.hparams == 'z_latent_dim=16' and a.tsne is None
    assert X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--tsne', '--out', 'o.npz']).tsne == 'mus'
    assert X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz', '--tsne', 'zs']).tsne == 'zs'
    with pytest.raises(SystemExit):
        X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz', '--tsne', 'logvars'])


# ---------------------------------------------------------------------------------------------- C ABI, host-side checks
def test_tsne_entries_are_declared_exported_and_bound():
    """the header-parsing recipe of test_host_logic.py, on the four new entries"""
    import t2v_hip
    with open(os.path.join(ROOT, 'include', 't2vae.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    protos = dict(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    lib = t2v_hip.load_library()
    for name in TSNE_ENTRIES:
        assert name in protos and name in t2v_hip.EXPORTS and hasattr(lib, name), name
        assert protos[name].count(',') + 1 == len(getattr(lib, name).argtypes), name
    assert re.search(r'#define\s+T2V_TSNE_MAX_POINTS\s+16384\b', src) and t2v_hip.TSNE_MAX_POINTS == 16384
    m = re.search(r'#define\s+T2V_TSNE_EXAG_ITERS\s+(\d+)', src)
    assert int(m.group(1)) == t2v_hip.TSNE_EXAG_ITERS == R.EXAG_ITERS


def test_scratch_size_and_refused_sizes():
    import t2v_hip
    lib = t2v_hip.load_library()
    a, b, c = (lib.t2v_tsne_scratch_bytes(n, 32) for n in (97, 1232, 16384))
    assert 0 < a < b < c < 64 << 20
    assert lib.t2v_tsne_scratch_bytes(16385, 32) == 0 and lib.t2v_tsne_scratch_bytes(600, 65) == 0
    assert lib.t2v_tsne_scratch_bytes(600, 1) == 0 and lib.t2v_tsne_scratch_bytes(3, 2) == 0
    # sizes and arguments are refused before any pointer is used or anything is launched
    assert lib.t2v_tsne_affinities(None, 16385, 32, 30.0, None, None, None) == -1
    assert lib.t2v_tsne_affinities(None, 600, 65, 30.0, None, None, None) == -1
    assert lib.t2v_tsne_affinities(None, 600, 32, 30.0, None, None, None) == -2
    assert lib.t2v_tsne_gradient(None, None, 16385, 1.0, None, None, None, None) == -1
    assert lib.t2v_tsne_gradient(None, None, 600, 1.0, None, None, None, None) == -2
    assert lib.t2v_tsne_run(None, None, 16385, 10, 50.0, None, None, None) == -1
    assert lib.t2v_tsne_run(None, None, 600, 10, 50.0, None, None, None) == -2


def test_tsne_refuses_cpu_tensors():
    import torch
    import t2v_hip
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.tsne(torch.zeros(100, 32))
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.tsne_affinities(torch.zeros(100, 32), 10.0)
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.tsne_gradient(torch.zeros(100, 100), torch.zeros(100, 2))
