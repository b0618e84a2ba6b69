"""Frame-aligned scores, host side: the fp64 reference (aligned_ref) on hand-worked cases, evaluation.aligned_fields and
summarize with the aligned keys, the --aligned flag, and the new names in the bindings and the header."""
import math
import os

import numpy as np
import pytest
import torch

import aligned_ref as AR
from test_evaluate import dtw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(t, seed):
    return np.random.RandomState(seed).randn(13, t)


# ---------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('tx,ty', [(1, 1), (1, 6), (6, 1), (17, 23), (40, 31)])
def test_reference_distance_is_the_existing_recurrence(tx, ty):
    x, y = _rand(tx, tx), _rand(ty, 100 + ty)
    dist, path = AR.dtw_path(x, y)
    assert dist == dtw_ref(x, y)
    assert AR.path_is_valid(path, tx, ty) and max(tx, ty) <= len(path) <= tx + ty - 1
    assert AR.path_cost(x, y, path) == pytest.approx(dist, rel=1e-13)


def test_reference_cepstrum_is_the_formula():
    m = np.random.RandomState(3).randn(80, 5) * 2 - 4
    c, scale = AR.cepstrum(m)
    for k in (1, 7, 13):
        for t in (0, 4):
            want = math.sqrt(2 / 80) * sum(m[n, t] * math.cos(math.pi * k * (n + 0.5) / 80) for n in range(80))
            assert c[k - 1, t] == pytest.approx(want, rel=1e-12, abs=1e-12)
    assert c.shape == (13, 5) and (scale >= np.abs(c) - 1e-12).all()
    # a flat spectrum has no cepstrum above c_0, and c_1 sees a tilt
    assert np.abs(AR.cepstrum(np.full((80, 2), -3.0))[0]).max() < 1e-12
    assert AR.cepstrum(np.linspace(0, -8, 80)[:, None])[0][0, 0] > 1.0


def test_binding_table_is_the_reference_table_rounded_once():
    import t2v_hip
    t = t2v_hip.cepstrum_table()
    assert t.dtype == np.float32 and t.shape == (13, 80) and not t.flags.writeable
    assert np.array_equal(t, AR.cepstrum_table().astype(np.float32))


def test_self_alignment_is_the_diagonal():
    x = _rand(23, 4)
    dist, path = AR.dtw_path(x, x)
    assert dist == 0.0 and np.array_equal(path, np.stack([np.arange(23)] * 2, 1))
    counts, sums, _ = AR.path_scores(x, x, path)
    d = AR.derived(counts, sums, f0=False)
    assert d['mcd_db'] == 0.0 and d['warp_dev'] == 0.0 and counts['n_points'] == 23


def test_doubled_frames_give_the_staircase():
    x = _rand(11, 5)
    y = np.repeat(x, 2, axis=1)
    dist, path = AR.dtw_path(x, y)
    j = np.arange(22)
    assert dist == 0.0 and np.array_equal(path, np.stack([j // 2, j], 1))
    counts, sums, _ = AR.path_scores(x, y, path)
    assert counts['n_points'] == 22 and AR.derived(counts, sums, f0=False)['mcd_db'] == 0.0


def test_all_zero_3x5_goes_diagonal_first():
    dist, path = AR.dtw_path(np.zeros((13, 3)), np.zeros((13, 5)))
    assert dist == 0.0
    assert path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    _, path = AR.dtw_path(np.zeros((13, 5)), np.zeros((13, 3)))
    assert path.tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]


def test_3x3_with_ties_by_hand():
    x, y = np.zeros((13, 3)), np.zeros((13, 3))
    x[0] = [0.0, 1.0, 1.0]
    y[0] = [0.0, 0.0, 1.0]
    # d = [[0, 0, 1], [1, 1, 0], [1, 1, 0]]
    # D(0,0) = 0; D(0,1) = 0; D(0,2) = 1; D(1,0) = 1; D(2,0) = 2
    # D(1,1) = min(0 + 2, 0 + 1, 1 + 1) = 1 from (0,1);  D(1,2) = min(0 + 0, 1 + 0, 1 + 0) = 0 from the diagonal (0,1)
    # D(2,1) = min(1 + 2, 1 + 1, 2 + 1) = 2 from (1,1);  D(2,2) = min(1 + 0, 0 + 0, 2 + 0) = 0 from (1,2)
    # walk: (2,2) <- (1,2) <- (0,1) <- (0,0)
    dist, path = AR.dtw_path(x, y)
    assert dist == 0.0 and path.tolist() == [[0, 0], [0, 1], [1, 2], [2, 2]]
    # a three-way tie at (1,1): d = 0 everywhere but d(0,1) = d(1,0) = 0 too -> the diagonal wins over both
    x[0], y[0] = [0.0, 0.0, 2.0], [0.0, 0.0, 2.0]
    _, path = AR.dtw_path(x, y)
    assert path.tolist() == [[0, 0], [1, 1], [2, 2]]
    # (i-1, j) before (i, j-1): d = [[0, 0], [1, 1]] -> D(1,1) = min(0 + 2, 0 + 1, 1 + 1) = 1 from (0,1) = (i-1, j);
    # d = [[0, 1], [0, 1]] -> D(1,1) = min(0 + 2, 1 + 1, 0 + 1) = 1 from (1,0) = (i, j-1)
    a, b = np.zeros((13, 2)), np.zeros((13, 2))
    a[0] = [0.0, 1.0]
    assert AR.dtw_path(a, b)[1].tolist() == [[0, 0], [0, 1], [1, 1]]
    assert AR.dtw_path(b, a)[1].tolist() == [[0, 0], [1, 0], [1, 1]]
    # and with both neighbours equal and cheaper than the diagonal, (i-1, j) is taken:
    # d = [[1, 0], [0, 1]]: D(0,0) = 2, D(0,1) = 2, D(1,0) = 2, D(1,1) = min(2 + 2, 2 + 1, 2 + 1) = 3 from (0,1)
    a[0], b[0] = [0.0, 1.0], [1.0, 0.0]
    assert AR.dtw_path(a, b)[1].tolist() == [[0, 0], [0, 1], [1, 1]]


def _diag(t):
    return np.stack([np.arange(t)] * 2, 1)


def test_f0_cases():
    x = _rand(20, 6)
    fy = np.linspace(100.0, 300.0, 20)
    counts, sums, _ = AR.path_scores(x, x, _diag(20), 2 * fy, fy)
    d = AR.derived(counts, sums)
    assert (d['gpe'], d['vde'], d['ffe']) == (1.0, 0.0, 1.0)
    assert d['lf0_rmse_cents'] == pytest.approx(1200.0) and d['lf0_bias_cents'] == pytest.approx(1200.0)
    assert d['lf0_corr'] == pytest.approx(1.0)
    counts, sums, _ = AR.path_scores(x, x, _diag(20), np.zeros(20), fy)
    d = AR.derived(counts, sums)
    assert d['vde'] == 1.0 and d['ffe'] == 1.0 and d['gpe'] is None and d['lf0_rmse_cents'] is None and d['lf0_corr'] is None
    assert counts == {'n_points': 20, 'n_both': 0, 'n_vde': 20, 'n_gpe': 0}
    counts, sums, _ = AR.path_scores(x, x, _diag(20), fy, fy)
    d = AR.derived(counts, sums)
    assert (d['gpe'], d['vde'], d['ffe'], d['lf0_rmse_cents'], d['lf0_bias_cents']) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert d['lf0_corr'] == pytest.approx(1.0)
    # no tracks: unvoiced on both sides is no voicing error
    counts, sums, _ = AR.path_scores(x, x, _diag(20))
    assert counts == {'n_points': 20, 'n_both': 0, 'n_vde': 0, 'n_gpe': 0}


def test_warp_dev_is_zero_for_a_linear_stretch_only():
    x = _rand(9, 7)
    j = np.arange(17)
    lin = np.stack([j // 2, j], 1)                       # (0,0) .. (8,16): i / 8 against j / 16 differ by at most 1 / 16
    counts, sums, _ = AR.path_scores(x, np.repeat(x, 2, 1)[:, :17], lin)
    assert AR.derived(counts, sums, f0=False)['warp_dev'] == pytest.approx(np.abs((j // 2) / 8 - j / 16).mean())
    counts, sums, _ = AR.path_scores(x, x, _diag(9))
    assert AR.derived(counts, sums, f0=False)['warp_dev'] == 0.0
    corner = np.asarray([(0, k) for k in range(9)] + [(k, 8) for k in range(1, 9)])
    counts, sums, _ = AR.path_scores(x, x, corner)
    assert AR.derived(counts, sums, f0=False)['warp_dev'] == pytest.approx((36 / 8 + 28 / 8) / 17)      # |0 - k/8| for k = 0..8, then |k/8 - 1| for k = 1..8


# ---------------------------------------------------------------------- aligned_fields
def test_aligned_fields_equals_the_reference_and_its_none_rules():
    from evaluation import ALIGNED_KEYS, aligned_fields
    rs = np.random.RandomState(8)
    x, y = _rand(30, 9), _rand(41, 10)
    _, path = AR.dtw_path(x, y)
    fx = np.where(rs.rand(30) < 0.3, 0.0, rs.uniform(60, 500, 30))
    fy = np.where(rs.rand(41) < 0.3, 0.0, rs.uniform(60, 500, 41))
    counts, sums, _ = AR.path_scores(x, y, path, fx, fy)
    crow = [counts[k] for k in ('n_points', 'n_both', 'n_vde', 'n_gpe')]
    srow = [sums[k] for k in ('sum_d', 'sum_e', 'sum_e2', 's_xx', 's_yy', 's_xy', 'sum_warp')] + [0.0]
    got = aligned_fields(crow, srow)
    assert tuple(got) == ALIGNED_KEYS
    want = AR.derived(counts, sums)
    assert all(got[k] == pytest.approx(want[k], rel=1e-12) for k in ALIGNED_KEYS)
    assert got['mcd_db'] == pytest.approx(10 / math.log(10) * math.sqrt(2) * sums['sum_d'] / len(path))
    # no tracks: mcd and warp only
    got = aligned_fields(crow, srow, f0=False)
    assert got['mcd_db'] == want['mcd_db'] and got['warp_dev'] == want['warp_dev']
    assert all(got[k] is None for k in ALIGNED_KEYS if k not in ('mcd_db', 'warp_dev'))
    # no both-voiced point: gpe and the log-F0 values are None, vde and ffe are not
    got = aligned_fields([10, 0, 4, 0], [5.0, 0, 0, 0, 0, 0, 1.0, 0])
    assert got['vde'] == 0.4 and got['ffe'] == 0.4 and got['warp_dev'] == 0.1
    assert got['gpe'] is None and got['lf0_rmse_cents'] is None and got['lf0_bias_cents'] is None and got['lf0_corr'] is None
    # one both-voiced point, or a zero variance: no correlation
    got = aligned_fields([10, 1, 0, 1], [5.0, 100.0, 10000.0, 0, 0, 0, 0, 0])
    assert got['gpe'] == 1.0 and got['lf0_rmse_cents'] == 100.0 and got['lf0_bias_cents'] == 100.0 and got['lf0_corr'] is None
    assert aligned_fields([10, 5, 0, 0], [5.0, 0, 0, 0.0, 2.0, 0.0, 0, 0])['lf0_corr'] is None
    assert aligned_fields([10, 5, 0, 0], [5.0, 0, 0, 2.0, 2.0, -2.0, 0, 0])['lf0_corr'] == -1.0
    # a refused pair
    assert aligned_fields([0, 0, 0, 0], [float('nan')] * 8) == dict.fromkeys(ALIGNED_KEYS)


# ---------------------------------------------------------------------- summarize
def _rec(dtw, hit, emo, **kw):
    r = {'dtw': dtw, 'n_frames': 100, 'n_ref_frames': 100, 'hit_max': hit, 'emotion': emo}
    r.update(kw)
    return r


def _al(mcd, warp, **kw):
    from evaluation import ALIGNED_KEYS
    d = dict.fromkeys(ALIGNED_KEYS)
    d.update(mcd_db=mcd, warp_dev=warp, **kw)
    return d


def test_summarize_with_the_aligned_keys():
    from evaluation import summarize
    recs = [_rec(1.0, False, 0, **_al(4.0, 0.1, vde=0.2, gpe=0.5, ffe=0.4, lf0_rmse_cents=100.0, lf0_bias_cents=5.0, lf0_corr=0.5)),
            _rec(2.0, False, 0, **_al(6.0, 0.3, vde=0.4, ffe=0.4)),                     # no both-voiced point
            _rec(9.0, True, 0, **_al(50.0, 0.9, vde=1.0, ffe=1.0)),                     # never stopped: not in the means
            _rec(3.0, False, 1, **_al(8.0, 0.2))]                                       # no tracks at all
    s = summarize(recs)
    o = s['overall']
    assert o['n_aligned'] == 3 and o['n_scored'] == 3
    assert o['mcd_db_mean'] == pytest.approx(6.0) and o['warp_dev_mean'] == pytest.approx(0.2)
    assert o['vde_mean'] == pytest.approx(0.3) and o['ffe_mean'] == pytest.approx(0.4)
    assert o['gpe_mean'] == 0.5 and o['lf0_rmse_cents_mean'] == 100.0 and o['lf0_corr_mean'] == 0.5
    assert 'lf0_bias_cents_mean' not in o
    e = s['by_emotion']
    assert e['neu']['n_aligned'] == 2 and e['neu']['mcd_db_mean'] == pytest.approx(5.0)
    assert e['sad']['n_aligned'] == 1 and e['sad']['mcd_db_mean'] == 8.0 and e['sad']['vde_mean'] is None
    assert e['ang']['n_aligned'] == 0 and e['ang']['mcd_db_mean'] is None and e['ang']['gpe_mean'] is None


def test_summarize_without_the_keys_is_todays_dict():
    from evaluation import summarize
    recs = [_rec(1.0, False, 0), _rec(3.0, False, 1), _rec(100.0, True, 3)]
    s = summarize(recs)
    plain = {'n_rows', 'n_hit_max', 'hit_max_share', 'n_scored', 'dtw_mean', 'dtw_median', 'length_ratio_mean'}
    assert set(s) == {'overall', 'by_emotion'} and set(s['overall']) == plain
    assert all(set(v) == plain for v in s['by_emotion'].values())
    assert s['overall'] == {'n_rows': 3, 'n_hit_max': 1, 'hit_max_share': 1 / 3, 'n_scored': 2, 'dtw_mean': 2.0,
                            'dtw_median': 2.0, 'length_ratio_mean': 1.0}


# ---------------------------------------------------------------------- command line, names
def test_evaluate_cli_aligned_flag():
    import evaluate
    base = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o.json']
    assert evaluate.parse_args(base).aligned is False
    a = evaluate.parse_args(base + ['--aligned'])
    assert a.aligned is True and a.prosody is False
    a = evaluate.parse_args(base + ['--aligned', '--prosody'])
    assert a.aligned and a.prosody
    assert '--aligned' in evaluate.__doc__


def test_new_names_are_exported_and_declared():
    import evaluation
    import t2v_hip
    names = ('t2v_mel_cepstrum', 't2v_cep_dtw_scratch_bytes', 't2v_cep_dtw_path', 't2v_path_scores')
    with open(os.path.join(ROOT, 'include', 't2vae.h'), encoding='utf-8') as f:
        header = f.read()
    for n in names:
        assert n in t2v_hip.EXPORTS and n + '(' in header
    assert '#define T2V_NCEP 13' in header and t2v_hip.NCEP == AR.NCEP == 13
    assert t2v_hip.ALIGNED_COUNTS == ('n_points', 'n_both', 'n_vde', 'n_gpe')
    assert t2v_hip.ALIGNED_SUMS == ('sum_d', 'sum_e', 'sum_e2', 's_xx', 's_yy', 's_xy', 'sum_warp')
    assert evaluation.ALIGNED_KEYS == ('mcd_db', 'vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_bias_cents', 'lf0_corr', 'warp_dev')
    assert evaluation.MCD_DB == pytest.approx(AR.MCD_DB)


def test_aligned_scores_refuses_cpu_tensors():
    import t2v_hip
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.aligned_scores(torch.zeros(1, 13, 4), [4], torch.zeros(1, 13, 5), [5])
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.mel_cepstrum(torch.zeros(1, 80, 4), [4])
