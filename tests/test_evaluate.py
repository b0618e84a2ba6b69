"""Checkpoint scoring, host side: the fp64 reference DTW that the GPU tests compare the kernel with (checked here on
hand-worked cases), evaluation.summarize, the evaluate.py command line, and mel_dtw's refusal of CPU tensors."""
import numpy as np
import pytest
import torch


def dtw_ref(x, y):
    """fp64 DTW distance of x (80, Tx) and y (80, Ty): Euclidean local cost from the differences, symmetric2 steps, no band,
    D(Tx, Ty) / (Tx + Ty).  One numpy operation per anti-diagonal; D[0, 0] = 0 is the virtual corner that makes D(1,1) = 2 d(1,1)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    tx, ty = x.shape[1], y.shape[1]
    d = np.sqrt(sum((x[c][:, None] - y[c][None, :]) ** 2 for c in range(x.shape[0])))
    D = np.full((tx + 1, ty + 1), np.inf)
    D[0, 0] = 0.0
    for k in range(tx + ty - 1):
        i = np.arange(max(0, k - ty + 1), min(tx, k + 1))
        j = k - i
        D[i + 1, j + 1] = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]) + d[i, j], D[i, j] + 2 * d[i, j])
    return D[tx, ty] / (tx + ty)


def _rand(t, seed):
    return np.random.RandomState(seed).randn(80, t) * 2 - 4


def test_reference_single_frames():
    x, y = _rand(1, 0), _rand(1, 1)
    assert dtw_ref(x, y) == pytest.approx(np.linalg.norm(x[:, 0] - y[:, 0]), rel=1e-14)


def test_reference_one_by_n():
    x, y = _rand(1, 2), _rand(6, 3)
    d = np.linalg.norm(x - y, axis=0)                   # d(1, j)
    want = (d[0] + d.sum()) / (1 + 6)
    assert dtw_ref(x, y) == pytest.approx(want, rel=1e-14)
    assert dtw_ref(y, x) == pytest.approx(want, rel=1e-14)


def test_reference_two_by_two_by_hand():
    x, y = np.zeros((80, 2)), np.zeros((80, 2))
    x[0] = [0.0, 3.0]
    y[0] = [1.0, 5.0]                                   # d = [[1, 5], [2, 2]]
    # D(1,1) = 2; D(1,2) = 7; D(2,1) = 4; D(2,2) = min(7 + 2, 4 + 2, 2 + 4) = 6
    assert dtw_ref(x, y) == pytest.approx(6.0 / 4)


def test_reference_identity_and_doubled_frames():
    x = _rand(23, 4)
    assert dtw_ref(x, x) == 0.0
    assert dtw_ref(x, np.repeat(x, 2, axis=1)) == 0.0
    assert dtw_ref(np.repeat(x, 2, axis=1), x) == 0.0


def test_reference_is_symmetric_and_bounded_by_the_diagonal():
    x, y = _rand(17, 5), _rand(17, 6)
    assert dtw_ref(x, y) == pytest.approx(dtw_ref(y, x), rel=1e-14)
    # the diagonal path is one of the candidates: 2 sum d(i, i) / (2 T)
    assert dtw_ref(x, y) <= np.linalg.norm(x - y, axis=0).mean() * (1 + 1e-14)


# ---------------------------------------------------------------------- summarize
def _rec(dtw, n, n_ref, hit, emo):
    return {'dtw': dtw, 'n_frames': n, 'n_ref_frames': n_ref, 'hit_max': hit, 'emotion': emo}


def test_summarize_counts_the_rows_it_leaves_out():
    from evaluation import summarize
    recs = [_rec(1.0, 100, 100, False, 0), _rec(3.0, 50, 100, False, 0), _rec(100.0, 600, 100, True, 0),
            _rec(2.0, 90, 100, False, 1), _rec(50.0, 600, 200, True, 3), _rec(4.0, 120, 100, False, 1),
            _rec(6.0, 110, 100, False, 1)]
    s = summarize(recs)
    o = s['overall']
    assert o['n_rows'] == 7 and o['n_hit_max'] == 2 and o['n_scored'] == 5
    assert o['hit_max_share'] == pytest.approx(2 / 7)
    assert o['dtw_mean'] == pytest.approx((1 + 3 + 2 + 4 + 6) / 5)          # the two rows that never stopped are not in it
    assert o['dtw_median'] == pytest.approx(3.0)
    assert o['length_ratio_mean'] == pytest.approx((1.0 + 0.5 + 6.0 + 0.9 + 3.0 + 1.2 + 1.1) / 7)     # ... but they are here
    e = s['by_emotion']
    assert list(e) == ['neu', 'sad', 'ang', 'hap']
    assert e['neu']['n_rows'] == 3 and e['neu']['n_hit_max'] == 1 and e['neu']['n_scored'] == 2
    assert e['neu']['dtw_mean'] == pytest.approx(2.0) and e['neu']['dtw_median'] == pytest.approx(2.0)
    assert e['sad']['n_scored'] == 3 and e['sad']['dtw_median'] == pytest.approx(4.0) and e['sad']['hit_max_share'] == 0.0
    # an emotion without rows: present, counted as empty, no invented numbers
    assert e['ang'] == {'n_rows': 0, 'n_hit_max': 0, 'hit_max_share': None, 'n_scored': 0, 'dtw_mean': None,
                        'dtw_median': None, 'length_ratio_mean': None}
    # an emotion whose only row never stopped: the row is counted, and there is no distance to report
    assert e['hap']['n_rows'] == 1 and e['hap']['n_hit_max'] == 1 and e['hap']['n_scored'] == 0
    assert e['hap']['dtw_mean'] is None and e['hap']['hit_max_share'] == 1.0
    assert e['hap']['length_ratio_mean'] == pytest.approx(3.0)


def test_summarize_empty_and_bad_label():
    from evaluation import summarize
    s = summarize([])
    assert s['overall']['n_rows'] == 0 and s['overall']['dtw_mean'] is None
    with pytest.raises(ValueError):
        summarize([_rec(1.0, 1, 1, False, 4)])


def test_emotion_names_match_the_synthesizer():
    import evaluation
    import synthesizer
    assert evaluation.EMOTIONS == synthesizer.EMOTIONS


# ---------------------------------------------------------------------- command line
def test_evaluate_cli_defaults():
    import evaluate
    a = evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o.json'])
    assert (a.load_path, a.filelist_path, a.out) == ('c', 'f', 'o.json')
    assert a.batch_size == evaluate.DEFAULT_BATCH_SIZE == 8
    assert a.condition == 'ref' and a.limit is None and a.hparams == ''
    a = evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o', '--condition', 'emotion', '--limit', '3',
                             '--batch_size', '2', '--hparams', 'max_decoder_steps=40'])
    assert (a.condition, a.limit, a.batch_size, a.hparams) == ('emotion', 3, 2, 'max_decoder_steps=40')


@pytest.mark.parametrize('extra', [['--condition', 'style'], ['--batch_size', '0'], ['--limit', '0'], ['--batch_size', 'x']])
def test_evaluate_cli_refuses(extra):
    import evaluate
    with pytest.raises(SystemExit):
        evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o'] + extra)


def test_evaluate_cli_needs_its_paths():
    import evaluate
    with pytest.raises(SystemExit):
        evaluate.parse_args(['--load_path', 'c', '--out', 'o'])


def test_read_rows(tmp_path):
    import evaluate
    f = tmp_path / 'list.txt'
    f.write_text("a.wav|hello|0|2\n\nb.wav|there|1|0\nc.wav|again|0|3\n", encoding='utf-8')
    assert evaluate.read_rows(str(f)) == [('a.wav', 'hello', '0', 2), ('b.wav', 'there', '1', 0), ('c.wav', 'again', '0', 3)]
    assert evaluate.read_rows(str(f), 2) == [('a.wav', 'hello', '0', 2), ('b.wav', 'there', '1', 0)]


# ---------------------------------------------------------------------- no CPU fall-back
def test_mel_dtw_refuses_cpu_tensors():
    import t2v_hip
    x, y = torch.zeros(1, 80, 4), torch.zeros(1, 80, 5)
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.mel_dtw(x, [4], y, [5])
    assert 't2v_mel_dtw' in t2v_hip.EXPORTS and 't2v_mel_dtw_scratch_bytes' in t2v_hip.EXPORTS
