"""Forced alignment, host side (no GPU): the fp64 reference of the monotonic search (tests/mas_ref.py) against brute force
over all paths, the arithmetic of evaluation.DURATION_KEYS on hand-made durations, the command lines of evaluate.py and
extract_durations.py, the host checks of t2v_hip.mas, and that nothing changes without the flag."""
import inspect
import math

import numpy as np
import pytest
import torch

import mas_ref


# ---------------------------------------------------------------------- the reference against brute force
@pytest.mark.parametrize('S', [1, 2, 3])
def test_reference_equals_brute_force_over_all_paths(S):
    rng = np.random.RandomState(10 + S)
    checked = 0
    for n in range(1, 8):
        for L in range(1, 5):
            for trial in range(3):
                A = rng.dirichlet(np.ones(L) * 0.5, size=n).astype(np.float32)
                if trial == 2:                                          # zeros, a NaN and a value under the floor: all the floor
                    A[rng.randint(n), rng.randint(L)] = 0.0
                    A[rng.randint(n), rng.randint(L)] = np.nan
                    A[rng.randint(n), rng.randint(L)] = 1e-30
                ref = mas_ref.search(A, n, L, S)
                if not mas_ref.feasible(n, L, S):
                    assert ref is None
                    continue
                best, paths = mas_ref.brute_force(A, n, L, S)
                assert paths and mas_ref.is_feasible_path(ref['path'], n, L, S)
                assert ref['total'] == pytest.approx(best, rel=1e-13, abs=1e-13)
                assert mas_ref.path_score(A, ref['path'], L) == pytest.approx(best, rel=1e-13, abs=1e-13)
                assert ref['durations'].sum() == n and len(ref['durations']) == L
                assert (ref['starts'] == np.concatenate([[0], np.cumsum(ref['durations'])[:-1]])).all()
                checked += 1
    assert checked > 40


def test_reference_tie_rule_staying_beats_advancing():
    for S in (1, 2, 3):
        for n, L in ((5, 3), (7, 4), (4, 4), (6, 1)):
            if not mas_ref.feasible(n, L, S):
                continue
            A = np.full((n, L), 1.0 / L, dtype=np.float32)             # every path ties exactly
            p = mas_ref.search(A, n, L, S)['path']
            # the walk back takes the smallest step whose predecessor lies in the band: p[t-1] = min(p[t], (t - 1) S), so the
            # path advances as early and as fast as the band allows and then stays
            want = np.minimum(L - 1, np.arange(n) * S)
            assert (p == want).all(), (S, n, L, p, want)


def test_reference_floor_and_hand_case():
    assert mas_ref.FLOOR == float(np.float32(1e-8)) and mas_ref.LN_FLOOR == pytest.approx(18.42, abs=0.01)
    A = np.array([[0.9, 0.1], [0.2, 0.8], [0.6, 0.4]], dtype=np.float32)
    r = mas_ref.search(A, 3, 2, 1)                                      # 0,0,1: .9 .2 .4 = .072   0,1,1: .9 .8 .4 = .288
    assert r['path'].tolist() == [0, 1, 1] and r['durations'].tolist() == [1, 2] and r['starts'].tolist() == [0, 1]
    assert r['total'] == pytest.approx(math.log(np.float32(0.9)) + math.log(np.float32(0.8)) + math.log(np.float32(0.4)))
    skipped = mas_ref.search(np.full((2, 3), 1 / 3, dtype=np.float32), 2, 3, 2)
    assert skipped['path'].tolist() == [0, 2] and skipped['durations'].tolist() == [1, 0, 1] and skipped['starts'].tolist() == [0, 1, 1]
    assert mas_ref.search(A, 1, 2, 1) is None
    assert mas_ref.gap_bound(6) == pytest.approx(12 * (2.0 ** -24 * 6 * mas_ref.LN_FLOOR + 2.0 ** -19))


# ---------------------------------------------------------------------- DURATION_KEYS arithmetic
def test_duration_fields_by_hand():
    from evaluation import DURATION_KEYS, duration_fields
    f = duration_fields([1, 2, 3, 4], [2, 2, 5, 3], -0.5, -0.25)
    assert tuple(f) == DURATION_KEYS
    assert f['dur_rmse_frames'] == pytest.approx(math.sqrt((1 + 0 + 4 + 1) / 4))
    assert f['dur_corr'] == pytest.approx(np.corrcoef([1, 2, 3, 4], [2, 2, 5, 3])[0, 1])
    ratio = np.log(np.array([2, 3, 4, 5]) / np.array([3, 3, 6, 4]))
    assert f['dur_log_ratio_spread'] == pytest.approx(ratio.std())
    assert f['align_logp_syn'] == -0.5 and f['align_logp_rec'] == -0.25
    same = duration_fields([3, 1, 2], [3, 1, 2], -1.0, -1.0)
    assert same['dur_rmse_frames'] == 0.0 and same['dur_corr'] == pytest.approx(1.0) and same['dur_log_ratio_spread'] == 0.0
    flat = duration_fields([2, 2, 2], [1, 3, 2], -1.0, -1.0)            # a zero variance: no correlation
    assert flat['dur_corr'] is None and flat['dur_rmse_frames'] == pytest.approx(math.sqrt(2 / 3))
    assert duration_fields([5], [3], -1.0, -1.0)['dur_corr'] is None
    # a side without a path: no comparison, and no log-probability on that side
    half = duration_fields(None, [1, 2], None, -0.3)
    assert half == {'dur_rmse_frames': None, 'dur_corr': None, 'dur_log_ratio_spread': None, 'align_logp_syn': None,
                    'align_logp_rec': -0.3}
    assert duration_fields([1, 2], None, -0.3, float('nan'))['align_logp_rec'] is None
    with pytest.raises(ValueError):
        duration_fields([1, 2], [1, 2, 3], -1.0, -1.0)


def test_segment_f0_fields_by_hand():
    from evaluation import DURATION_F0_KEYS, segment_f0_fields
    # symbols 0 and 2 are voiced on both sides; 1 only in the synthesis, 3 in neither
    f = segment_f0_fields([400.0, 300.0, 220.0, 0.0], [2, 1, 1, 0], [200.0, 0.0, 440.0, 0.0], [1, 0, 2, 0])
    assert tuple(f) == DURATION_F0_KEYS
    assert f['seg_f0_rmse_cents'] == pytest.approx(0.0, abs=1e-9)       # 400 / 2 = 200 and 220 = 440 / 2
    assert f['seg_f0_corr'] == pytest.approx(1.0)
    g = segment_f0_fields([400.0, 220.0], [1, 1], [200.0, 220.0], [1, 1])
    assert g['seg_f0_rmse_cents'] == pytest.approx(1200.0 * math.sqrt(0.5))         # one octave and nothing
    assert segment_f0_fields([100.0], [1], [100.0], [1]) == {'seg_f0_rmse_cents': 0.0, 'seg_f0_corr': None}
    assert segment_f0_fields([0.0], [0], [100.0], [1]) == dict.fromkeys(DURATION_F0_KEYS)
    assert segment_f0_fields(None, None, [100.0], [1]) == dict.fromkeys(DURATION_F0_KEYS)


def _rec(emo, hit=False, **more):
    return dict({'dtw': 1.0, 'n_frames': 10, 'n_ref_frames': 10, 'hit_max': hit, 'emotion': emo}, **more)


def test_summarize_means_of_the_duration_keys():
    from evaluation import DURATION_KEYS, duration_fields, summarize
    recs = [_rec(0, **duration_fields([1, 2], [2, 1], -1.0, -2.0)), _rec(0, **duration_fields([2, 2, 1], [2, 2, 1], -3.0, -4.0)),
            _rec(1, **duration_fields(None, [1, 1], None, -0.5)), _rec(1, True, **duration_fields([1, 2], [3, 4], -9.0, -9.0))]
    s = summarize(recs)
    o = s['overall']
    assert o['n_durations'] == 2                                        # not the row without a path, not the one that never stopped
    assert o['dur_rmse_frames_mean'] == pytest.approx((1.0 + 0.0) / 2)
    assert o['align_logp_syn_mean'] == pytest.approx(-2.0) and o['align_logp_rec_mean'] == pytest.approx((-2 - 4 - 0.5) / 3)
    assert s['by_emotion']['sad']['n_durations'] == 0 and s['by_emotion']['sad']['dur_rmse_frames_mean'] is None
    assert s['by_emotion']['sad']['align_logp_rec_mean'] == pytest.approx(-0.5)
    assert all(k + '_mean' in o for k in DURATION_KEYS) and 'seg_f0_corr_mean' not in o
    with_f0 = summarize([dict(r, seg_f0_rmse_cents=50.0, seg_f0_corr=None) for r in recs])['overall']
    assert with_f0['seg_f0_rmse_cents_mean'] == pytest.approx(50.0) and with_f0['seg_f0_corr_mean'] is None


def test_without_the_flag_nothing_has_a_new_key():
    import evaluation
    from evaluation import DURATION_F0_KEYS, DURATION_KEYS, summarize
    from synthesizer import Synthesizer
    s = summarize([_rec(0), _rec(2, True)])
    assert set(s) == {'overall', 'by_emotion'}
    assert set(s['overall']) == {'n_rows', 'n_hit_max', 'hit_max_share', 'n_scored', 'dtw_mean', 'dtw_median', 'length_ratio_mean'}
    others = set()
    for name in ('PROSODY_KEYS', 'ALIGNMENT_KEYS', 'ALIGNED_KEYS', 'ENERGY_KEYS', 'ENERGY_ALIGNED_KEYS', 'VOICE_KEYS',
                 'VOICE_ALIGNED_KEYS', 'STYLE_KEYS'):
        others |= set(getattr(evaluation, name))
    assert not (set(DURATION_KEYS) | set(DURATION_F0_KEYS)) & (others | set(_rec(0)))
    sig = inspect.signature(Synthesizer.evaluate).parameters
    assert sig['durations'].default is False and sig['max_step'].default == 1
    sig = inspect.signature(Synthesizer.alignment).parameters
    assert sig['mas'].default is False
    assert inspect.signature(Synthesizer.durations).parameters['batch_size'].default == 8


# ---------------------------------------------------------------------- command lines
BASE = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']


def test_evaluate_cli_durations():
    import evaluate
    a = evaluate.parse_args(BASE)
    assert a.durations is False and a.max_step == evaluate.DEFAULT_MAX_STEP == 1
    a = evaluate.parse_args(BASE + ['--durations', '--max_step', '3', '--prosody'])
    assert a.durations is True and a.max_step == 3 and a.prosody
    for extra in (['--max_step', '0'], ['--max_step', '4'], ['--max_step', 'x'],
                  ['--durations', '--prosody', '--speed', '1.5'], ['--durations', '--prosody', '--pitch', '2']):
        with pytest.raises(SystemExit):
            evaluate.parse_args(BASE + extra)
    assert evaluate.parse_args(BASE + ['--durations', '--speed', '1.5']).speed == 1.5      # without --prosody no waveform is read


def test_extract_durations_cli():
    import extract_durations as X
    a = X.parse_args(BASE)
    assert (a.load_path, a.filelist_path, a.out) == ('c', 'f', 'o')
    assert a.max_step == 1 and a.min_logp is None and a.weights is None and a.batch_size == X.DEFAULT_BATCH_SIZE == 8
    a = X.parse_args(BASE + ['--weights', 'ema', '--max_step', '2', '--min_logp', '-3.5', '--batch_size', '4'])
    assert (a.weights, a.max_step, a.min_logp, a.batch_size) == ('ema', 2, -3.5, 4)
    for extra in (['--max_step', '0'], ['--max_step', '4'], ['--min_logp', '0.5'], ['--min_logp', 'x'], ['--batch_size', '0'],
                  ['--weights', 'best']):
        with pytest.raises(SystemExit):
            X.parse_args(BASE + extra)
    with pytest.raises(SystemExit):
        X.parse_args(['--load_path', 'c', '--out', 'o'])


def test_extract_durations_pack_and_suspects():
    import extract_durations as X
    results = [{'durations': [2, 1, 3], 'starts': [0, 2, 3], 'n_frames': 6, 'n_symbols': 3, 'align_logp': -0.5},
               {'durations': None, 'starts': None, 'n_frames': 1, 'n_symbols': 2, 'align_logp': None},
               {'durations': [4], 'starts': [0], 'n_frames': 4, 'n_symbols': 1, 'align_logp': -2.0}]
    d = X.pack(results, [[5, 6, 7], [8, 9], [3]], ['a.wav', 'b.wav', 'c.wav'], 2)
    assert d['offsets'].tolist() == [0, 3, 5, 6] and d['durations'].tolist() == [2, 1, 3, -1, -1, 4]
    assert d['starts'].tolist() == [0, 2, 3, -1, -1, 0] and d['text_ids'].tolist() == [5, 6, 7, 8, 9, 3]
    assert d['n_frames'].tolist() == [6, 1, 4] and d['n_symbols'].tolist() == [3, 2, 1] and int(d['max_step']) == 2
    assert d['align_logp'][0] == -0.5 and np.isnan(d['align_logp'][1]) and d['paths'].tolist() == ['a.wav', 'b.wav', 'c.wav']
    assert d['durations'].dtype == np.int32 and d['offsets'].dtype == np.int64 and d['align_logp'].dtype == np.float32
    assert X.suspects(d['align_logp'].tolist(), -1.0) == [2]            # the row without a path is reported apart
    with pytest.raises(ValueError):
        X.pack(results, [[5, 6], [8, 9], [3]], ['a', 'b', 'c'], 1)


# ---------------------------------------------------------------------- binding and host checks
def test_mas_is_declared_exported_and_checked_on_the_host():
    import t2v_hip
    for name in ('t2v_mas', 't2v_mas_scratch_bytes', 't2v_segment_means'):
        assert name in t2v_hip.EXPORTS
    assert t2v_hip.MAS_MAX_SYMBOLS >= 2048 and t2v_hip.MAS_FLOOR == pytest.approx(mas_ref.FLOOR)
    assert t2v_hip.mas_feasible(3, 3, 1) and not t2v_hip.mas_feasible(2, 3, 1) and t2v_hip.mas_feasible(2, 3, 2)
    assert not t2v_hip.mas_feasible(0, 1, 1) and t2v_hip.mas_feasible(1, 1, 3)
    with pytest.raises(ValueError):
        t2v_hip.mas(torch.zeros(1, 4, 5), [4], [4])                     # a CPU tensor
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.mas(torch.zeros(1, 4, 5), [4], [4])
    with pytest.raises(ValueError):
        t2v_hip.mas(torch.zeros(4, 5), [4], [4])
    with pytest.raises(ValueError):
        t2v_hip.mas(torch.zeros(1, 4, 5, dtype=torch.float64), [4], [4])
