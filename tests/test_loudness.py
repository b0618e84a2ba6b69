"""The loudness meter without a device: the fp64 reference itself (K-weighting coefficients, the full-scale sine of BS.1770,
the filter loop, both gates), the host side of t2v_hip.loudness, prepare_corpus.py's gain arithmetic and arguments, and the
energy fields and summary block of evaluation.py.  The kernels are checked against the same reference in test_loudness_gpu.py."""
import math
import os

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- the reference
def test_coefficients_are_the_standards_table_at_48k():
    import t2v_hip
    want = np.array(R.BS1770_48K)
    assert np.abs(R.coefficients(48000) - want).max() < 1e-12
    got = t2v_hip.kweight_coefficients(48000)
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12
    for sr in (8000, 16000, 22050, 44100):
        assert np.array_equal(t2v_hip.kweight_coefficients(sr), R.coefficients(sr))


def test_full_scale_sine_reads_what_bs1770_states():
    for sr, want in ((48000, -3.01), (16000, -2.970)):
        x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * sr) / sr)
        got = R.measure(x, sr, R.coefficients(sr))['integrated']
        assert abs(got - want) < 0.01, (sr, got)


def test_filter_loop_equals_lfilter():
    lfilter = pytest.importorskip("scipy.signal").lfilter
    x = R.gating_signal(16000)[:20000]
    b0, b1, b2, a1, a2, d1, d2 = R.coefficients_f32(16000)
    z = lfilter([1.0, -2.0, 1.0], [1.0, d1, d2], lfilter([b0, b1, b2], [1.0, a1, a2], x))
    assert np.abs(R.kweight(x, R.coefficients_f32(16000), use_lfilter=False) - z).max() < 1e-12


def test_relative_gate_matters_on_the_burst_signal():
    m = R.measure(R.gating_signal(16000), 16000)
    assert m['integrated'] - m['ungated'] > 1.0                       # a meter without the relative gate reads the ungated value
    assert m['margin_abs'] > 0.5 and m['margin_rel'] > 0.5            # no block near a gate: the count is well defined
    assert 0 < m['gated_blocks'] < m['n_blocks']
    # without the relative gate every block above -70 counts, and the loudness is lower
    bp = m['block_powers']
    above = bp[np.array([R.lufs(p) for p in bp]) > R.ABS_GATE]
    assert R.lufs(float(above.mean())) < m['integrated'] - 0.5


def test_rows_without_a_loudness():
    short = R.measure(0.1 * np.random.RandomState(0).randn(6399), 16000)
    assert short['n_blocks'] == 0 and short['integrated'] == float('-inf') and short['momentary_max'] == float('-inf')
    silent = R.measure(np.zeros(16000), 16000)
    assert silent['n_blocks'] == 7 and silent['integrated'] == float('-inf') and silent['ungated'] == float('-inf')
    faint = R.measure(1e-5 * np.random.RandomState(1).randn(16000), 16000)          # about -100 LUFS: under the absolute gate
    assert faint['integrated'] == float('-inf') and faint['gated_blocks'] == 0 and math.isfinite(faint['ungated'])
    assert R.pooled([0.0, 0.0], [0, 0]) == float('-inf')


def test_pooling_two_rows_from_their_sums():
    rng = np.random.RandomState(2)
    a, b = R.measure(0.2 * rng.randn(16000), 16000), R.measure(0.02 * rng.randn(32000), 16000)
    want = R.lufs((a['gated_sum'] + b['gated_sum']) / (a['gated_blocks'] + b['gated_blocks']))
    assert R.pooled([a['gated_sum'], b['gated_sum']], [a['gated_blocks'], b['gated_blocks']]) == pytest.approx(want, abs=1e-12)
    assert b['integrated'] < want < a['integrated']


# ---------------------------------------------------------------------- t2v_hip, host side
def test_rates_are_checked_and_named():
    import t2v_hip
    for sr in (11025, 7990, 48010, 16001, True):
        with pytest.raises(ValueError, match=str(sr)):
            t2v_hip.kweight_coefficients(sr)
    for sr in (8000, 16000, 22050, 44100, 48000):
        assert t2v_hip.kweight_coefficients(sr).shape == (7,)


def test_table_holds_the_powers_of_the_chunk_transition():
    import t2v_hip
    t = t2v_hip.loudness_table(16000)
    assert t.dtype == np.float64 and t.shape == (8 + 16 * 65,) and not t.flags.writeable
    c = R.coefficients_f32(16000)
    assert np.array_equal(t[:7], c) and np.array_equal(t[:7], t[:7].astype(np.float32))      # fp32 values, held as fp64
    assert np.array_equal(t[8:24].reshape(4, 4), np.eye(4))
    # M = A^64: running the filter on 64 zeros from a state must give M state
    b0, b1, b2, a1, a2, d1, d2 = c
    s = np.array([0.3, -0.2, 0.1, 0.05])
    v = s.copy()
    for _ in range(t2v_hip.LOUDNESS_CHUNK):
        y1 = v[0]
        z = y1 + v[2]
        v = np.array([-a1 * y1 + v[1], -a2 * y1, -2.0 * y1 - d1 * z + v[3], y1 - d2 * z])
    M = t[24:40].reshape(4, 4)
    assert np.abs(M @ s - v).max() < 1e-12
    M64 = t[8 + 16 * 64:].reshape(4, 4)
    assert np.abs(np.linalg.matrix_power(M, 64) - M64).max() < 1e-10
    assert t2v_hip.LOUDNESS_TILE == 256 * t2v_hip.LOUDNESS_CHUNK


def test_energy_db_helper_and_exports():
    import t2v_hip
    assert t2v_hip.energy_db(np.array([1.0, 0.0, 1e-20]))[0] == pytest.approx(-0.691)
    assert t2v_hip.energy_db(np.array([0.0]))[0] == pytest.approx(-0.691 - 120.0)
    import torch
    assert float(t2v_hip.energy_db(torch.tensor([0.1]))[0]) == pytest.approx(-10.691, abs=1e-5)
    assert t2v_hip.Loudness._fields == ('integrated', 'ungated', 'momentary_max', 'gated_sum', 'gated_blocks', 'n_blocks', 'frame_ms')
    lib = t2v_hip.load_library()
    for name in ('t2v_loudness', 't2v_loudness_scratch_bytes', 't2v_scale_rows'):
        assert name in t2v_hip.EXPORTS and hasattr(lib, name)
    assert lib.t2v_loudness_scratch_bytes(2, 6400, 1600) == 4 * 2 * (2 * 100 + 5)
    assert lib.t2v_loudness_scratch_bytes(2, 6400, 1102) > 0 and lib.t2v_loudness_scratch_bytes(2, 6400, 700) == 0
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.loudness(torch.zeros(1, 100), [100])
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.scale_rows(torch.zeros(1, 100), [100], [1.0])


# ---------------------------------------------------------------------- prepare_corpus.py
def test_gain_for():
    import prepare_corpus as PC
    assert PC.gain_for(-23.0, -30.0, 0.1, -1.0) == (7.0, False)
    assert PC.gain_for(-23.0, -20.0, 0.9, -1.0) == (-3.0, False)               # a cut is never limited
    g, limited = PC.gain_for(-23.0, -40.0, 0.5, -1.0)                           # +17 dB would put the peak at +11 dBFS
    assert limited and g == pytest.approx(-1.0 - 20.0 * math.log10(0.5))
    assert 0.5 * 10.0 ** (g / 20.0) == pytest.approx(10.0 ** (-1.0 / 20.0))    # the peak lands on --peak_db exactly
    assert PC.gain_for(-23.0, float('-inf'), 0.5, -1.0) == (0.0, False)
    assert PC.gain_for(-23.0, None, 0.0, -1.0) == (0.0, False)
    assert PC.gain_for(-23.0, -30.0, 0.0, -1.0) == (7.0, False)                 # no peak, nothing to limit


def test_speaker_gains_pool_and_limit():
    import prepare_corpus as PC
    # speaker a: 10 blocks of power 0.01 and 30 of 0.0001; speaker b has one loud row whose peak limits the gain
    rows = [('a', 0.1, 10, 0.3), ('a', 0.003, 30, 0.05), ('b', 0.004, 40, 0.02), ('b', 0.0, 0, 0.9), ('c', 0.0, 0, 0.0)]
    g = PC.speaker_gains(rows, -23.0, -1.0)
    la = -0.691 + 10.0 * math.log10(0.103 / 40)
    assert g['a']['loudness_lufs'] == pytest.approx(la) and g['a']['gain_db'] == pytest.approx(-23.0 - la)
    assert not g['a']['gain_limited'] and g['a']['rows'] == 2
    lb = -0.691 + 10.0 * math.log10(0.004 / 40)
    assert g['b']['loudness_lufs'] == pytest.approx(lb)
    assert g['b']['gain_limited'] and g['b']['gain_db'] == pytest.approx(-1.0 - 20.0 * math.log10(0.9))
    assert g['c'] == dict(loudness_lufs=None, gain_db=0.0, gain_limited=False, rows=1)
    assert PC.pooled_loudness([0.0], [0]) is None
    t = PC.loudness_totals([dict(loudness_lufs=-20.0), dict(loudness_lufs=-30.0), dict(loudness_lufs=None), dict(skipped='x')])
    assert t == dict(rows=2, mean_lufs=-25.0, spread_lu=5.0)


def test_prepare_corpus_lufs_arguments():
    import prepare_corpus as PC
    base = ['--filelist_path', 'f', '--out_dir', 'd', '--out_filelist', 'g']
    a = PC.parse_args(base)
    assert a.lufs is None and a.lufs_scope == 'utterance' and a.peak_db == -1.0
    a = PC.parse_args(base + ['--lufs', '-23', '--lufs_scope', 'speaker', '--peak_db', '-3'])
    assert a.lufs == -23.0 and a.lufs_scope == 'speaker' and a.peak_db == -3.0
    with pytest.raises(SystemExit):
        PC.parse_args(base + ['--lufs', '-23', '--lufs_scope', 'corpus'])
    with pytest.raises(SystemExit):
        PC.parse_args(base + ['--lufs', '-23', '--peak_db', '0.5'])
    with pytest.raises(SystemExit):
        PC.parse_args(base + ['--lufs', 'nan'])


# ---------------------------------------------------------------------- evaluation.py
def test_energy_fields():
    import evaluation as EV
    track = [-20.0, -22.0, -24.0, -90.0]                                        # the last frame does not sound
    ref = [-30.0, -30.0, -34.0]
    f = EV.energy_fields(-21.0, track, -31.5, ref)
    assert set(f) == set(EV.ENERGY_KEYS)
    assert f['loudness_lufs'] == -21.0 and f['loudness_ref_lufs'] == -31.5 and f['loudness_shift_lu'] == pytest.approx(10.5)
    assert f['energy_spread_db'] == pytest.approx(float(np.std([-20.0, -22.0, -24.0])))
    assert f['energy_ref_spread_db'] == pytest.approx(float(np.std(ref)))
    assert f['energy_spread_db'] == pytest.approx(R.spread_db(track))
    none = EV.energy_fields(None, None, float('-inf'), ref)                      # no waveform; a recording under the gates
    assert none['loudness_lufs'] is None and none['loudness_ref_lufs'] is None and none['loudness_shift_lu'] is None
    assert none['energy_spread_db'] is None and none['energy_ref_spread_db'] is not None
    assert EV.energy_fields(float('-inf'), track, -30.0, ref)['loudness_shift_lu'] is None
    assert EV.ENERGY_FLOOR_DB == 40.0


def test_energy_path_fields_equal_the_reference():
    import evaluation as EV
    rng = np.random.RandomState(3)
    x, y = -30.0 + 8.0 * rng.randn(20), -28.0 + 8.0 * rng.randn(17)
    x[4], y[9] = -100.0, -110.0
    path = np.array([(min(p, 19), min(p * 17 // 20, 16)) for p in range(20)])
    sx, sy = R.sounding(x), R.sounding(y)
    pairs = [(x[i], y[j]) for i, j in path if sx[i] and sy[j]]
    assert len(pairs) < len(path)
    got = EV.energy_path_fields(pairs)
    rmse, corr = R.path_energy(x, y, path)
    assert got['energy_rmse_db'] == pytest.approx(rmse) and got['energy_corr'] == pytest.approx(corr)
    assert EV.energy_path_fields([]) == dict(energy_rmse_db=None, energy_corr=None)
    assert EV.energy_path_fields([(1.0, 2.0)]) == dict(energy_rmse_db=1.0, energy_corr=None)
    assert EV.energy_path_fields([(1.0, 2.0), (1.0, 3.0)])['energy_corr'] is None


def _record(emotion, lufs, ref, spread=4.0, ref_spread=8.0, hit_max=False, **more):
    r = {'dtw': 1.0, 'n_frames': 50, 'n_ref_frames': 60, 'hit_max': hit_max, 'emotion': emotion,
         'loudness_lufs': lufs, 'loudness_ref_lufs': ref,
         'loudness_shift_lu': lufs - ref if lufs is not None and ref is not None else None,
         'energy_spread_db': spread, 'energy_ref_spread_db': ref_spread}
    r.update(more)
    return r


def test_summarize_energy_block():
    import evaluation as EV
    recs = [_record(0, -25.0, -24.0), _record(0, -27.0, -26.0), _record(2, -20.0, -16.0), _record(1, -26.5, -31.0),
            _record(1, None, -30.0, spread=None), _record(2, -5.0, -16.0, hit_max=True)]
    s = EV.summarize(recs)
    e = s['energy']
    assert e['overall']['n_energy'] == 4                                        # the None row and the hit_max row are out
    assert e['overall']['loudness_shift_lu_mean'] == pytest.approx((-1.0 - 1.0 - 4.0 + 4.5) / 4)
    assert e['overall']['loudness_shift_lu_abs_mean'] == pytest.approx((1.0 + 1.0 + 4.0 + 4.5) / 4)
    assert e['overall']['energy_spread_ratio_mean'] == pytest.approx(0.5)
    assert 'energy_rmse_db_mean' not in e['overall']
    by = e['by_emotion']
    assert set(by) == set(EV.EMOTIONS)
    assert by['neu']['loudness_vs_neu_lu'] == 0.0 and by['neu']['loudness_ref_vs_neu_lu'] == 0.0
    assert by['ang']['loudness_vs_neu_lu'] == pytest.approx(6.0) and by['ang']['loudness_ref_vs_neu_lu'] == pytest.approx(9.0)
    assert by['sad']['loudness_vs_neu_lu'] == pytest.approx(-0.5) and by['sad']['loudness_ref_vs_neu_lu'] == pytest.approx(-5.5)
    assert by['hap']['n_energy'] == 0 and by['hap']['loudness_vs_neu_lu'] is None
    assert by['sad']['n_energy'] == 1
    # the other blocks do not move
    assert 'n_energy' not in s['overall'] and 'style' not in s


def test_summarize_energy_block_with_path_keys():
    import evaluation as EV
    recs = [_record(0, -25.0, -24.0, energy_rmse_db=3.0, energy_corr=0.5), _record(0, -25.0, -24.0, energy_rmse_db=5.0, energy_corr=None),
            _record(1, -25.0, -24.0, hit_max=True, energy_rmse_db=50.0, energy_corr=-1.0)]
    e = EV.summarize(recs)['energy']['overall']
    assert e['energy_rmse_db_mean'] == pytest.approx(4.0) and e['energy_corr_mean'] == pytest.approx(0.5)


def test_summarize_without_the_keys_is_unchanged():
    import evaluation as EV
    plain = [{'dtw': 1.0 + i, 'n_frames': 50, 'n_ref_frames': 60, 'hit_max': False, 'emotion': i % 4} for i in range(6)]
    s = EV.summarize(plain)
    assert set(s) == {'overall', 'by_emotion'}
    assert set(s['overall']) == {'n_rows', 'n_hit_max', 'hit_max_share', 'n_scored', 'dtw_mean', 'dtw_median', 'length_ratio_mean'}
    with_energy = EV.summarize([dict(r, **EV.energy_fields(-20.0, [-20.0, -21.0], -22.0, [-22.0, -25.0])) for r in plain])
    assert with_energy['overall'] == s['overall'] and with_energy['by_emotion'] == s['by_emotion']
