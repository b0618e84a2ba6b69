"""Prosody scoring, host side: the fp64 YIN reference that the GPU tests compare the kernel with (tests/yin_ref.py, checked
here on steady tones, silence and noise), evaluation.summarize with and without prosody records, evaluate.py --prosody's
argument parsing and the library's exports."""
import math

import numpy as np
import pytest

import yin_ref

TONES = (200.0, 233.3, 60.0, 499.0)         # period 80 exactly, a fractional period, and the two ends of the lag range
# The largest relative error of the reference on TONES, measured here (frames at least 3 from either end): 1.25e-3, at
# 60 Hz, where tau* = tau_max = 267 has no right-hand neighbour and f0 is 16000 / 267; 5.3e-4 at 499 Hz, 9.4e-5 at 200 Hz,
# 4.8e-5 at 233.3 Hz.  The assertion is twice that maximum.
TONE_MEASURED_MAX_REL_ERR = 1.25e-3
TONE_BOUND = 2 * TONE_MEASURED_MAX_REL_ERR


@pytest.mark.parametrize("freq", TONES)
def test_reference_recovers_steady_tones(freq):
    """Five decaying harmonics at a steady frequency: every frame at least 3 away from either end is voiced and within
    TONE_BOUND of the frequency.  Measured maximum of the relative error over the four tones: 1.25e-3 (60 Hz: the period 266.7
    is cut to tau_max = 267, which has no neighbour to interpolate with); the bound asserted is twice that."""
    r = yin_ref.yin(yin_ref.harmonic_tone(freq, 12000))
    assert len(r['f0']) == 12000 // 256 + 1
    inner = r['f0'][3:-3]
    err = np.abs(inner / freq - 1.0)
    print("%.1f Hz: max rel err %.3e, max aperiodicity %.3g, lags %s" % (freq, err.max(), r['aperiodicity'][3:-3].max(),
                                                                           sorted(set(r['tau'][3:-3].tolist()))))
    assert (inner > 0).all()
    assert err.max() <= TONE_BOUND
    assert (r['aperiodicity'][3:-3] < 0.1).all()
    tau_min, tau_max = yin_ref.lags()
    assert (tau_min, tau_max) == (32, 267)
    assert ((r['tau'][3:-3] >= tau_min) & (r['tau'][3:-3] <= tau_max)).all()


def test_reference_silence_and_noise_are_unvoiced():
    r = yin_ref.yin(np.zeros(6000))
    assert (r['f0'] == 0).all() and (r['aperiodicity'] == 1).all() and (r['tau'] == 0).all()
    r = yin_ref.yin(0.1 * np.random.RandomState(0).randn(6000))
    assert (r['f0'] == 0).all() and (r['aperiodicity'] == 1).all()
    assert np.isfinite(r['margin']).all() and (r['margin'] > 0).all()


def test_reference_frame_grid_and_out_of_signal_samples():
    """n // 256 + 1 frames; a tone embedded in zeros gives the frames of the tone cut at its length: what lies outside [0, n)
    counts as 0"""
    for n in (1, 255, 256, 257, 1023, 1024):
        assert len(yin_ref.yin(np.ones(n))['f0']) == n // 256 + 1
    x = yin_ref.harmonic_tone(200.0, 4096)
    whole = yin_ref.yin(x)
    padded = yin_ref.yin(np.concatenate([x, np.zeros(1024)]))
    assert np.array_equal(whole['f0'], padded['f0'][:len(whole['f0'])])
    assert (padded['f0'][len(whole['f0']) + 2:] == 0).all()


def test_reference_non_default_range():
    assert yin_ref.lags(80.0, 400.0) == (40, 200)
    r = yin_ref.yin(yin_ref.harmonic_tone(150.0, 8000), 80.0, 400.0, 0.15)
    assert np.abs(r['f0'][3:-3] / 150.0 - 1.0).max() <= TONE_BOUND


# ---------------------------------------------------------------------- evaluation.summarize
def _rec(dtw, n, n_ref, hit, emo, **prosody):
    return dict({'dtw': dtw, 'n_frames': n, 'n_ref_frames': n_ref, 'hit_max': hit, 'emotion': emo}, **prosody)


def _pro(med, rmed, spread, rspread, share, rshare):
    return {'f0_median_hz': med, 'f0_ref_median_hz': rmed, 'f0_spread_st': spread, 'f0_ref_spread_st': rspread,
            'voiced_share': share, 'voiced_ref_share': rshare,
            'f0_shift_st': None if med is None or rmed is None else 12.0 * math.log2(med / rmed)}


PLAIN_KEYS = {'n_rows', 'n_hit_max', 'hit_max_share', 'n_scored', 'dtw_mean', 'dtw_median', 'length_ratio_mean'}
PROSODY_STATS = {'n_prosody', 'f0_shift_st_mean', 'f0_shift_st_abs_mean', 'f0_spread_ratio_mean', 'voiced_share_mean',
                 'voiced_ref_share_mean'}


def test_summarize_without_prosody_records_is_unchanged():
    from evaluation import summarize
    recs = [_rec(1.0, 100, 100, False, 0), _rec(3.0, 90, 100, False, 0), _rec(9.0, 600, 100, True, 3)]
    s = summarize(recs)
    assert set(s['overall']) == PLAIN_KEYS
    assert s['overall'] == {'n_rows': 3, 'n_hit_max': 1, 'hit_max_share': 1 / 3, 'n_scored': 2, 'dtw_mean': 2.0,
                            'dtw_median': 2.0, 'length_ratio_mean': (1.0 + 0.9 + 6.0) / 3}
    assert s['by_emotion']['ang'] == {'n_rows': 0, 'n_hit_max': 0, 'hit_max_share': None, 'n_scored': 0, 'dtw_mean': None,
                                      'dtw_median': None, 'length_ratio_mean': None}


def test_summarize_with_prosody_records():
    from evaluation import summarize
    recs = [_rec(1.0, 100, 100, False, 0, **_pro(220.0, 110.0, 1.0, 2.0, 0.5, 0.6)),         # + 12 st, ratio 0.5
            _rec(2.0, 100, 100, False, 0, **_pro(100.0, 200.0, 3.0, 2.0, 0.7, 0.8)),         # - 12 st, ratio 1.5
            _rec(3.0, 100, 100, False, 1, **_pro(None, 150.0, None, 1.0, 0.1, 0.9)),         # too few voiced frames: counted out
            _rec(4.0, 600, 100, True, 1, **_pro(300.0, 150.0, 1.0, 1.0, 0.9, 0.9)),          # never stopped: counted out
            _rec(5.0, 100, 100, False, 1, **_pro(150.0 * 2 ** 0.25, 150.0, 0.5, 1.0, 0.3, 0.4))]     # + 3 st, ratio 0.5
    s = summarize(recs)
    o = s['overall']
    assert set(o) == PLAIN_KEYS | PROSODY_STATS
    assert o['n_rows'] == 5 and o['n_hit_max'] == 1 and o['n_scored'] == 4 and o['dtw_mean'] == pytest.approx(11.0 / 4)
    assert o['n_prosody'] == 3
    assert o['f0_shift_st_mean'] == pytest.approx((12.0 - 12.0 + 3.0) / 3)
    assert o['f0_shift_st_abs_mean'] == pytest.approx((12.0 + 12.0 + 3.0) / 3)
    assert o['f0_spread_ratio_mean'] == pytest.approx((0.5 + 1.5 + 0.5) / 3)
    assert o['voiced_share_mean'] == pytest.approx((0.5 + 0.7 + 0.1 + 0.3) / 4)               # every stopped row
    assert o['voiced_ref_share_mean'] == pytest.approx((0.6 + 0.8 + 0.9 + 0.4) / 4)
    sad = s['by_emotion']['sad']
    assert sad['n_rows'] == 3 and sad['n_hit_max'] == 1 and sad['n_prosody'] == 1
    assert sad['f0_shift_st_mean'] == pytest.approx(3.0) and sad['f0_spread_ratio_mean'] == pytest.approx(0.5)
    ang = s['by_emotion']['ang']
    assert ang['n_prosody'] == 0 and all(ang[k] is None for k in PROSODY_STATS - {'n_prosody'})


def test_pitch_stats_and_prosody_fields():
    from evaluation import MIN_VOICED_FRAMES, PROSODY_KEYS, pitch_stats, prosody_fields
    assert MIN_VOICED_FRAMES == 5
    track = [0.0, 100.0, 200.0, 0.0, 400.0, 200.0, 200.0, 0.0]
    med, spread, share = pitch_stats(track)
    st = 12 * np.log2(np.array([100.0, 200.0, 400.0, 200.0, 200.0]) / 200.0)
    assert med == 200.0 and spread == pytest.approx(np.std(st)) and share == pytest.approx(5 / 8)
    assert pitch_stats(track[:5]) == (None, None, 3 / 5)                        # 3 voiced frames: no F0 values
    assert pitch_stats([]) == (None, None, None)
    f = prosody_fields([v * 2 for v in track], track)
    assert set(f) == set(PROSODY_KEYS)
    assert f['f0_shift_st'] == pytest.approx(12.0) and f['f0_spread_st'] == pytest.approx(f['f0_ref_spread_st'])
    f = prosody_fields(None, track)                                             # a row without a waveform
    assert f['f0_median_hz'] is None and f['voiced_share'] is None and f['f0_shift_st'] is None and f['f0_ref_median_hz'] == 200.0
    f = prosody_fields(track[:5], track)
    assert f['f0_shift_st'] is None and f['voiced_share'] == pytest.approx(0.6)


# ---------------------------------------------------------------------- command line and exports
def test_evaluate_cli_parses_prosody():
    import evaluate
    base = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']
    assert evaluate.parse_args(base).prosody is False
    assert evaluate.parse_args(base + ['--prosody']).prosody is True
    text = evaluate.build_arg_parser().format_help()
    assert '--prosody' in text and 'f0_shift_st' in text
    assert 'f0_spread_ratio_mean' in evaluate.__doc__ and 'n_prosody' in evaluate.__doc__


def test_f0_exports_and_host_checks():
    import torch
    import t2v_hip
    assert 't2v_f0_yin' in t2v_hip.EXPORTS
    assert hasattr(t2v_hip.load_library(), 't2v_f0_yin')
    assert t2v_hip.F0_MAX_LAG == 400
    assert t2v_hip.f0_lags() == (32, 267) == yin_ref.lags()
    assert t2v_hip.f0_lags(80, 400) == (40, 200) and t2v_hip.f0_lags(40, 1000) == (16, 400)
    for bad in ((39.9, 500), (60, 1000.1), (500, 500), (600, 500)):
        with pytest.raises(ValueError):
            t2v_hip.f0_lags(*bad)
    with pytest.raises(t2v_hip.T2VHipError):                                    # no CPU path
        t2v_hip.f0(torch.zeros(1, 1000), [1000])
