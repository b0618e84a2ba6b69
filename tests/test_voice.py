"""The voice-quality score without a device: the fp64 reference (voice_ref) against closed forms and the literature's ranges,
what its own arithmetic loses in fp32 (the GPU tests' tolerance), and the host side: voice_counted, voice_fields, summarize,
the command line flag and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import voice_ref as R


def _medians(x):
    r = R.voice_quality(x)
    keep = R.counted(r['level_db'])
    assert keep.sum() > 40
    return {k: float(np.median(r[k][keep])) for k in R.FEATS}, r, keep


# ---------------------------------------------------------------------- the reference
def test_reference_equals_the_line_spectrum_of_a_harmonic_tone():
    """220.5 Hz: no harmonic lies within 70 Hz (four bins and a half) of an edge of the band sums (50 Hz, 1 and 5 kHz), so each
    holds whole harmonics; the 2 kHz edge parts two maxima, and the ninth harmonic just under it is neither"""
    f0 = 220.5
    harmonics = f0 * np.arange(1, int(7000 // f0) + 1)
    assert min(abs(h - edge) for h in harmonics for edge in (50.0, 1000.0, 5000.0)) > 70.0
    alpha, hammarberg = R.line_spectrum(f0)
    assert alpha == pytest.approx(-9.06, abs=0.005) and hammarberg == pytest.approx(20.0, abs=1e-9)
    med, r, keep = _medians(R.tone(f0, 16000, power=1, seed=3))
    print("alpha %.3f (line spectrum %.3f), hammarberg %.3f (%.3f)" % (med['alpha_db'], alpha, med['hammarberg_db'], hammarberg))
    assert abs(med['alpha_db'] - alpha) <= 0.1 and abs(med['hammarberg_db'] - hammarberg) <= 0.1
    assert len(r['alpha_db']) == 16000 // 256 + 1


def test_cepstral_peak_separates_tones_from_noise():
    noise_cpp = []
    for seed in range(4):
        r = R.voice_quality(R.noise(16000, seed=seed))
        noise_cpp += r['cpp_db'][R.counted(r['level_db'])].tolist()
    noise_med, noise_95 = float(np.median(noise_cpp)), float(np.percentile(noise_cpp, 95))
    print("noise: median cpp %.2f dB, 95th percentile %.2f dB" % (noise_med, noise_95))
    assert noise_med < 17.0
    for power, freqs in ((1, (70.0, 110.0, 220.5, 330.0)), (2, (110.0, 220.5, 330.0, 480.0))):
        for f0 in freqs:
            med, r, keep = _medians(R.tone(f0, 16000, power=power, snr_db=30.0, seed=int(f0)))
            period = R.SR / f0
            lags = r['cpp_lag'][keep]
            multiple = np.maximum(np.round(lags / period), 1.0)
            print("1/k^%d tone at %g Hz: median cpp %.2f dB, median lag %g (period %.2f)" % (power, f0, med['cpp_db'], med['cpp_lag'], period))
            assert med['cpp_db'] > 20.0 > 17.0 > noise_med
            assert np.median(np.abs(lags - multiple * period)) <= 1.0      # the period or a rahmonic of it


def test_reference_edge_cases():
    # an all-zero row is silent in every frame; a row's frames are n // 256 + 1
    r = R.voice_quality(np.zeros(700, dtype=np.float32))
    assert len(r['level_db']) == 3 and (r['level_db'] == R.SILENT_DB).all()
    assert all(not r[k].any() for k in R.FEATS[1:]) and not R.counted(r['level_db']).any()
    # a flat spectrum: no tilt, no peak, and the first quefrency of the range
    x = np.zeros(1792, dtype=np.float32)
    x[300] = 0.5
    r = R.voice_quality(x)
    seen = r['level_db'] > R.SILENT_DB
    assert seen.tolist() == [True] * 4 + [False] * 4
    assert np.abs(r['hammarberg_db'][seen]).max() < 1e-9 and np.abs(r['slope_db_khz'][seen]).max() < 1e-9
    assert np.abs(r['cpp_db'][seen]).max() < 1e-9 and (r['cpp_lag'][seen] == 32).all()
    assert r['alpha_db'][seen] == pytest.approx(10.0 * np.log10(256.0 / 60.0))             # the bands' widths in bins
    # a band without energy reads the floor, 90 dB under the largest bin: a 220 Hz sine has nothing in 2 - 5 kHz
    t = np.arange(16000) / R.SR
    r = R.voice_quality((0.5 * np.sin(2 * np.pi * 218.75 * t)).astype(np.float32))           # bin 14 exactly
    mid = slice(8, 50)
    assert np.allclose(r['hammarberg_db'][mid], 90.0, atol=1e-6)
    # the scale of the waveform moves the level alone
    x = R.tone(220.5, 4000, power=2, snr_db=20.0, seed=5)
    a, b = R.voice_quality(x), R.voice_quality((0.125 * x).astype(np.float32))
    for k in R.FEATS[1:]:
        assert np.allclose(a[k], b[k], atol=1e-9), k
    assert np.allclose(a['level_db'] - b['level_db'], 20.0 * np.log10(8.0))


def test_fp32_arithmetic_stays_within_the_recorded_distance():
    """the tolerance of the GPU tests is four times FP32_MAX; the figures are in profiles/voice_parity.txt"""
    worst, exempt, total = R.measure_fp32()
    for k in R.FP32_MAX:
        print("%-14s fp32 - fp64: %.3e (recorded %.3e, GPU tolerance %.3e)" % (k, worst[k], R.FP32_MAX[k], R.GPU_TOL[k]))
    print("%d frames, %.2f %% left out of the lag comparison" % (total, 100.0 * exempt))
    for k in R.FP32_MAX:
        assert 0.5 * R.FP32_MAX[k] <= worst[k] <= R.FP32_MAX[k], (k, worst[k])
        assert R.GPU_TOL[k] == 4.0 * R.FP32_MAX[k]
    assert exempt <= R.LAG_EXEMPT_CAP
    lengths = sorted({len(x) for _, x in R.gpu_rows()})
    W = R.FRAMES_PER_WORKGROUP
    assert lengths == sorted({1, 255, 256, 257, 513, 256 * (W - 1), 256 * W, 256 * W + 1, 16000})


# ---------------------------------------------------------------------- the host side
def test_voice_counted_on_hand_worked_tracks():
    import evaluation as E
    import t2v_hip
    assert E.VOICE_SILENT_DB == t2v_hip.VOICE_SILENT_DB == R.SILENT_DB
    assert E.VOICE_FLOOR_DB == t2v_hip.VOICE_FLOOR_DB == R.COUNT_FLOOR_DB == 40.0
    track = [-200.0, -45.0, -20.0, 10.0, -30.0, -30.1, -200.0]
    want = [False, False, True, True, False, False, False]                 # > 10 - 40: -30 itself is out
    assert E.voice_counted(track) == want
    assert t2v_hip.voice_counted(torch.tensor(track)).tolist() == want
    assert R.counted(track).tolist() == want
    assert E.voice_counted([-200.0, -200.0]) == [False, False] and E.voice_counted([]) == []
    assert not t2v_hip.voice_counted(torch.tensor([-200.0, -200.0])).any()
    # a batch wider than its rows: the padding (+0) neither counts nor sets the maximum
    level = torch.tensor([[-80.0, -60.0, -200.0, 0.0, 0.0], [5.0, -50.0, -30.0, 1.0, 0.0]])
    got = t2v_hip.voice_counted(level, [3, 4])
    assert got.tolist() == [[True, True, False, False, False], [True, False, True, True, False]]
    assert t2v_hip.voice_counted(level, torch.tensor([3, 4]), floor_db=10.0).tolist() == [[False, True, False, False, False],
                                                                                           [True, False, False, True, False]]
    assert t2v_hip.VOICE_FEATS == R.FEATS and t2v_hip.VoiceQuality._fields == R.FEATS


def _tracks(level, alpha, hammarberg, slope, cpp):
    return {'level_db': level, 'alpha_db': alpha, 'hammarberg_db': hammarberg, 'slope_db_khz': slope, 'cpp_db': cpp}


def test_voice_fields_on_hand_worked_tracks():
    import evaluation as E
    assert E.VOICE_KEYS == ('alpha_db', 'alpha_ref_db', 'alpha_shift_db', 'hammarberg_db', 'hammarberg_ref_db', 'slope_db_khz',
                            'slope_ref_db_khz', 'cpp_db', 'cpp_ref_db', 'cpp_shift_db')
    assert E.VOICE_ALIGNED_KEYS == ('alpha_rmse_db', 'alpha_corr')
    # counted: frames 1, 2 and 4 of the synthesis (frame 0 is silent, frame 3 lies 50 dB under the top), all three of the recording
    syn = _tracks([-200.0, 20.0, 30.0, -20.0, 25.0], [0.0, -10.0, -12.0, 99.0, -20.0], [0.0, 20.0, 22.0, 99.0, 30.0],
                  [0.0, -8.0, -6.0, 99.0, -7.0], [0.0, 25.0, 21.0, 99.0, 23.0])
    ref = _tracks([10.0, 12.0, 11.0], [-9.0, -7.0, -8.0], [18.0, 19.0, 30.0], [-5.0, -4.0, -3.0], [26.0, 28.0, 27.0])
    got = E.voice_fields(syn, ref)
    assert got == {'alpha_db': -12.0, 'alpha_ref_db': -8.0, 'alpha_shift_db': -4.0, 'hammarberg_db': 22.0, 'hammarberg_ref_db': 19.0,
                   'slope_db_khz': -7.0, 'slope_ref_db_khz': -4.0, 'cpp_db': 23.0, 'cpp_ref_db': 27.0, 'cpp_shift_db': -4.0}
    assert tuple(got) == E.VOICE_KEYS
    # an even count: the mean of the middle two
    two = _tracks([0.0, 1.0], [-4.0, -6.0], [1.0, 2.0], [3.0, 4.0], [10.0, 20.0])
    assert E.voice_fields(two, two)['alpha_db'] == -5.0 and E.voice_fields(two, two)['alpha_shift_db'] == 0.0
    # no waveform, or no counted frame: None on that side and on the shifts
    none = E.voice_fields(None, ref)
    assert none['alpha_db'] is None and none['cpp_db'] is None and none['alpha_shift_db'] is None and none['cpp_shift_db'] is None
    assert none['alpha_ref_db'] == -8.0 and none['cpp_ref_db'] == 27.0 and tuple(none) == E.VOICE_KEYS
    silent = _tracks([-200.0, -200.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0])
    got = E.voice_fields(syn, silent)
    assert got['alpha_ref_db'] is None and got['slope_ref_db_khz'] is None and got['cpp_shift_db'] is None and got['alpha_db'] == -12.0
    # the path values are energy_path_fields' arithmetic under the voice names
    pairs = [(-10.0, -8.0), (-12.0, -11.0), (-20.0, -15.0)]
    path = E.voice_path_fields(pairs)
    assert path == dict(zip(E.VOICE_ALIGNED_KEYS, E.energy_path_fields(pairs).values()))
    assert path['alpha_rmse_db'] == pytest.approx(np.sqrt((4.0 + 1.0 + 25.0) / 3.0))
    assert path['alpha_corr'] == pytest.approx(np.corrcoef([p[0] for p in pairs], [p[1] for p in pairs])[0, 1])
    assert E.voice_path_fields([]) == {'alpha_rmse_db': None, 'alpha_corr': None}
    assert E.voice_path_fields([(1.0, 2.0)]) == {'alpha_rmse_db': 1.0, 'alpha_corr': None}


def test_summarize_adds_a_voice_block_only_for_voice_records():
    import evaluation as E

    def rec(emotion, hit_max, alpha, alpha_ref, cpp, cpp_ref, **more):
        r = {'dtw': 1.0, 'n_frames': 10, 'n_ref_frames': 10, 'hit_max': hit_max, 'emotion': emotion}
        r.update(dict.fromkeys(E.VOICE_KEYS))
        shift = lambda a, b: None if a is None or b is None else a - b
        r.update(alpha_db=alpha, alpha_ref_db=alpha_ref, alpha_shift_db=shift(alpha, alpha_ref), cpp_db=cpp, cpp_ref_db=cpp_ref,
                 cpp_shift_db=shift(cpp, cpp_ref), hammarberg_db=20.0, hammarberg_ref_db=22.0, slope_db_khz=-5.0, slope_ref_db_khz=-6.0)
        r.update(more)
        return r
    records = [rec(0, False, -12.0, -10.0, 24.0, 26.0), rec(0, False, -14.0, -12.0, 22.0, 28.0), rec(1, False, -20.0, -18.0, 16.0, 20.0),
               rec(2, False, -6.0, -4.0, 25.0, 27.0), rec(2, True, 50.0, 50.0, 50.0, 50.0),       # ran to the end: not in any mean
               rec(2, False, None, -8.0, None, 25.0)]                                            # no waveform
    s = E.summarize(records)
    assert set(s) == {'overall', 'by_emotion', 'voice'} and 'n_voice' not in s['overall']
    v = s['voice']
    assert set(v) == {'overall', 'by_emotion'} and set(v['by_emotion']) == set(E.EMOTIONS)
    o = v['overall']
    assert set(o) == {'n_voice'} | {k + '_mean' for k in E.VOICE_KEYS}
    assert o['n_voice'] == 4 and o['alpha_db_mean'] == pytest.approx(-13.0) and o['alpha_ref_db_mean'] == pytest.approx(-10.4)
    assert o['alpha_shift_db_mean'] == pytest.approx(-2.0) and o['cpp_shift_db_mean'] == pytest.approx(-3.5)
    neu, sad, ang, hap = (v['by_emotion'][k] for k in E.EMOTIONS)
    assert neu['n_voice'] == 2 and neu['alpha_vs_neu_db'] == 0.0 and neu['cpp_ref_vs_neu_db'] == 0.0
    assert sad['alpha_vs_neu_db'] == pytest.approx(-7.0) and sad['alpha_ref_vs_neu_db'] == pytest.approx(-7.0)
    assert sad['cpp_vs_neu_db'] == pytest.approx(-7.0) and sad['cpp_ref_vs_neu_db'] == pytest.approx(-7.0)
    assert ang['n_voice'] == 1 and ang['alpha_vs_neu_db'] == pytest.approx(7.0) and ang['alpha_ref_vs_neu_db'] == pytest.approx(5.0)
    assert ang['cpp_ref_vs_neu_db'] == pytest.approx(-1.0)
    assert hap['n_voice'] == 0 and hap['alpha_db_mean'] is None and hap['alpha_vs_neu_db'] is None
    assert 'alpha_rmse_db_mean' not in o
    with_path = [dict(r, alpha_rmse_db=2.0 + i, alpha_corr=None if i else 0.5) for i, r in enumerate(records)]
    o = E.summarize(with_path)['voice']['overall']
    assert o['alpha_rmse_db_mean'] == pytest.approx(np.mean([2.0, 3.0, 4.0, 5.0, 7.0])) and o['alpha_corr_mean'] == 0.5
    # records without the keys: no block, and the other blocks do not move
    plain = [{k: r[k] for k in ('dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion')} for r in records]
    assert set(E.summarize(plain)) == {'overall', 'by_emotion'}
    assert E.summarize(plain)['overall'] == s['overall'] and E.summarize(plain)['by_emotion'] == s['by_emotion']
    assert 'neu' not in ('sad', 'ang') and E.summarize(records, emotions=('sad', 'x', 'ang'))['voice']['by_emotion']['x']['alpha_vs_neu_db'] is None


def test_the_command_line_has_the_flag_and_cpu_tensors_are_refused():
    import evaluate
    import t2v_hip
    text = evaluate.build_arg_parser().format_help()
    assert '--voice' in text and 'alpha_shift_db' in text
    args = evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o'])
    assert args.voice is False
    assert evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o', '--voice']).voice is True
    with pytest.raises(SystemExit, match="--voice"):
        evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o', '--voice', '--aligned', '--speed', '1.5'])
    with pytest.raises(t2v_hip.T2VHipError, match="CPU tensor"):
        t2v_hip.voice_quality(torch.zeros(1, 1000), [1000])
    assert 't2v_voice_quality' in t2v_hip.EXPORTS and t2v_hip.VOICE_FRAMES == R.FRAMES_PER_WORKGROUP
