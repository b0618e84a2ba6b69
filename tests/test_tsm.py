"""Tempo and pitch control without a GPU: the rate arithmetic of t2v_hip, the fp64 restatement of the phase vocoder
(tsm_ref.py) on a tone, the new command-line flags and prepare_corpus's naming scheme."""
import os
import re

import numpy as np
import pytest

import tsm_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tone(hz, seconds, sr=16000, amp=0.5):
    return amp * np.sin(2.0 * np.pi * hz * np.arange(int(round(seconds * sr))) / sr)


def test_stretch_ratio_values_and_errors():
    import t2v_hip
    assert t2v_hip.stretch_ratio(1) == (1, 1) and t2v_hip.stretch_ratio(1.0) == (1, 1)
    assert t2v_hip.stretch_ratio(0.8) == (4, 5) and t2v_hip.stretch_ratio(1.25) == (5, 4)
    assert t2v_hip.stretch_ratio(0.5) == (1, 2) and t2v_hip.stretch_ratio(2) == (2, 1)
    assert t2v_hip.stretch_ratio(1.37) == (137, 100)
    assert t2v_hip.stretch_ratio(0.25) == (1, 4) and t2v_hip.stretch_ratio(4.0) == (4, 1)
    for rate in (0.2501, 0.333333, 0.9, 1.001, 3.999, 2.0 ** 0.5, np.float32(1.1)):
        num, den = t2v_hip.stretch_ratio(rate)
        assert 1 <= num <= 1023 and 1 <= den <= 1023
        # limit_denominator(N) is within 1 / (den N) of its argument; above 1 it may be the reciprocal that is limited, and
        # |1 / x - den / num| <= 1 / (num N) gives |x - num / den| <= x / (den N)
        assert abs(num / den - float(rate)) <= max(1.0, float(rate)) / 1023
    for bad in (0.2499, 4.001, 0.0, -1.0, float('nan'), float('inf'), None, 'fast', True):
        with pytest.raises(ValueError):
            t2v_hip.stretch_ratio(bad)


def test_pitch_ratio_values_and_errors():
    import t2v_hip
    assert t2v_hip.pitch_ratio(0) == (1, 1) and t2v_hip.pitch_ratio(12) == (2, 1) and t2v_hip.pitch_ratio(-12) == (1, 2)
    for st in (-11.5, -2, -1, 0.5, 1, 2, 7):
        p, q = t2v_hip.pitch_ratio(st)
        assert 1 <= p <= 1023 and 1 <= q <= 1023
        f = 2.0 ** (st / 12.0)
        assert abs(p / q - f) <= max(1.0, f) / 1023                       # as for stretch_ratio
        assert abs(12.0 * np.log2(p / q) - st) < 0.02
    assert t2v_hip.pitch_ratio(2)[0] > t2v_hip.pitch_ratio(2)[1]
    for bad in (12.01, -12.5, float('nan'), None, 'up', False):
        with pytest.raises(ValueError):
            t2v_hip.pitch_ratio(bad)


def test_vocoder_rates_combine_speed_and_pitch():
    import fractions
    import t2v_hip
    assert t2v_hip.vocoder_rates(1.0, 0.0) == ((1, 1), (1, 1))
    assert t2v_hip.vocoder_rates(0.8, 0.0) == ((4, 5), (1, 1))
    (num, den), (p, q) = t2v_hip.vocoder_rates(1.25, 12)
    assert (p, q) == (2, 1) and fractions.Fraction(num, den) == fractions.Fraction(5, 8)
    with pytest.raises(ValueError):
        t2v_hip.vocoder_rates(0.3, 12)                                    # 0.15: outside what the kernel's caller accepts
    with pytest.raises(ValueError):
        t2v_hip.vocoder_rates(5.0, 0)


def test_lengths_of_the_restatement():
    assert P.out_frames(600, 1, 2) == 1200 and P.out_frames(9, 137, 100) == 7 and P.out_frames(2, 2, 1) == 1
    assert P.out_frames(70, 5, 4) == 56 and P.out_frames(70, 4, 5) == 88
    i, a = P.positions(9, 137, 100)
    assert i.tolist() == [0, 1, 2, 4, 5, 6, 8] and np.allclose(a, [0, .37, .74, .11, .48, .85, .22])
    # 8000 samples, 32 frames: 40 frames at 4/5 -> min(39 * 256, 10000)
    assert P.out_samples(8000, 4, 5) == 9984 and P.out_samples(8000, 5, 4) == min(25 * 256, 6400)


def test_peaks_and_nearest_peak_follow_the_definition():
    m = np.zeros(513)
    m[[0, 10, 11, 20, 512]] = [3, 5, 5, 1, 2]
    pk = P.peaks(m)
    assert np.flatnonzero(pk).tolist() == [0, 20, 512]                    # 10 and 11 tie: neither is strictly greater
    near = P.nearest_peak(pk)
    assert near[0] == 0 and near[10] == 0 and near[11] == 20 and near[20] == 20 and near[266] == 20 and near[267] == 512
    assert near[512] == 512
    assert P.nearest_peak(np.zeros(513, dtype=bool)) is None


@pytest.mark.parametrize('num,den', [(4, 5), (5, 4)])
@pytest.mark.parametrize('lock', [False, True])
def test_reference_keeps_a_tone_and_scales_its_length(num, den, lock):
    y = tone(440.0, 0.5)
    out = P.time_stretch(y, num, den, lock)
    assert len(out) == P.out_samples(len(y), num, den)
    assert abs(len(out) - len(y) * den / num) <= 256                      # the duration follows the rate to within a frame
    hz, spacing = P.tone_frequency(out, 16000)
    assert abs(hz - 440.0) < 0.25 * spacing, (hz, spacing)
    mid = out[len(out) // 4:3 * len(out) // 4]
    # still a tone, of the amplitude 0.5 at most: the sum starts from frame 0, whose reflect-padded half is no steady tone, and
    # without locking the main lobe's bins keep that frame's relative phases and partly cancel (0.25 at the rate 4/5)
    assert 0.1 < np.sqrt(2.0 * np.mean(mid ** 2)) < 0.6


def test_reference_at_rate_one_returns_the_phases():
    rng = np.random.RandomState(0)
    y = 0.1 * rng.randn(5000) + tone(300.0, 5000 / 16000.0)
    import vocoder_ref as V
    spec = V.stft(y)
    mag, phase = np.abs(spec), np.angle(spec)
    m, p = P.phase_vocoder_row(mag, phase, 1, 1)
    assert m.shape == mag.shape and np.array_equal(m, mag)
    assert P.phase_distance(p, phase).max() < 1e-9
    m, p = P.phase_vocoder_row(mag, phase, 1, 1, phase_lock=True)         # locking at rate 1: phi_kp + phi_k - phi_kp
    assert P.phase_distance(p, phase).max() < 1e-9


def test_tone_frequency_reads_a_tone():
    for hz in (220.0, 440.0, 493.9):
        got, spacing = P.tone_frequency(tone(hz, 0.5), 16000)
        assert spacing == 4.0 and abs(got - hz) < 0.1 * spacing


def test_new_exports_are_declared_and_bound():
    import t2v_hip
    with open(os.path.join(ROOT, 'include', 't2vae.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    protos = dict(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    lib = t2v_hip.load_library()
    for name in ('t2v_phase_vocoder', 't2v_phase_vocoder_scratch_bytes'):
        assert name in protos and name in t2v_hip.EXPORTS and hasattr(lib, name), name
        assert protos[name].count(',') + 1 == len(getattr(lib, name).argtypes)
    assert t2v_hip.TSM_MAX_RATIO == int(re.search(r'#define T2V_TSM_MAX_RATIO (\d+)', src).group(1))
    # the scratch answer: one 32-bit accumulator per output element with locking, none without, none for refused sizes
    assert lib.t2v_phase_vocoder_scratch_bytes(3, 100, 1) == 3 * 513 * 100 * 4
    assert lib.t2v_phase_vocoder_scratch_bytes(3, 100, 0) == 0 and lib.t2v_phase_vocoder_scratch_bytes(0, 100, 1) == 0
    # argument checks come before any launch (no device is touched): the ratio, then the sizes
    one = 1                                                               # any non-null address: refused before it is read
    assert lib.t2v_phase_vocoder(one, None, one, 1, 4, 4, 1024, 1, 0, one, None, 8, None, None) == -1     # T2V_ERR_DIMS
    assert lib.t2v_phase_vocoder(one, None, one, 1, 4, 4, 0, 1, 0, one, None, 8, None, None) == -1
    assert lib.t2v_phase_vocoder(one, None, one, 1, 4, 4, 1, 2, 0, one, None, 7, None, None) == -2        # out_stride < 8
    assert lib.t2v_phase_vocoder(one, one, one, 1, 4, 4, 1, 2, 0, one, None, 8, None, None) == -2         # phase without phase_out
    assert lib.t2v_phase_vocoder(one, one, one, 1, 4, 4, 1, 2, 1, one, one, 8, None, None) == -2          # locking without scratch
    assert lib.t2v_phase_vocoder(one, None, one, 1, 4, 3, 1, 2, 0, one, None, 8, None, None) == -2        # t_stride < T


def test_synthesis_command_lines_take_speed_and_pitch():
    import evaluate
    import synthesizer
    a = synthesizer.parse_args(['--load_path', 'c', '--text', 'x', '--vocoder', 'griffin_lim', '--speed', '0.8', '--pitch', '-2'])
    assert a.speed == 0.8 and a.pitch == -2.0
    assert synthesizer.tempo_options(a) == {'speed': 0.8, 'pitch': -2.0}
    d = synthesizer.parse_args(['--load_path', 'c', '--text', 'x'])
    assert d.speed == 1.0 and d.pitch == 0.0
    with pytest.raises(SystemExit, match="--vocoder"):
        synthesizer.parse_args(['--load_path', 'c', '--text', 'x', '--speed', '0.8'])
    with pytest.raises(SystemExit, match="0.25"):
        synthesizer.parse_args(['--load_path', 'c', '--text', 'x', '--vocoder', 'griffin_lim', '--speed', '5'])
    e = evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o', '--speed', '1.25', '--pitch', '1'])
    assert e.speed == 1.25 and e.pitch == 1.0
    e = evaluate.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o'])
    assert e.speed == 1.0 and e.pitch == 0.0
    ev = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']
    for flags in (['--aligned', '--prosody', '--speed', '0.8'], ['--aligned', '--energy', '--pitch', '1']):
        with pytest.raises(SystemExit, match="time axis"):                # the path is over mel frames, the waveform is not
            evaluate.parse_args(ev + flags)
    assert evaluate.parse_args(ev + ['--aligned', '--speed', '0.8']).aligned          # mels alone: nothing to refuse
    assert evaluate.parse_args(ev + ['--aligned', '--prosody', '--energy']).aligned


def test_extract_latents_takes_probe():
    import extract_latents
    a = extract_latents.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o.npz', '--probe', 'p.json'])
    assert a.probe == 'p.json'
    assert extract_latents.parse_args(['--load_path', 'c', '--filelist_path', 'f', '--out', 'o.npz']).probe is None


def test_prepare_corpus_perturbation_flags_and_names():
    import prepare_corpus as PC
    base = ['--filelist_path', 'f', '--out_dir', 'd', '--out_filelist', 'g']
    a = PC.parse_args(base)
    assert a.speed_perturb == [] and a.pitch_perturb == []
    a = PC.parse_args(base + ['--speed_perturb', '0.9,1.1', '--pitch_perturb', '-1,1'])
    assert a.speed_perturb == [0.9, 1.1] and a.pitch_perturb == [-1.0, 1.0]
    for bad in (['--speed_perturb', '1.0'], ['--speed_perturb', '0.9,0.9'], ['--speed_perturb', '5'], ['--pitch_perturb', '0'],
                ['--pitch_perturb', '13'], ['--speed_perturb', 'x'], ['--speed_perturb', '0.901,0.902']):
        with pytest.raises(SystemExit):
            PC.parse_args(base + bad)
    assert PC.perturbed_name('a.wav', 'speed', 0.9) == 'a_sp0.90.wav'
    assert PC.perturbed_name('a.wav', 'speed', 1.1) == 'a_sp1.10.wav'
    assert PC.perturbed_name('spk_a.wav', 'pitch', -1.0) == 'spk_a_ps-1.wav'
    assert PC.perturbed_name('a.wav', 'pitch', 1.0) == 'a_ps1.wav'
    assert PC.perturbed_name('a.wav', 'pitch', 1.5) == 'a_ps1.5.wav'
    with pytest.raises(ValueError):
        PC.perturbed_name('a.wav', 'gain', 1.0)


def test_synthesizer_keeps_the_four_knobs():
    from synthesizer import GriffinLimVocoder, Synthesizer
    s = Synthesizer()
    assert (s.speed, s.pitch_st, s.ref_speed, s.ref_pitch) == (1.0, 0.0, 1.0, 0.0) and not s._ref_perturbed
    assert callable(s.pitch)                                             # the F0 tracker keeps its name
    s = Synthesizer(speed=0.8, pitch=2, ref_speed=1.1, ref_pitch=-1)
    assert s._ref_perturbed and s._ref_stretch == (11, 10)
    v = GriffinLimVocoder.named('griffin_lim_fast', s.stft, s.speed, s.pitch_st)
    assert v.momentum == 0.99 and v.shift[0] > v.shift[1] and v.stretch[0] < v.stretch[1]
    with pytest.raises(ValueError):
        Synthesizer(speed=9.0)
    with pytest.raises(ValueError):
        Synthesizer(ref_pitch=40)
    with pytest.raises(ValueError):
        GriffinLimVocoder(s.stft, speed=0.1)
