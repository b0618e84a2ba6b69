"""The spectral envelope without a GPU: the definition on the fp64 restatement (envelope_ref.py), a synthetic vowel under the
plain and the formant-preserving pitch shift and under the formant shift, the new export's declaration, binding and argument
checks, the new command-line flags and prepare_corpus's naming scheme."""
import os
import re

import numpy as np
import pytest

import envelope_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _harmonic_spectrum(f0_bins=14.0, n=3):
    """(513, n) fp32: narrow harmonic peaks every f0_bins bins under a smooth two-formant envelope, on a low floor"""
    k = np.arange(513, dtype=np.float64)
    env = 1.0 / (1.0 + ((k - 45.0) / 12.0) ** 2) + 0.5 / (1.0 + ((k - 160.0) / 20.0) ** 2) + 1e-3
    comb = np.exp(-0.5 * (((k + f0_bins / 2.0) % f0_bins - f0_bins / 2.0) / 1.2) ** 2) + 1e-3
    return np.stack([(1.0 + 0.1 * t) * env * comb for t in range(n)], axis=1).astype(np.float32), f0_bins


def test_a_flat_spectrum_gives_a_flat_envelope():
    mag = np.full((513, 2), 0.25, dtype=np.float32)
    mag[:, 1] = 0.0                                                       # an all-zero frame: flat at the floor, log(1e-10)
    for order, iters in ((1, 0), (32, 8), (256, 3)):
        env = E.log_envelope(mag, order, iters)
        assert np.allclose(env[:, 0], np.log(0.25), rtol=0, atol=1e-12)
        assert np.allclose(env[:, 1], np.log(np.float64(np.float32(1e-10))), rtol=0, atol=1e-11)
    assert E.log_floor(mag).tolist() == [np.float32(1e-7) * np.float32(0.25), np.float32(1e-10)]


def test_zero_iterations_is_the_plain_liftered_cepstrum():
    mag, _ = _harmonic_spectrum()
    L = np.log(np.maximum(mag, E.log_floor(mag)[None, :]).astype(np.float64))
    for order in (1, 24, 256):
        # the definition, by the plain DFT matrix of the even extension: c[n] = (1/1024) sum_j x[j] cos(2 pi n j / 1024)
        full = np.concatenate([L, L[-2:0:-1]], axis=0)
        j = np.arange(1024)
        C = np.cos(2.0 * np.pi * np.outer(j, j) / 1024.0)
        c = C @ full / 1024.0
        keep = (j <= order) | (j >= 1024 - order)
        want = (C @ (c * keep[:, None]))[:513]
        assert np.abs(E.log_envelope(mag, order, 0) - want).max() < 1e-10
    with pytest.raises(ValueError):
        E.log_envelope(mag, 0, 0)
    with pytest.raises(ValueError):
        E.log_envelope(mag, 32, 33)


def test_the_true_envelope_rises_to_the_harmonic_peaks():
    mag, f0 = _harmonic_spectrum()
    L = np.log(mag.astype(np.float64))
    e0, e8 = E.log_envelope(mag, 32, 0), E.log_envelope(mag, 32, 8)
    peaks = np.round(np.arange(1, 30) * f0).astype(int)
    assert np.all(e8[peaks] >= e0[peaks])                                 # at or above the cepstral envelope on the peaks
    assert np.mean(L[peaks] - e8[peaks]) < 0.25 * np.mean(L[peaks] - e0[peaks])      # and most of the way up to them
    assert np.all(np.diff([np.mean(E.log_envelope(mag, 32, i)[peaks]) for i in (0, 1, 2, 4, 8)]) >= 0)


def test_warp_follows_the_integer_positions_and_clamps_at_bin_512():
    mag, _ = _harmonic_spectrum()
    env = E.log_envelope(mag, 32, 2)
    assert np.array_equal(E.warp(mag, env, 7, 7), mag.astype(np.float64))  # p == q: the identity
    i, a = E.positions(5, 4)
    assert i[:5].tolist() == [0, 1, 2, 3, 5] and a[:5].tolist() == [0.0, 0.25, 0.5, 0.75, 0.0]
    assert i[409] == 511 and a[409] == 0.25 and i[410] == 512               # 410 * 5 / 4 = 512.5: past the end
    ramp = np.arange(513, dtype=np.float64)[:, None]                      # an "envelope" that reads back its own position
    ew = E.warp_log_envelope(ramp, 5, 4)[:, 0]
    assert np.allclose(ew[:410], np.arange(410) * 1.25) and np.all(ew[410:] == 512.0)
    assert np.allclose(E.warp_log_envelope(ramp, 1, 2)[:, 0], np.arange(513) / 2.0)
    out = E.warp(mag, env, 5, 4)
    assert np.allclose(out[410:], mag[410:] * np.exp(env[512][None, :] - env[410:]))
    # moving the envelope up by p / q and reading it back down returns it, away from the ends
    back = E.moved_envelope(E.moved_envelope(env[:, 0], 5, 4), 4, 5)
    assert np.abs(back - env[:, 0])[5:400].max() < 0.05


@pytest.fixture(scope='module')
def vowel_figures():
    """per (f0, semitones): the distances and F0 readings of the fp64 reference, computed once"""
    out = {}
    for f0 in (120.0, 220.0):
        y = E.vowel(f0)
        e0 = E.mean_log_envelope(y)
        for st in (-4, 4):
            p, q = E.ratio(st)
            plain, kept, moved = E.pitch_shift(y, st, False), E.pitch_shift(y, st, True), E.formant_shift(y, st)
            em = E.mean_log_envelope(moved)
            out[(f0, st)] = dict(d_plain=E.envelope_distance(y, plain), d_kept=E.envelope_distance(y, kept),
                                 d_orig=E.log_spectral_distance(em, e0),
                                 d_moved=E.log_spectral_distance(em, E.moved_envelope(e0, p, q)),
                                 f0=[E.f0_autocorrelation(v) for v in (y, plain, kept, moved)], n=[len(v) for v in (y, plain, kept, moved)])
    return out


def test_the_vowel_keeps_its_envelope_under_the_preserving_shift(vowel_figures):
    """Measured on this reference (resample_ref's filter, rolloff 0.95): plain 7.3 to 8.3 dB, preserving 0.35 to 2.0 dB, the
    ratio at most 0.27 (the downward shifts, whose top bins lie in the resampler's transition band); the formant shift lands
    0.86 to 1.14 dB from the moved envelope and 7.1 to 8.2 dB from the original, the ratio at most 0.14."""
    for (f0, st), v in sorted(vowel_figures.items()):
        print("vowel %g Hz %+d st: plain %.2f dB, preserving %.2f dB (ratio %.3f); formant shift %.2f dB from the original, "
              "%.2f dB from the moved envelope (ratio %.3f); F0 %s" % (f0, st, v['d_plain'], v['d_kept'], v['d_kept'] / v['d_plain'],
                                                                      v['d_orig'], v['d_moved'], v['d_moved'] / v['d_orig'], v['f0']))
        assert v['d_kept'] < v['d_plain'] / 3.0
        assert v['d_moved'] < v['d_orig'] / 3.0
        f_in, f_plain, f_kept, f_moved = v['f0']
        assert f_kept == f_plain and f_moved == f_in                      # F0 goes where the plain shift puts it, or stays
        p, q = E.ratio(st)
        assert abs(f_plain / f_in - p / q) < 0.02 and abs(12.0 * np.log2(p / q) - st) < 0.02
        n_in, n_plain, n_kept, n_moved = v['n']
        assert n_kept == n_plain and abs(n_plain - n_in) <= 257 and n_moved == (n_in // 256) * 256


def test_the_float32_restatement_is_single_precision_and_close():
    mag, _ = _harmonic_spectrum()
    for order, iters in ((1, 0), (32, 8)):
        e32, e64 = E.log_envelope32(mag, order, iters), E.log_envelope(mag, order, iters)
        assert e32.dtype == np.float32 and e64.dtype == np.float64
        err = np.abs(e32.astype(np.float64) - e64).max()
        assert 0.0 < err < 64 * 2.0 ** -24 * np.abs(e64).max()


def test_new_exports_are_declared_and_bound():
    import t2v_hip
    with open(os.path.join(ROOT, 'include', 't2vae.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    protos = dict(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    lib = t2v_hip.load_library()
    name = 't2v_spectral_envelope'
    assert name in protos and name in t2v_hip.EXPORTS and hasattr(lib, name)
    assert protos[name].count(',') + 1 == len(getattr(lib, name).argtypes) == 13
    assert t2v_hip.ENV_MAX_ORDER == int(re.search(r'#define T2V_ENV_MAX_ORDER (\d+)', src).group(1)) == 256
    assert t2v_hip.ENV_MAX_ITERS == int(re.search(r'#define T2V_ENV_MAX_ITERS (\d+)', src).group(1)) == 32
    # argument checks come before any launch (no device is touched)
    one = 1                                                               # any non-null address: refused before it is read
    DIMS, ARG = -1, -2

    def call(B=1, T=4, t_stride=4, order=32, iters=8, p=1, q=1, env=one, out=None, out_stride=4, mag=one, n=one):
        return lib.t2v_spectral_envelope(mag, n, B, T, t_stride, order, iters, p, q, env, out, out_stride, None)
    for bad in (dict(order=0), dict(order=257), dict(iters=-1), dict(iters=33), dict(p=0), dict(p=1024), dict(q=0), dict(q=1024),
                dict(B=0), dict(T=0), dict(T=(1 << 20) + 1, t_stride=(1 << 20) + 1, out_stride=(1 << 20) + 1)):
        assert call(**bad) == DIMS, bad
    for bad in (dict(env=None, out=None), dict(t_stride=3), dict(out_stride=3), dict(mag=None), dict(n=None)):
        assert call(**bad) == ARG, bad
    for name in ('spectral_envelope', 'warp_envelope', 'formant_shift', 'pitch_shift', 'vocoder_warp'):
        assert callable(getattr(t2v_hip, name))


def test_vocoder_warp_combines_pitch_correction_and_formant_factor():
    import fractions
    import t2v_hip
    assert t2v_hip.vocoder_warp(0.0) == (1, 1) and t2v_hip.vocoder_warp(2.0) == (1, 1)          # not preserving: no correction
    assert t2v_hip.vocoder_warp(12, 0.0, True) == (2, 1) and t2v_hip.vocoder_warp(-12, 0.0, True) == (1, 2)
    assert t2v_hip.vocoder_warp(0, 12) == (1, 2) and t2v_hip.vocoder_warp(5, -12, False) == (2, 1)
    assert t2v_hip.vocoder_warp(3, 3, True) == (1, 1)                     # the formants follow the pitch after all
    p, q = t2v_hip.pitch_ratio(2)
    P, Q = t2v_hip.pitch_ratio(-1)
    a, b = t2v_hip.vocoder_warp(2, -1, True)
    assert 1 <= a <= 1023 and 1 <= b <= 1023 and abs(a / b - float(fractions.Fraction(p * Q, q * P))) < 4.0 / 1023
    # each factor lies in 0.5..2, so the product stays in 0.25..4: the ends are reached and accepted
    assert t2v_hip.vocoder_warp(12, -12, True) == (4, 1) and t2v_hip.vocoder_warp(-12, 12, True) == (1, 4)
    for bad in ((12, -12.5, True), (13, 0, True), (0, None, False), (0, 'up', False)):
        with pytest.raises(ValueError):
            t2v_hip.vocoder_warp(*bad)
    assert t2v_hip.vocoder_warp(13, 0, False) == (1, 1)                   # not preserving: the pitch is vocoder_rates' to check


def test_synthesis_command_lines_take_formant_and_preserve_formants():
    import evaluate
    import synthesizer
    base = ['--load_path', 'c', '--text', 'x']
    a = synthesizer.parse_args(base + ['--vocoder', 'griffin_lim', '--formant', '-2', '--pitch', '3', '--preserve_formants'])
    assert a.formant == -2.0 and a.preserve_formants is True
    assert synthesizer.tempo_options(a) == {'speed': 1.0, 'pitch': 3.0, 'formant': -2.0, 'preserve_formants': True}
    d = synthesizer.parse_args(base)
    assert d.formant == 0.0 and d.preserve_formants is False
    assert synthesizer.tempo_options(d) == {'speed': 1.0, 'pitch': 0.0}      # off: the keys of before
    for flags in (['--formant', '1'], ['--preserve_formants']):
        with pytest.raises(SystemExit, match="--vocoder"):
            synthesizer.parse_args(base + flags)
    with pytest.raises(SystemExit, match="-12"):
        synthesizer.parse_args(base + ['--vocoder', 'griffin_lim', '--formant', '13'])
    a = synthesizer.parse_args(base + ['--vocoder', 'griffin_lim', '--formant=-12', '--pitch', '12', '--preserve_formants'])
    assert a.formant == -12.0                                             # the largest combined warp, 4, is accepted
    ev = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']
    e = evaluate.parse_args(ev + ['--formant', '1.5', '--preserve_formants'])
    assert e.formant == 1.5 and e.preserve_formants is True
    e = evaluate.parse_args(ev)
    assert e.formant == 0.0 and e.preserve_formants is False
    with pytest.raises(SystemExit):
        evaluate.parse_args(ev + ['--formant', '-12.5'])
    assert evaluate.parse_args(ev + ['--aligned', '--prosody', '--formant', '2']).aligned   # the time axis is not touched


def test_extract_latents_takes_the_probe_flags():
    import extract_latents
    base = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o.npz']
    a = extract_latents.parse_args(base + ['--probe', 'p.json', '--probe_formant=-2,2', '--probe_preserve_formants'])
    assert a.probe_formant == [-2.0, 2.0] and a.probe_preserve_formants is True
    d = extract_latents.parse_args(base + ['--probe', 'p.json'])
    assert d.probe_formant == [] and d.probe_preserve_formants is False
    for bad in (['--probe_formant', '2'], ['--probe_preserve_formants'], ['--probe', 'p.json', '--probe_formant', '13'],
                ['--probe', 'p.json', '--probe_formant', 'x']):
        with pytest.raises(SystemExit):
            extract_latents.parse_args(base + bad)


def test_prepare_corpus_formant_flags_and_names():
    import prepare_corpus as PC
    base = ['--filelist_path', 'f', '--out_dir', 'd', '--out_filelist', 'g']
    a = PC.parse_args(base)
    assert a.formant_perturb == [] and a.preserve_formants is False
    a = PC.parse_args(base + ['--formant_perturb', '-1,1', '--pitch_perturb', '2', '--preserve_formants'])
    assert a.formant_perturb == [-1.0, 1.0] and a.pitch_perturb == [2.0] and a.preserve_formants is True
    for bad in (['--formant_perturb', '0'], ['--formant_perturb', '13'], ['--formant_perturb', '1,1'], ['--formant_perturb', 'x'],
                ['--formant_perturb', '1.0000001,1.0000002'], ['--preserve_formants']):
        with pytest.raises(SystemExit):
            PC.parse_args(base + bad)
    assert PC.perturbed_name('a.wav', 'formant', -1.0) == 'a_fs-1.wav'
    assert PC.perturbed_name('a.wav', 'formant', 1.5) == 'a_fs1.5.wav' and PC.perturbed_name('spk_a.wav', 'formant', 2) == 'spk_a_fs2.wav'
    assert PC.perturbed_name('a.wav', 'pitch', -1.0) == 'a_ps-1.wav'         # the pitch tag as it was
    with pytest.raises(ValueError):
        PC.perturbed_name('a.wav', 'gain', 1.0)


def test_synthesizer_and_vocoder_keep_their_defaults_and_refuse_bad_values():
    from synthesizer import GriffinLimVocoder, Synthesizer
    s = Synthesizer()
    assert (s.formant, s.ref_formant, s.preserve_formants) == (0.0, 0.0, False) and not s._ref_perturbed
    assert s._ref_warp == (1, 1)
    v = GriffinLimVocoder(s.stft)
    assert (v.formant, v.preserve_formants, v.warp) == (0.0, False, (1, 1))
    v = GriffinLimVocoder.named('griffin_lim', s.stft)
    assert v.warp == (1, 1) and v.stretch == (1, 1) and v.shift == (1, 1)
    v = GriffinLimVocoder(s.stft, pitch=2)
    assert v.warp == (1, 1)                                               # the plain pitch knob: no warp, as before
    v = GriffinLimVocoder.named('griffin_lim_fast', s.stft, 1.0, 2.0, formant=0.0, preserve_formants=True)
    assert v.momentum == 0.99 and v.warp == v.shift and v.warp[0] > v.warp[1]
    v = GriffinLimVocoder(s.stft, formant=3)
    assert v.warp[0] < v.warp[1] and v.shift == (1, 1)                    # the envelope is read lower: it moves up
    s = Synthesizer(ref_formant=1)
    assert s._ref_perturbed and s._ref_warp[0] > s._ref_warp[1]
    s = Synthesizer(pitch=2, formant=-1, preserve_formants=True)
    assert not s._ref_perturbed and (s.formant, s.preserve_formants) == (-1.0, True)
    for bad in (dict(ref_formant=13), dict(formant=-40), dict(formant=float('nan'))):
        with pytest.raises(ValueError):
            Synthesizer(**bad)
    for bad in (dict(formant=12.5), dict(formant=None)):
        with pytest.raises(ValueError):
            GriffinLimVocoder(s.stft, **bad)
