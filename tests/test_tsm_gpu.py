"""csrc/tsm.hip on the device against the fp64 definitions of tsm_ref.py: the phase vocoder's core with and without
phase locking (bounds from the number formats, not measured), bit identity across batch, stride and composition, a tone
end to end, and the routes that use it: GriffinLimVocoder(speed=, pitch=), prepare_corpus.main with perturbed copies,
Synthesizer.latent_probe and the report of evaluate.py."""
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as R
import tsm_ref as P

pytestmark = pytest.mark.gpu

ROWS = (2, 9, 70, 600)                          # frames per row: the shortest a row can be, odd sizes, many 64-frame chunks
STRIDE = 640                                    # wider than the longest row
RATES = ((1, 2), (4, 5), (1, 1), (5, 4), (2, 1), (137, 100))
U = 2.0 ** -24


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def tables():
    import stft
    return stft.STFT(1024, 256, 1024).tables(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def spectra(tables):
    """(mag, phase) (4, 513, STRIDE) fp32: stft_polar of noise plus two tones, NaN from each row's count on"""
    import t2v_hip
    n = 256 * (max(ROWS) - 1) + 17
    rng = np.random.RandomState(3)
    t = np.arange(n) / 16000.0
    y = np.stack([0.05 * rng.randn(n) + 0.3 * np.sin(2 * np.pi * (220.0 + 40 * b) * t) + 0.2 * np.sin(2 * np.pi * (1510.0 - 90 * b) * t)
                  for b in range(len(ROWS))]).astype(np.float32)
    m, p = t2v_hip.stft_polar(torch.from_numpy(y).cuda(), None, tables)
    assert m.shape == (len(ROWS), 513, max(ROWS))
    mag = np.full((len(ROWS), 513, STRIDE), np.nan, dtype=np.float32)
    phase = mag.copy()
    for b, k in enumerate(ROWS):
        mag[b, :, :k] = m[b, :, :k].cpu().numpy()
        phase[b, :, :k] = p[b, :, :k].cpu().numpy()
    return mag, phase


@pytest.fixture(scope='module')
def references(spectra):
    """{(num, den, lock): [(mag_out, phase_out) per row, fp64]}, computed once from the kernel's own fp32 inputs"""
    mag, phase = spectra
    return {(num, den, lock): [P.phase_vocoder_row(mag[b, :, :k], phase[b, :, :k], num, den, lock) for b, k in enumerate(ROWS)]
            for num, den in RATES for lock in (False, True)}


@pytest.mark.parametrize('lock', [False, True])
@pytest.mark.parametrize('num,den', RATES)
def test_core_against_the_fp64_reference(spectra, references, num, den, lock):
    """Magnitudes: a = r / den and 1 - a = (den - r) / den are each one rounding of an exact quotient (u = 2^-24 relative),
    (1 - a) m0 one more and the fma one more on the sum: at most 3 u (|m0| + |m1|) to first order.
    Phases, compared modulo 2 pi: 16 pi u (j + 1) + pi u.  Per term of the sum two conversions to turns and two subtractions, at
    most about u turns each were they done in fp32, doubled: 8 u turns = 16 pi u radians per term, (j + 1) terms with the
    starting phase; and pi u for the one rounding of the result, a value in [-pi, pi), to fp32.  The kernel's fixed-point terms
    (two conversions of 2^-33 turns, exact integer subtraction and addition) lie far inside the per-term figure; with locking
    two more conversions are added once, not per term, and the peak sets are identical by construction (the decision compares
    the same fp32 magnitudes on both sides), so the same bound holds."""
    import t2v_hip
    mag, phase = spectra
    m, p, n_out = t2v_hip.phase_vocoder(torch.from_numpy(mag).cuda(), torch.from_numpy(phase).cuda(), list(ROWS), (num, den), lock)
    assert n_out == [P.out_frames(k, num, den) for k in ROWS] == [-((-k * den) // num) for k in ROWS]
    assert tuple(m.shape) == tuple(p.shape) == (len(ROWS), 513, max(n_out))
    m, p = m.cpu().numpy(), p.cpu().numpy()
    for b, k in enumerate(ROWS):
        want_m, want_p = references[(num, den, lock)][b]
        t = n_out[b]
        for tail in (m[b, :, t:], p[b, :, t:]):
            assert np.all(tail == 0) and not np.signbit(tail).any()
        assert np.isfinite(m[b, :, :t]).all() and np.isfinite(p[b, :, :t]).all()          # no NaN from past the row's count
        i, _ = P.positions(k, num, den)
        m0 = np.abs(mag[b, :, :k].astype(np.float64)[:, i])
        m1 = np.where((i + 1 < k)[None, :], np.abs(mag[b, :, :k].astype(np.float64)[:, np.minimum(i + 1, k - 1)]), 0.0)
        err_m = np.abs(m[b, :, :t].astype(np.float64) - want_m)
        bound_m = 3.0 * U * (m0 + m1)
        err_p = P.phase_distance(p[b, :, :t], want_p)
        bound_p = (16.0 * np.pi * U * (np.arange(t) + 1.0) + np.pi * U)[None, :]
        print("rate %d/%d lock %d row of %d -> %d frames: worst magnitude error / bound %.3f, worst phase error %.3g rad, / bound %.3g"
              % (num, den, lock, k, t, np.max(err_m / np.maximum(bound_m, 1e-300)), err_p.max(), np.max(err_p / bound_p)))
        assert np.all(err_m <= bound_m), (b, 'magnitude')
        assert np.all(err_p <= bound_p), (b, 'phase')
        assert np.all(np.abs(p[b, :, :t]) <= np.float32(np.pi))


def test_magnitude_only_form_gives_the_same_magnitudes(spectra):
    import t2v_hip
    mag, phase = spectra
    for rate in ((4, 5), (137, 100)):
        m, p, n = t2v_hip.phase_vocoder(torch.from_numpy(mag).cuda(), torch.from_numpy(phase).cuda(), list(ROWS), rate, False)
        m2, n2 = t2v_hip.stretch_magnitude(torch.from_numpy(mag).cuda(), list(ROWS), rate)
        assert n == n2 and _bits(m) == _bits(m2)


@pytest.mark.parametrize('lock', [False, True])
def test_a_row_gives_the_same_bytes_alone_in_the_batch_and_at_another_stride(spectra, lock):
    import t2v_hip
    mag, phase = spectra
    for rate in ((1, 2), (137, 100)):
        m, p, n_out = t2v_hip.phase_vocoder(torch.from_numpy(mag).cuda(), torch.from_numpy(phase).cuda(), list(ROWS), rate, lock)
        for b, k in enumerate(ROWS):
            for stride in (k, k + 7):
                mb = np.full((1, 513, stride), np.nan, dtype=np.float32)
                pb = mb.copy()
                mb[0, :, :k], pb[0, :, :k] = mag[b, :, :k], phase[b, :, :k]
                m1, p1, n1 = t2v_hip.phase_vocoder(torch.from_numpy(mb).cuda(), torch.from_numpy(pb).cuda(), [k], rate, lock)
                assert n1 == [n_out[b]]
                assert _bits(m1[0]) == _bits(m[b, :, :n1[0]]) and _bits(p1[0]) == _bits(p[b, :, :n1[0]]), (rate, b, stride)


def test_arguments_are_checked(spectra):
    import t2v_hip
    mag, phase = (torch.from_numpy(a).cuda() for a in spectra)
    with pytest.raises(ValueError):
        t2v_hip.phase_vocoder(mag, phase, list(ROWS), 5.0)
    with pytest.raises(ValueError):
        t2v_hip.phase_vocoder(mag, phase, list(ROWS), (1024, 1))
    with pytest.raises(ValueError):
        t2v_hip.phase_vocoder(mag, phase, [2, 9, 70, STRIDE + 1], 0.8)
    with pytest.raises(ValueError):
        t2v_hip.phase_vocoder(mag, phase[:, :512], list(ROWS), 0.8)
    with pytest.raises(ValueError, match="512"):
        t2v_hip.time_stretch(torch.zeros(2, 4000, device='cuda'), [4000, 512], 0.8)


# ---------------------------------------------------------------------- time_stretch, pitch_shift
def _waves(seed=7, lengths=(8000, 5000, 1300)):
    rng = np.random.RandomState(seed)
    y = np.zeros((len(lengths), max(lengths) + 50), dtype=np.float32)
    for b, n in enumerate(lengths):
        y[b, :n] = (0.1 * rng.randn(n) + 0.4 * np.sin(2 * np.pi * (200.0 + 60 * b) * np.arange(n) / 16000.0)).astype(np.float32)
    return torch.from_numpy(y).cuda(), list(lengths)


@pytest.mark.parametrize('lock', [False, True])
def test_time_stretch_is_the_three_call_composition(tables, lock):
    import t2v_hip
    y, n = _waves()
    for rate in (0.8, 1.25, 1.37):
        num, den = t2v_hip.stretch_ratio(rate)
        out, n_out = t2v_hip.time_stretch(y, n, rate, lock)
        mag, phase = t2v_hip.stft_polar(y, torch.tensor(n), tables)
        m, p, t_out = t2v_hip.phase_vocoder(mag, phase, [k // 256 + 1 for k in n], rate, lock)
        want = t2v_hip.istft(m, p, t_out, tables)
        assert n_out == [P.out_samples(k, num, den) for k in n] and out.shape == (len(n), max(n_out))
        for b, k in enumerate(n_out):
            assert _bits(out[b, :k]) == _bits(want[b, :k]), (rate, b)
            assert np.all(out[b, k:].cpu().numpy() == 0)


def test_identity_returns_the_input(tables):
    import t2v_hip
    y, n = _waves()
    for out, n_out in (t2v_hip.time_stretch(y, n, 1.0), t2v_hip.time_stretch(y, n, (3, 3)), t2v_hip.pitch_shift(y, n, 0),
                       t2v_hip.pitch_shift(y, n, 0.0, phase_lock=False)):
        assert n_out == n and out.shape == y.shape and _bits(out) == _bits(y)


def _tone(hz=440.0, seconds=0.5):
    return (0.5 * np.sin(2.0 * np.pi * hz * np.arange(int(seconds * 16000)) / 16000.0)).astype(np.float32)


@pytest.mark.parametrize('rate', [0.8, 1.25])
def test_a_tone_keeps_its_frequency_under_time_stretch(rate):
    """The estimator, not the vocoder, limits the reading: the device's deviation from 440 Hz may exceed that of the fp64
    reference on the same fp32 samples by a quarter of the estimator's bin spacing at most."""
    import t2v_hip
    y = _tone()
    num, den = t2v_hip.stretch_ratio(rate)
    out, n_out = t2v_hip.time_stretch(torch.from_numpy(y[None]).cuda(), [len(y)], rate)
    assert n_out == [P.out_samples(len(y), num, den)] and out.shape == (1, n_out[0])
    got, spacing = P.tone_frequency(out[0].cpu().double().numpy(), 16000)
    ref, _ = P.tone_frequency(P.time_stretch(y, num, den, True), 16000)
    print("time_stretch %g: %d -> %d samples, device %.4f Hz (off by %.4f), fp64 reference %.4f Hz (off by %.4f), bin spacing %.3f Hz"
          % (rate, len(y), n_out[0], got, abs(got - 440.0), ref, abs(ref - 440.0), spacing))
    assert abs(got - 440.0) <= abs(ref - 440.0) + 0.25 * spacing


@pytest.mark.parametrize('semitones', [-2, 2])
def test_a_tone_moves_by_the_semitones_under_pitch_shift(semitones):
    import t2v_hip
    y = _tone()
    p, q = t2v_hip.pitch_ratio(semitones)
    target = 440.0 * p / q
    out, n_out = t2v_hip.pitch_shift(torch.from_numpy(y[None]).cuda(), [len(y)], semitones)
    stretched = P.out_samples(len(y), q, p)
    up, down, half, taps = t2v_hip.resample_taps(p, q)
    assert n_out == [t2v_hip.resample_length(stretched, up, down)] and abs(n_out[0] - len(y)) <= 256 + 1       # within a frame
    got, spacing = P.tone_frequency(out[0].cpu().double().numpy(), 16000)
    ref_wave = R.resample(P.time_stretch(y, q, p, True), up, down, half, taps)[0]
    ref, _ = P.tone_frequency(ref_wave, 16000)
    print("pitch_shift %+d st (%d/%d): target %.3f Hz, device %.4f Hz (off by %.4f), fp64 reference %.4f Hz (off by %.4f), "
          "bin spacing %.3f Hz" % (semitones, p, q, target, got, abs(got - target), ref, abs(ref - target), spacing))
    assert abs(got - target) <= abs(ref - target) + 0.25 * spacing


# ---------------------------------------------------------------------- the routes that use it
def test_vocoder_speed_and_pitch():
    from layers import TacotronSTFT
    from synthesizer import GriffinLimVocoder
    stft = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    g = torch.Generator().manual_seed(2)
    mel = (torch.randn(2, 80, 37, generator=g) - 4.0).cuda()
    n = [37, 21]
    np.random.seed(11)
    plain = GriffinLimVocoder(stft, n_iters=3).batch(mel, n)
    np.random.seed(11)
    same = GriffinLimVocoder(stft, n_iters=3, speed=1, pitch=0).batch(mel, n)
    assert all(_bits(a) == _bits(b) for a, b in zip(plain, same))                  # the defaults give today's bytes
    np.random.seed(11)
    one = GriffinLimVocoder(stft, n_iters=3)(mel[:1])
    np.random.seed(11)
    assert _bits(GriffinLimVocoder(stft, n_iters=3, speed=1.0, pitch=0.0)(mel[:1])) == _bits(one)
    slow = GriffinLimVocoder(stft, n_iters=3, speed=0.8).batch(mel, n)
    assert [w.numel() for w in slow] == [(-(-k * 5 // 4) - 1) * 256 for k in n]     # ceil(T / 0.8) frames of audio
    assert all(torch.isfinite(w).all() and float(w.abs().max()) > 0 for w in slow)
    whole = GriffinLimVocoder(stft, n_iters=3, speed=0.8)(mel[:1])
    assert whole.shape == (1, (47 - 1) * 256)
    import t2v_hip
    high = GriffinLimVocoder(stft, n_iters=3, pitch=2)
    p, q = t2v_hip.pitch_ratio(2)
    got = high.batch(mel, n)
    for w, k in zip(got, n):
        frames = t2v_hip.stretch_frames(k, *high.stretch)
        assert w.numel() == t2v_hip.resample_length((frames - 1) * 256, q, p)
        assert abs(w.numel() - (k - 1) * 256) <= 2 * 256                            # the duration stays
    with pytest.raises(ValueError, match="row 1"):
        GriffinLimVocoder(stft, n_iters=1, speed=2.0).batch(mel, [37, 6])


def _wav(path, sr, n, seed):
    from scipy.io.wavfile import write
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    x = 6000 * np.sin(2 * np.pi * (150.0 + 50 * seed) * t) + 800 * rng.randn(n)
    write(str(path), sr, np.clip(x, -32768, 32767).astype(np.int16))
    return str(path)


def test_prepare_corpus_writes_perturbed_copies(tmp_path):
    import prepare_corpus as PC
    import t2v_hip
    from scipy.io.wavfile import read
    src = [_wav(tmp_path / 'a.wav', 16000, 9000, 1), _wav(tmp_path / 'b.wav', 22050, 8000, 2), _wav(tmp_path / 'tiny.wav', 16000, 400, 3)]
    (tmp_path / 'in.txt').write_text(''.join('%s|text %d|spk|%d\n' % (p, i, i) for i, p in enumerate(src)), encoding='utf-8')

    def run(name, extra):
        base = ['--filelist_path', str(tmp_path / 'in.txt'), '--out_dir', str(tmp_path / name), '--out_filelist',
                str(tmp_path / (name + '.txt')), '--no_trim']
        report = PC.main(base + extra)
        return report, [line.split('|') for line in (tmp_path / (name + '.txt')).read_text(encoding='utf-8').splitlines()]

    plain, plain_rows = run('plain', [])
    report, rows = run('aug', ['--speed_perturb', '0.9', '--pitch_perturb', '-1'])
    assert 'perturbations' not in plain and all('perturbed' not in r for r in plain['rows'])
    assert report['perturbations'] == {'speed': [0.9], 'pitch': [-1.0], 'n_written': 4}
    names = [os.path.basename(r[0]) for r in rows]
    assert names == ['a.wav', 'a_sp0.90.wav', 'a_ps-1.wav', 'b.wav', 'b_sp0.90.wav', 'b_ps-1.wav', 'tiny.wav']
    assert [r[1:] for r in rows] == [['text 0', 'spk', '0']] * 3 + [['text 1', 'spk', '1']] * 3 + [['text 2', 'spk', '2']]
    for name in ('a.wav', 'b.wav', 'tiny.wav'):                                     # the plain rows' bytes are unchanged
        assert open(str(tmp_path / 'aug' / name), 'rb').read() == open(str(tmp_path / 'plain' / name), 'rb').read()
    for i, rec in enumerate(report['rows']):
        assert {k: v for k, v in rec.items() if k not in ('perturbed', 'perturb_skipped', 'out_path')} == \
               {k: v for k, v in plain['rows'][i].items() if k != 'out_path'}
    assert report['rows'][2]['perturbed'] == [] and '512' in report['rows'][2]['perturb_skipped']
    for i in (0, 1):
        rec = report['rows'][i]
        assert 'perturb_skipped' not in rec and [(c['kind'], c['value']) for c in rec['perturbed']] == [('speed', 0.9), ('pitch', -1.0)]
        n = rec['samples_out']
        sp, ps = rec['perturbed']
        assert set(sp) == {'kind', 'value', 'out_path', 'samples_out', 'peak', 'clipped_samples'}
        assert sp['samples_out'] == P.out_samples(n, 9, 10) and abs(ps['samples_out'] - n) <= 257
        for c in (sp, ps):
            rate, data = read(c['out_path'])
            assert rate == 16000 and data.dtype == np.int16 and len(data) == c['samples_out'] and np.abs(data).max() > 1000
        # the speed copy is time_stretch of the row's own samples
        y = torch.from_numpy(read(rec['out_path'])[1].astype(np.float32) / 32768.0)[None].cuda()
        if rec['source_rate'] == 16000:
            want, k = t2v_hip.time_stretch(y, [n], 0.9)
            pcm = t2v_hip.crop(want, [[0, k[0]]], pcm16=True)[0]
            assert read(sp['out_path'])[1].tobytes() == pcm[0, :k[0]].cpu().numpy().tobytes()


def test_latent_probe_and_the_command_lines(tmp_path):
    import evaluate
    import extract_latents
    from synthesizer import Synthesizer
    from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=6", gate_bias=-1e3)
    wavs = [_wav(tmp_path / ('r%d.wav' % i), 16000, n, i + 1) for i, n in enumerate((6000, 9000, 7500))]
    syn = Synthesizer(hp).load_checkpoint(ck)
    probe = syn.latent_probe(wavs, pitch=(0, 2), speed=(1.0, 0.85), gain_db=(0, -6), batch_size=2)
    assert set(probe) == {'n_clips', 'scale', 'scale_kind', 'perturbations'}
    assert probe['n_clips'] == 3 and probe['scale_kind'] == 'clip_pairs' and probe['scale'] > 0
    by = {(r['kind'], r['value']): r for r in probe['perturbations']}
    assert list(by) == [('pitch', 0.0), ('pitch', 2.0), ('speed', 1.0), ('speed', 0.85), ('gain_db', 0.0), ('gain_db', -6.0)]
    for r in probe['perturbations']:
        assert set(r) == {'kind', 'value', 'mean', 'median', 'mean_rel', 'median_rel'}
        assert r['mean_rel'] == r['mean'] / probe['scale'] and r['median_rel'] == r['median'] / probe['scale']
        print("%s %+g: mean %.5g, median %.5g, mean / scale %.4g" % (r['kind'], r['value'], r['mean'], r['median'], r['mean_rel']))
    for key in (('pitch', 0.0), ('speed', 1.0), ('gain_db', 0.0)):
        assert by[key]['mean'] == 0.0 and by[key]['median'] == 0.0                  # the identity: exactly 0
    for key in (('pitch', 2.0), ('speed', 0.85), ('gain_db', -6.0)):
        assert by[key]['mean'] > 0.0 and np.isfinite(by[key]['mean'])
    labelled = syn.latent_probe(wavs, emotions=[0, 1, 1], pitch=(), speed=(), gain_db=(6,))
    assert labelled['scale_kind'] == 'emotion_centroids' and labelled['scale'] > 0 and len(labelled['perturbations']) == 1
    # the reference-clip knobs: the mel of the perturbed clip is what load_mels gives
    import t2v_hip
    fast = Synthesizer(hp, ref_speed=1.25, ref_pitch=1)
    y, n = syn.load_wavs(wavs[:2])
    y2, n2 = t2v_hip.pitch_shift(*t2v_hip.time_stretch(y, n, 1.25), 1)
    got, counts = fast.load_wavs(wavs[:2])
    assert counts == n2 and _bits(got) == _bits(y2) and max(n2) < 0.85 * max(n)
    # the command lines
    with open(fl, 'w', encoding='utf-8') as f:
        for i, w in enumerate(wavs):
            f.write('%s|%s|0|%d\n' % (w, OTHER_TEXTS[i % 3], i % 2))
    out = tmp_path / 'lat.npz'
    extract_latents.main(['--load_path', ck, '--filelist_path', fl, '--out', str(out), '--probe', str(tmp_path / 'probe.json'),
                          '--hparams', 'max_decoder_steps=6'])
    cli = json.loads((tmp_path / 'probe.json').read_text(encoding='utf-8'))
    assert cli['n_clips'] == 3 and cli['scale_kind'] == 'emotion_centroids'
    assert [(r['kind'], r['value']) for r in cli['perturbations']] == [('pitch', -2.0), ('pitch', 2.0), ('speed', 0.85),
                                                                      ('speed', 1.15), ('gain_db', -6.0), ('gain_db', 6.0)]
    evaluate.main(['--load_path', ck, '--filelist_path', fl, '--out', str(tmp_path / 'ev.json'), '--limit', '2',
                   '--speed', '0.8', '--pitch', '-1', '--hparams', 'max_decoder_steps=6'])
    rep = json.loads((tmp_path / 'ev.json').read_text(encoding='utf-8'))
    assert rep['speed'] == 0.8 and rep['pitch'] == -1.0 and rep['attention_window'] is None and len(rep['rows']) == 2
    evaluate.main(['--load_path', ck, '--filelist_path', fl, '--out', str(tmp_path / 'ev0.json'), '--limit', '1',
                   '--hparams', 'max_decoder_steps=6'])
    rep = json.loads((tmp_path / 'ev0.json').read_text(encoding='utf-8'))
    assert rep['speed'] == 1.0 and rep['pitch'] == 0.0
    # and the vocoder object that synthesize_batch writes through
    slow = Synthesizer(hp, speed=0.8).load(ck, vocoder='griffin_lim', filelist_path=fl)
    assert slow.vocoder.speed == 0.8 and slow.vocoder.stretch == (4, 5)
    slow.vocoder.n_iters = 2
    paths = [str(tmp_path / 's0.wav'), str(tmp_path / 's1.wav')]
    res = slow.synthesize_batch([OTHER_TEXTS[0], OTHER_TEXTS[2]], paths)
    from scipy.io.wavfile import read
    for (mel, _), path in zip(res, paths):
        assert mel.size(2) == 6 and len(read(path)[1]) == (8 - 1) * 256             # ceil(6 / 0.8) = 8 frames


@pytest.mark.parametrize('speed', [0.8, 1.25])
def test_evaluate_tracks_run_over_the_waveforms_own_frames(tmp_path, monkeypatch, speed):
    """evaluate(prosody=True, energy=True) under a vocoder with speed: the synthesised side's pitch and level fields are those
    of the whole waveform the vocoder wrote, ceil(n / speed) frames, composed here by hand from the same decoder seeds and
    np.random state, not of its first n frames (too few at 0.8) or of n frames with zero padding (too many at 1.25)."""
    import evaluate
    import t2v_hip
    from evaluation import ENERGY_KEYS, PROSODY_KEYS, energy_fields, prosody_fields
    from synthesizer import Synthesizer
    from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
    from test_prosody_gpu import _write_harmonic_wavs
    steps = 12
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=%d" % steps, gate_bias=-1e3)          # every row runs to the last step
    wavs = _write_harmonic_wavs(tmp_path, 3)
    rows = [(w, OTHER_TEXTS[i], '0', i % 2) for i, w in enumerate(wavs)]
    with open(fl, 'w', encoding='utf-8') as f:
        for r in rows:
            f.write('%s|%s|%s|%d\n' % r)
    syn = Synthesizer(hp, speed=speed).load(ck, vocoder='griffin_lim', filelist_path=fl)
    syn.vocoder.n_iters = 2
    dec = syn.model.decoder
    dec._calls = 0
    import evaluation
    used = {'f0': [], 'db': []}                                                     # the lengths of the tracks evaluate hands on

    def spy_prosody(track, ref_track):
        used['f0'].append(len(track))
        return prosody_fields(track, ref_track)

    def spy_energy(loudness, track_db, ref_loudness, ref_track_db):
        used['db'].append(len(track_db))
        return energy_fields(loudness, track_db, ref_loudness, ref_track_db)
    monkeypatch.setattr(evaluation, 'prosody_fields', spy_prosody)
    monkeypatch.setattr(evaluation, 'energy_fields', spy_energy)
    np.random.seed(5)
    recs = syn.evaluate(rows, 2, prosody=True, energy=True)
    monkeypatch.undo()
    frames = P.out_frames(steps, *t2v_hip.stretch_ratio(speed))
    assert frames != steps and frames == -(-steps * 100 // int(round(speed * 100)))
    assert used == {'f0': [frames] * 3, 'db': [frames] * 3}                         # ceil(12 / speed), not the 12 mel frames
    np.random.seed(5)
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        dec._calls = i0
        with torch.no_grad():
            mel, _, _, _, n_frames, _ = syn._synthesize_ragged([r[1] for r in g], True, [r[0] for r in g], (1.0, 0.0, 0.0, 0.0))
        assert n_frames.tolist() == [steps] * len(g)
        out = syn.vocoder.batch(mel, n_frames.tolist())
        y_ref, n_ref = syn.load_wavs([r[0] for r in g])
        f0_ref = t2v_hip.f0(y_ref, n_ref).cpu().tolist()
        loud_ref = t2v_hip.loudness(y_ref, n_ref, 16000)
        db_ref = t2v_hip.energy_db(loud_ref.frame_ms).cpu().tolist()
        for b, w in enumerate(out):
            assert w.numel() == (frames - 1) * 256
            track = t2v_hip.f0(w[None].contiguous(), [w.numel()])[0].cpu().tolist()
            loud = t2v_hip.loudness(w[None].contiguous(), [w.numel()], 16000)
            db = t2v_hip.energy_db(loud.frame_ms)[0].cpu().tolist()
            assert len(track) == len(db) == frames                                  # the track lengths that are used
            k = n_ref[b] // 256 + 1
            want = dict(prosody_fields(track, f0_ref[b][:k]))
            want.update(energy_fields(loud.integrated[0], db, loud_ref.integrated[b], db_ref[b][:k]))
            rec = recs[i0 + b]
            assert set(PROSODY_KEYS) | set(ENERGY_KEYS) <= set(rec) and rec['n_frames'] == steps
            for key, v in want.items():
                assert (rec[key] is None and v is None) or rec[key] == pytest.approx(v, rel=1e-9, abs=1e-12), (i0 + b, key, rec[key], v)
            voiced = sum(1 for v in track if v > 0)
            print("speed %g row %d: %d mel frames, %d waveform frames, %d voiced, voiced_share %s"
                  % (speed, i0 + b, steps, frames, voiced, rec['voiced_share']))
            assert rec['voiced_share'] == pytest.approx(voiced / float(frames))      # over the waveform's frames, not n_frames
    # the frame-by-frame scores walk the mels' path: refused with a waveform on another time axis, fine on mels alone
    with pytest.raises(ValueError, match="time axis"):
        syn.evaluate(rows, 2, prosody=True, aligned=True)
    with pytest.raises(ValueError, match="time axis"):
        syn.evaluate(rows, 2, energy=True, aligned=True)
    dec._calls = 0
    assert all(r['mcd_db'] is not None for r in syn.evaluate(rows, 2, aligned=True))
    if speed == 0.8:                                                                # the command line, vocoder leg included
        out_json = tmp_path / 'ev.json'
        evaluate.main(['--load_path', ck, '--filelist_path', fl, '--out', str(out_json), '--prosody', '--energy', '--speed', '0.8',
                       '--batch_size', '2', '--hparams', 'max_decoder_steps=%d' % steps])
        rep = json.loads(out_json.read_text(encoding='utf-8'))
        assert rep['speed'] == 0.8 and rep['pitch'] == 0.0 and len(rep['rows']) == 3
        assert all(set(PROSODY_KEYS) | set(ENERGY_KEYS) <= set(r) for r in rep['rows'])


def test_prepare_corpus_copies_respect_the_peak_limit_under_a_speaker_gain(tmp_path):
    """--lufs_scope speaker limits the speaker's gain by the peaks of the unperturbed rows; a copy takes that gain unless its
    own peak would pass --peak_db, and then exactly the gain that puts its peak there"""
    import prepare_corpus as PC
    src = [_wav(tmp_path / 'a.wav', 16000, 12000, 1), _wav(tmp_path / 'b.wav', 16000, 9000, 2)]
    (tmp_path / 'in.txt').write_text(''.join('%s|text|spk|%d\n' % (p, i) for i, p in enumerate(src)), encoding='utf-8')
    report = PC.main(['--filelist_path', str(tmp_path / 'in.txt'), '--out_dir', str(tmp_path / 'out'), '--out_filelist',
                      str(tmp_path / 'out.txt'), '--no_trim', '--lufs', '-3', '--lufs_scope', 'speaker', '--peak_db', '-1',
                      '--speed_perturb', '0.9', '--pitch_perturb=-1,1'])
    spk = report['speakers']['spk']
    assert spk['gain_limited'] is True                                             # -3 LUFS is out of reach: the peak limits it
    limit = 10.0 ** (-1.0 / 20.0)
    step = 0.5 / 32768.0                                                            # the 16-bit write-out rounds to nearest
    for rec in report['rows']:
        assert rec['gain_db'] == spk['gain_db'] and rec['peak'] <= limit + step and len(rec['perturbed']) == 3
        for c in rec['perturbed']:
            print("%s %s %+g: gain %.3f dB (speaker %.3f), peak %.5f, limited %s"
                  % (os.path.basename(rec['path']), c['kind'], c['value'], c['gain_db'], spk['gain_db'], c['peak'], c['gain_limited']))
            assert c['gain_db'] <= spk['gain_db'] and c['peak'] <= limit + step and c['clipped_samples'] == 0
            if c['gain_db'] < spk['gain_db']:
                assert c['gain_limited'] is True and abs(c['peak'] - limit) <= step
    # a speaker's gain that a copy's own peak cannot take (30 dB here) is lowered to exactly the limit
    from wavio import read_wav
    front = PC.front_end([read_wav(p) for p in src], 16000, None, 2)
    made = PC.process_batch_perturbed(front, 16000, [('speed', 0.9), ('pitch', 1.0)], -3.0, -1.0, [(30.0, False), (-20.0, False)])
    for pcm, c in made[0]:
        assert c['gain_limited'] is True and c['gain_db'] < 30.0 and abs(c['peak'] - limit) <= step and c['clipped_samples'] == 0
        assert abs(np.abs(pcm.astype(np.float64)).max() / 32768.0 - limit) <= 2 * step
    for pcm, c in made[1]:
        assert c['gain_limited'] is False and c['gain_db'] == -20.0 and c['peak'] < 0.2             # room enough: as it came
