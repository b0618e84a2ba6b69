"""csrc/envelope.hip on the device against the fp64 definitions of envelope_ref.py: the log envelope and the warped magnitudes
(tolerance from the float32 restatement of the same algorithm, not from the kernel), bit identity across batch, stride and
requested outputs, `formant_shift` and `pitch_shift(preserve_formants=True)` as their stated compositions, a synthetic vowel
end to end, and the routes that use them: latent_probe, Synthesizer(ref_formant=), GriffinLimVocoder(formant=,
preserve_formants=) and prepare_corpus --formant_perturb."""
import os

import numpy as np
import pytest
import torch

import envelope_ref as E

pytestmark = pytest.mark.gpu

ROWS = (1, 9, 70)                               # frames per row: one frame, one more than a workgroup's 8, many workgroups
STRIDE = 80
ORDERS = (1, 32, 256)
ITERS = (0, 1, 8)
RATIOS = ((1, 1), (890, 999), (999, 890), (1, 2), (2, 1))
ZERO_FRAME = (2, 5)                             # (row, frame) of the all-zero spectrum
U = 2.0 ** -24


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def tables():
    import stft
    return stft.STFT(1024, 256, 1024).tables(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def spectra(tables):
    """mag (3, 513, STRIDE) fp32: stft_polar of the vowel at three pitches plus noise, one all-zero frame, NaN from each
    row's count on"""
    import t2v_hip
    n = 256 * (max(ROWS) + 2) + 17                                   # three frames more than the longest row
    rng = np.random.RandomState(5)
    y = np.stack([E.vowel(120.0 + 50 * b, 1.2)[:n] + 0.01 * rng.randn(n) for b in range(len(ROWS))]).astype(np.float32)
    m, _ = t2v_hip.stft_polar(torch.from_numpy(y).cuda(), None, tables)
    assert m.shape == (len(ROWS), 513, max(ROWS) + 3)
    mag = np.full((len(ROWS), 513, STRIDE), np.nan, dtype=np.float32)
    for b, k in enumerate(ROWS):
        mag[b, :, :k] = m[b, :, 3:3 + k].cpu().numpy()               # past the first frames, whose reflected half is no vowel
    mag[ZERO_FRAME[0], :, ZERO_FRAME[1]] = 0.0
    return mag


@pytest.fixture(scope='module')
def references(spectra):
    """{(order, iters): ([E fp64 per row], tol_E)}: tol_E is 4 x the worst error of the float32 restatement against the fp64
    one on these inputs and parameters, computed once from the kernel's own fp32 inputs"""
    out = {}
    for order in ORDERS:
        for iters in ITERS:
            e64 = [E.log_envelope(spectra[b, :, :k], order, iters) for b, k in enumerate(ROWS)]
            e32 = [E.log_envelope32(spectra[b, :, :k], order, iters) for b, k in enumerate(ROWS)]
            out[(order, iters)] = (e64, 4.0 * max(float(np.abs(a.astype(np.float64) - r).max()) for a, r in zip(e32, e64)))
    return out


@pytest.mark.parametrize('iters', ITERS)
@pytest.mark.parametrize('order', ORDERS)
def test_core_against_the_fp64_reference(spectra, references, order, iters):
    """Log envelope: within 4 x the worst error of the same algorithm in float32 on scipy.fft (the factor for the other FFT
    factorisation and the device's log).  Warped magnitudes: within |mag_out| (2 tol_E + 4 u): Ew and E each carry tol_E,
    the interpolation weights, the product, the subtraction and exp a rounding each."""
    import t2v_hip
    mag = torch.from_numpy(spectra).cuda()
    want, tol = references[(order, iters)]
    env = t2v_hip.spectral_envelope(mag, list(ROWS), order, iters)
    assert tuple(env.shape) == (len(ROWS), 513, STRIDE)
    env = env.cpu().numpy()
    worst = 0.0
    for b, k in enumerate(ROWS):
        assert np.all(env[b, :, k:] == 0) and not np.signbit(env[b, :, k:]).any()
        assert np.isfinite(env[b, :, :k]).all()                      # no NaN from past the row's count
        worst = max(worst, float(np.abs(env[b, :, :k].astype(np.float64) - want[b]).max()))
    print("order %d iters %d: worst log-envelope error %.3g, tolerance %.3g, ratio %.3f, |E| up to %.3g"
          % (order, iters, worst, tol, worst / tol, max(float(np.abs(w).max()) for w in want)))
    assert worst <= tol
    for p, q in RATIOS:
        out = t2v_hip.warp_envelope(mag, list(ROWS), (p, q), order, iters)
        assert tuple(out.shape) == (len(ROWS), 513, STRIDE)
        out = out.cpu().numpy()
        worst_w = 0.0
        for b, k in enumerate(ROWS):
            assert np.all(out[b, :, k:] == 0) and not np.signbit(out[b, :, k:]).any()
            assert np.isfinite(out[b, :, :k]).all()
            if p == q:
                assert out[b, :, :k].tobytes() == spectra[b, :, :k].tobytes()
                continue
            ref = E.warp(spectra[b, :, :k], want[b], p, q)
            err = np.abs(out[b, :, :k].astype(np.float64) - ref)
            bound = np.abs(out[b, :, :k].astype(np.float64)) * (2.0 * tol + 4.0 * U)
            assert np.all(err <= bound), (p, q, b)
            worst_w = max(worst_w, float(np.max(err / np.maximum(bound, 1e-300))))
        zb, zt = ZERO_FRAME
        assert np.all(out[zb, :, zt] == 0)                             # the all-zero frame stays zero
        print("  warp %d/%d: worst error / bound %.3f" % (p, q, worst_w))


def test_a_row_gives_the_same_bytes_alone_in_the_batch_at_another_stride_and_with_either_output(spectra):
    import t2v_hip
    mag = torch.from_numpy(spectra).cuda()
    for order, iters, ratio in ((32, 8, (890, 999)), (256, 1, (2, 1))):
        env = t2v_hip.spectral_envelope(mag, list(ROWS), order, iters)
        out = t2v_hip.warp_envelope(mag, list(ROWS), ratio, order, iters)
        both = t2v_hip._envelope_launch("both", mag, list(ROWS), order, iters, ratio, True, True)
        assert _bits(both[0]) == _bits(env) and _bits(both[1]) == _bits(out)
        for b, k in enumerate(ROWS):
            for stride in (k, k + 7):
                mb = np.full((1, 513, stride), np.nan, dtype=np.float32)
                mb[0, :, :k] = spectra[b, :, :k]
                e1 = t2v_hip.spectral_envelope(torch.from_numpy(mb).cuda(), [k], order, iters)
                o1 = t2v_hip.warp_envelope(torch.from_numpy(mb).cuda(), [k], ratio, order, iters)
                assert _bits(e1[0, :, :k]) == _bits(env[b, :, :k]) and _bits(o1[0, :, :k]) == _bits(out[b, :, :k]), (b, stride)
        # a frame's bits depend on that frame alone: the 70-frame row from its frame 3 on, in other workgroup positions
        sh = np.ascontiguousarray(spectra[2:3, :, 3:70])
        e2 = t2v_hip.spectral_envelope(torch.from_numpy(sh).cuda(), [67], order, iters)
        assert _bits(e2[0]) == _bits(env[2, :, 3:70])


def test_arguments_are_checked(spectra):
    import t2v_hip
    mag = torch.from_numpy(spectra).cuda()
    for bad in (dict(order=0), dict(order=257), dict(iters=-1), dict(iters=33), dict(order=1.5)):
        with pytest.raises(ValueError):
            t2v_hip.spectral_envelope(mag, list(ROWS), **bad)
    for ratio in ((1024, 1), (0, 1), 1.5, (1, 2, 3)):
        with pytest.raises(ValueError):
            t2v_hip.warp_envelope(mag, list(ROWS), ratio)
    with pytest.raises(ValueError):
        t2v_hip.spectral_envelope(mag, [1, 9, STRIDE + 1])
    with pytest.raises(ValueError):
        t2v_hip.spectral_envelope(mag[:, :512], list(ROWS))
    with pytest.raises(ValueError):
        t2v_hip.formant_shift(torch.zeros(1, 4000, device='cuda'), [4000], 13)


# ---------------------------------------------------------------------- formant_shift, pitch_shift
def _waves(seed=7, lengths=(8000, 5000, 1300)):
    rng = np.random.RandomState(seed)
    y = np.zeros((len(lengths), max(lengths) + 50), dtype=np.float32)
    for b, n in enumerate(lengths):
        y[b, :n] = (0.02 * rng.randn(n) + E.vowel(150.0 + 40 * b, 0.6)[:n]).astype(np.float32)
    return torch.from_numpy(y).cuda(), list(lengths)


def test_the_shifts_are_their_stated_compositions(tables):
    import t2v_hip
    y, n = _waves()
    frames = [k // 256 + 1 for k in n]
    for st in (-3, 2):
        p, q = t2v_hip.pitch_ratio(st)
        mag, phase = t2v_hip.stft_polar(y, torch.tensor(n), tables)
        # formant_shift: stft_polar -> warp_envelope by (q, p) -> istft with the analysis phases
        out, n_out = t2v_hip.formant_shift(y, n, st, order=24, iters=4)
        want = t2v_hip.istft(t2v_hip.warp_envelope(mag, frames, (q, p), 24, 4), phase, frames, tables)
        assert n_out == [(k // 256) * 256 for k in n] and out.shape == (len(n), max(n_out))
        for b, k in enumerate(n_out):
            assert _bits(out[b, :k]) == _bits(want[b, :k]) and np.all(out[b, k:].cpu().numpy() == 0), (st, b)
        for lock in (False, True):
            # preserving: stft_polar -> warp_envelope by (p, q) -> phase_vocoder at (q, p) -> istft -> resample(p, q)
            out, n_out = t2v_hip.pitch_shift(y, n, st, lock, preserve_formants=True)
            m, ph, t_out = t2v_hip.phase_vocoder(t2v_hip.warp_envelope(mag, frames, (p, q)), phase, frames, (q, p), lock)
            mid = t2v_hip.istft(m, ph, t_out, tables)
            n_mid = [min((t - 1) * 256, t2v_hip.stretch_frames(k, q, p)) for t, k in zip(t_out, n)]
            mid = mid[:, :max(n_mid)].contiguous()
            for b, k in enumerate(n_mid):
                mid[b, k:] = 0.0
            want, n_want = t2v_hip.resample(mid, n_mid, p, q)
            assert n_out == n_want and _bits(out) == _bits(want), (st, lock)
            # not preserving: the parent's composition, time_stretch then resample
            out, n_out = t2v_hip.pitch_shift(y, n, st, lock)
            want, n_want = t2v_hip.resample(*t2v_hip.time_stretch(y, n, (q, p), lock), p, q)
            assert n_out == n_want and _bits(out) == _bits(want), (st, lock)
            assert _bits(t2v_hip.pitch_shift(y, n, st, lock, preserve_formants=False, order=8, iters=0)[0]) == _bits(want)


def test_zero_semitones_returns_the_input():
    import t2v_hip
    y, n = _waves()
    for out, n_out in (t2v_hip.formant_shift(y, n, 0), t2v_hip.formant_shift(y, n, 0.0, order=8, iters=1),
                       t2v_hip.pitch_shift(y, n, 0, preserve_formants=True), t2v_hip.pitch_shift(y, n, 0.0)):
        assert n_out == n and out.shape == y.shape and _bits(out) == _bits(y)


VOWEL_MARGIN_DB = 0.0028   # device distance against the fp64 reference's: ten times the worst gap measured, 2.8e-4 dB


@pytest.mark.parametrize('f0', [120.0, 220.0])
def test_the_vowel_keeps_its_formants_end_to_end(f0):
    """The three assertions of test_envelope.py on the device's waveforms, and the device's distances against the fp64
    reference's on the same fp32 samples."""
    import t2v_hip
    y = E.vowel(f0).astype(np.float32)
    yd = torch.from_numpy(y[None]).cuda()
    e0 = E.mean_log_envelope(y)
    for st in (-4, 4):
        p, q = t2v_hip.pitch_ratio(st)
        assert (p, q) == E.ratio(st)
        plain = t2v_hip.pitch_shift(yd, [len(y)], st)[0][0].cpu().double().numpy()
        kept = t2v_hip.pitch_shift(yd, [len(y)], st, preserve_formants=True)[0][0].cpu().double().numpy()
        moved = t2v_hip.formant_shift(yd, [len(y)], st)[0][0].cpu().double().numpy()
        d_plain, d_kept = E.envelope_distance(y, plain), E.envelope_distance(y, kept)
        em = E.mean_log_envelope(moved)
        d_orig, d_moved = E.log_spectral_distance(em, e0), E.log_spectral_distance(em, E.moved_envelope(e0, p, q))
        r_plain, r_kept = E.envelope_distance(y, E.pitch_shift(y, st, False)), E.envelope_distance(y, E.pitch_shift(y, st, True))
        rm = E.mean_log_envelope(E.formant_shift(y, st))
        r_orig, r_moved = E.log_spectral_distance(rm, e0), E.log_spectral_distance(rm, E.moved_envelope(e0, p, q))
        gaps = [abs(d_plain - r_plain), abs(d_kept - r_kept), abs(d_orig - r_orig), abs(d_moved - r_moved)]
        print("vowel %g Hz %+d st: plain %.4f dB (fp64 %.4f), kept %.4f (%.4f), formant shift to original %.4f (%.4f), to the "
              "moved envelope %.4f (%.4f); worst gap %.3g dB" % (f0, st, d_plain, r_plain, d_kept, r_kept, d_orig, r_orig, d_moved,
                                                                 r_moved, max(gaps)))
        assert d_kept < d_plain / 3.0
        assert d_moved < d_orig / 3.0
        assert E.f0_autocorrelation(kept) == E.f0_autocorrelation(plain) and E.f0_autocorrelation(moved) == E.f0_autocorrelation(y)
        assert max(gaps) <= VOWEL_MARGIN_DB


# ---------------------------------------------------------------------- the routes that use it
def _wav(path, sr, n, seed):
    from scipy.io.wavfile import write
    x = 20000 * E.vowel(130.0 + 30 * seed, n / float(sr), sr)[:n] + 300 * np.random.RandomState(seed).randn(n)
    write(str(path), sr, np.clip(x, -32768, 32767).astype(np.int16))
    return str(path)


def test_latent_probe_tells_pitch_from_formants_and_reference_knobs_compose(tmp_path):
    import t2v_hip
    from synthesizer import Synthesizer
    from test_batch_synthesis_gpu import _synth
    hp, ck, _ = _synth(tmp_path, "max_decoder_steps=6", gate_bias=-1e3)
    wavs = [_wav(tmp_path / ('r%d.wav' % i), 16000, n, i + 1) for i, n in enumerate((6000, 9000, 7500))]
    syn = Synthesizer(hp).load_checkpoint(ck)
    probe = syn.latent_probe(wavs, pitch=(0, 2), speed=(), gain_db=(0,), batch_size=2, formant=(0, 2), preserve_formants=True)
    assert set(probe) == {'n_clips', 'scale', 'scale_kind', 'perturbations'} and probe['n_clips'] == 3
    by = {(r['kind'], r['value']): r for r in probe['perturbations']}
    assert list(by) == [('pitch', 0.0), ('pitch', 2.0), ('gain_db', 0.0), ('formant', 0.0), ('formant', 2.0)]   # formant after gain_db
    for r in probe['perturbations']:
        assert set(r) == {'kind', 'value', 'mean', 'median', 'mean_rel', 'median_rel'}
        print("%s %+g: mean %.5g, median %.5g, mean / scale %.4g" % (r['kind'], r['value'], r['mean'], r['median'], r['mean_rel']))
    for key in (('pitch', 0.0), ('gain_db', 0.0), ('formant', 0.0)):
        assert by[key]['mean'] == 0.0 and by[key]['median'] == 0.0                  # the identity: exactly 0
    for key in (('pitch', 2.0), ('formant', 2.0)):
        assert by[key]['mean'] > 0.0 and np.isfinite(by[key]['mean'])
    # the preserving pitch entry is another perturbation than the plain one; the default call is the list of before
    plain = syn.latent_probe(wavs, batch_size=2)
    assert [(r['kind'], r['value']) for r in plain['perturbations']] == [('pitch', -2.0), ('pitch', 2.0), ('speed', 0.85),
                                                                        ('speed', 1.15), ('gain_db', -6.0), ('gain_db', 6.0)]
    assert all(set(r) == {'kind', 'value', 'mean', 'median', 'mean_rel', 'median_rel'} for r in plain['perturbations'])
    assert plain['perturbations'][1]['mean'] != by[('pitch', 2.0)]['mean']
    with pytest.raises(ValueError):
        syn.latent_probe(wavs, formant=(13,))
    # the reference-clip knobs: tempo, then the preserving pitch shift, then the formant shift
    y, n = syn.load_wavs(wavs[:2])
    knobs = Synthesizer(hp, ref_formant=1, preserve_formants=True, ref_pitch=1)
    got, counts = knobs.load_wavs(wavs[:2])
    y2, n2 = t2v_hip.formant_shift(*t2v_hip.pitch_shift(y, n, 1, preserve_formants=True), 1)
    assert counts == n2 and _bits(got) == _bits(y2)
    got, counts = Synthesizer(hp, ref_formant=-2).load_wavs(wavs[:2])
    y3, n3 = t2v_hip.formant_shift(y, n, -2)
    assert counts == n3 == [(k // 256) * 256 for k in n] and _bits(got) == _bits(y3)
    got, counts = Synthesizer(hp, ref_pitch=1).load_wavs(wavs[:2])                    # without the new knobs: the plain shift
    y4, n4 = t2v_hip.pitch_shift(y, n, 1)
    assert counts == n4 and _bits(got) == _bits(y4) and _bits(y4) != _bits(t2v_hip.pitch_shift(y, n, 1, preserve_formants=True)[0])


def test_vocoder_formant_and_preserve_formants():
    from layers import TacotronSTFT
    from synthesizer import GriffinLimVocoder
    stft = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    g = torch.Generator().manual_seed(2)
    mel = (torch.randn(2, 80, 37, generator=g) - 4.0).cuda()
    n = [37, 21]
    np.random.seed(11)
    plain = GriffinLimVocoder(stft, n_iters=3).batch(mel, n)
    np.random.seed(11)
    same = GriffinLimVocoder(stft, n_iters=3, formant=0, preserve_formants=True).batch(mel, n)     # no pitch: nothing to preserve
    assert all(_bits(a) == _bits(b) for a, b in zip(plain, same))                  # the defaults give today's bytes
    np.random.seed(11)
    high = GriffinLimVocoder(stft, n_iters=3, pitch=2).batch(mel, n)
    np.random.seed(11)
    kept = GriffinLimVocoder(stft, n_iters=3, pitch=2, preserve_formants=True).batch(mel, n)
    assert [w.numel() for w in kept] == [w.numel() for w in high]                   # the frame and sample counts of pitch=2 alone
    assert all(torch.isfinite(w).all() and float(w.abs().max()) > 0 for w in kept)
    assert any(_bits(a) != _bits(b) for a, b in zip(kept, high))
    np.random.seed(11)
    moved = GriffinLimVocoder(stft, n_iters=3, formant=-3).batch(mel, n)
    assert [w.numel() for w in moved] == [(k - 1) * 256 for k in n] and all(torch.isfinite(w).all() for w in moved)
    assert any(_bits(a) != _bits(b) for a, b in zip(moved, plain))
    one = GriffinLimVocoder(stft, n_iters=3, formant=-3)(mel[:1])
    assert one.shape == (1, 36 * 256) and torch.isfinite(one).all()


def test_prepare_corpus_writes_formant_copies(tmp_path):
    import prepare_corpus as PC
    import t2v_hip
    from scipy.io.wavfile import read
    src = [_wav(tmp_path / 'a.wav', 16000, 9000, 1), _wav(tmp_path / 'b.wav', 16000, 7000, 2)]
    (tmp_path / 'in.txt').write_text(''.join('%s|text %d|spk|%d\n' % (p, i, i) for i, p in enumerate(src)), encoding='utf-8')

    def run(name, extra):
        base = ['--filelist_path', str(tmp_path / 'in.txt'), '--out_dir', str(tmp_path / name), '--out_filelist',
                str(tmp_path / (name + '.txt')), '--no_trim']
        report = PC.main(base + extra)
        return report, [line.split('|') for line in (tmp_path / (name + '.txt')).read_text(encoding='utf-8').splitlines()]

    old, _ = run('old', ['--pitch_perturb', '-1'])
    assert old['perturbations'] == {'speed': [], 'pitch': [-1.0], 'n_written': 2}   # without the new flags: none of the new keys
    report, rows = run('aug', ['--formant_perturb', '1', '--pitch_perturb', '-1', '--preserve_formants'])
    assert report['perturbations'] == {'speed': [], 'pitch': [-1.0], 'n_written': 4, 'formant': [1.0], 'preserve_formants': True}
    assert [os.path.basename(r[0]) for r in rows] == ['a.wav', 'a_ps-1.wav', 'a_fs1.wav', 'b.wav', 'b_ps-1.wav', 'b_fs1.wav']
    for i, rec in enumerate(report['rows']):
        assert [(c['kind'], c['value']) for c in rec['perturbed']] == [('pitch', -1.0), ('formant', 1.0)]
        n = rec['samples_out']
        ps, fs = rec['perturbed']
        assert set(fs) == {'kind', 'value', 'out_path', 'samples_out', 'peak', 'clipped_samples'}
        assert fs['samples_out'] == (n // 256) * 256 and abs(ps['samples_out'] - n) <= 257
        y = torch.from_numpy(read(rec['out_path'])[1].astype(np.float32) / 32768.0)[None].cuda()
        for c, (want, k) in ((fs, t2v_hip.formant_shift(y, [n], 1.0)), (ps, t2v_hip.pitch_shift(y, [n], -1.0, preserve_formants=True))):
            pcm = t2v_hip.crop(want, [[0, k[0]]], pcm16=True)[0]
            rate, data = read(c['out_path'])
            assert rate == 16000 and data.tobytes() == pcm[0, :k[0]].cpu().numpy().tobytes() and np.abs(data).max() > 1000
        # the plain pitch copy of the run without the flag is another file
        assert open(ps['out_path'], 'rb').read() != open(old['rows'][i]['perturbed'][0]['out_path'], 'rb').read()
