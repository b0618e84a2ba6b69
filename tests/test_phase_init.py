"""The phase start from magnitudes (single-pass spectrogram inversion), CPU side: the integer-turn restatement of
tests/spsi_ref.py against the properties the GPU tests lean on, what it buys on steady tones (spectral convergence on true
magnitudes, voicing on mel-inverted ones: DESIGN 7r), and the Python wrappers' arguments, which need no GPU."""
import numpy as np
import pytest

import spsi_ref as S
import vocoder_ref as R
import yin_ref as Y

# DESIGN 7r, CPU fp64: spectral convergence of the waveform on the true magnitudes of a 2 s five-harmonic tone
TABLE_SC = {91: (0.11, 0.64, 0.21), 125: (0.11, 0.67, 0.22), 220: (0.09, 0.66, 0.23)}      # SPSI at 0, random at 0, random at 16


@pytest.fixture(scope='module')
def basis():
    from layers import slaney_mel_filterbank
    return slaney_mel_filterbank(16000, 1024, 80, 0.0, 8000.0).astype(np.float32)


def _lobe(x, amp=1.0, n=40):
    """n frames of a stationary partial at the (non-integer) bin x: the periodic Hann window's main lobe, fp32"""
    k = np.arange(S.BINS, dtype=np.float64)
    d = k - x
    with np.errstate(all='ignore'):
        w = np.sinc(d) / (1.0 - d * d)                       # |W(d)| of the Hann window, up to a factor
    w = np.where(np.abs(np.abs(d) - 1.0) < 1e-12, 0.5, w)
    return np.repeat((amp * np.abs(w))[:, None], n, axis=1).astype(np.float32)


def test_stationary_partial_advances_by_its_frequency():
    for x in (40.3, 41.0, 100.75, 257.5001):
        mag = _lobe(x)
        pk, p, adv = S.advances(mag)
        k = int(round(x))
        # a parabola through linear magnitudes of a Hann lobe pulls the offset towards the bin, by up to 0.06 bins near +-0.3
        assert pk[k].all() and p[k, 0] * (x - k) >= 0 and abs(p[k, 0] - (x - k)) <= 0.07, (x, p[k, 0])
        acc = S.accumulate(adv)
        step = np.diff(acc[k].astype(np.int64)) % (1 << 32)
        want = (((k & 3) << 30) + int(np.rint(p[k, 0] * 2.0 ** 30))) % (1 << 32)
        assert np.all(step == want), x
        # (k + p) / 4 turns per frame, to the rounding of one advance
        turns = want / 2.0 ** 32
        assert abs((turns - (k + p[k, 0]) / 4.0 + 0.5) % 1.0 - 0.5) <= 2.0 ** -32, x
        assert acc[k, 0] == want and acc[k, -1] == (want * mag.shape[1]) % (1 << 32)
        assert not acc[0].any() and not acc[512].any()


def test_phases_lie_in_the_half_open_interval():
    rs = np.random.RandomState(3)
    mag = np.exp(rs.randn(S.BINS, 70)).astype(np.float32)
    ph = S.spsi_phase(mag)
    assert ph.dtype == np.float32 and ph.shape == mag.shape
    assert ph.min() >= np.float32(-np.pi) and ph.max() < np.float32(np.pi)
    # the ends of the range themselves: -2^31 turns is -pi, 2^31 - 1 rounds to pi in fp32 only through the fp64 product
    assert S.radians(np.array([0x80000000], dtype=np.uint32))[0] == np.float32(-np.pi)
    assert S.radians(np.array([0], dtype=np.uint32))[0] == 0.0


def test_a_row_does_not_depend_on_what_follows_its_length():
    rs = np.random.RandomState(4)
    mag = np.exp(rs.randn(2, S.BINS, 90)).astype(np.float32)
    full = S.spsi_batch(mag, [90, 90])
    cut = mag.copy()
    cut[0, :, 37:] = np.nan
    cut[1, :, 64:] = 1e30
    out = S.spsi_batch(cut, [37, 64])
    assert np.array_equal(out[0, :, :37], full[0, :, :37]) and np.array_equal(out[1, :, :64], full[1, :, :64])
    assert not out[0, :, 37:].any() and not out[1, :, 64:].any() and not np.signbit(out[:, :, 64:]).any()
    assert not np.isnan(out).any()


def _ramp(points):
    """a frame through the (bin, value) control points, linear between them: strictly monotone between two points"""
    ks, vs = zip(*points)
    return np.interp(np.arange(S.BINS), ks, vs).astype(np.float32)


def test_tie_and_plateau_rules():
    # peaks at 64 and 66 alone: bin 65 is as far from both and takes the lower one
    fr = _ramp([(0, 1.0), (64, 3.0), (65, 2.0), (66, 2.5), (512, 0.5)])
    pk = S.peaks(fr[:, None])[:, 0]
    assert np.flatnonzero(pk).tolist() == [64, 66]
    kp = S.nearest_peak(pk)
    assert kp[65] == 64 and kp[64] == 64 and kp[66] == 66 and kp[0] == 64 and kp[512] == 66 and kp[67] == 66
    # a plateau M[k] == M[k + 1] above its neighbours is no peak, and neither are bins 0 and 512
    fr = _ramp([(0, 5.0), (50, 1.0), (100, 3.0), (101, 3.0), (200, 1.0), (300, 2.0), (511, 1.0), (512, 9.0)])
    assert np.flatnonzero(S.peaks(fr[:, None])[:, 0]).tolist() == [300]
    # without a peak the frame is +0: equal magnitudes, zeros
    for fr in (np.ones(S.BINS, np.float32), np.zeros(S.BINS, np.float32)):
        ph = S.spsi_phase(np.repeat(fr[:, None], 3, axis=1))
        assert not ph.any() and not np.signbit(ph).any()
    # one peak: every bin hangs on it, half a turn apart from bin to bin
    fr = _ramp([(0, 1.0), (1, 2.0), (512, 0.5)])
    turns, has, acc = S.spsi_turns(fr[:, None])
    assert has.all() and np.flatnonzero(S.peaks(fr[:, None])[:, 0]).tolist() == [1]
    d = (turns[1:, 0].astype(np.int64) - turns[:-1, 0].astype(np.int64)) % (1 << 32)
    assert np.all(d == 1 << 31)


def test_spectral_convergence_on_true_magnitudes():
    for f, (t_spsi, t_r0, t_r16) in TABLE_SC.items():
        mag = np.abs(R.stft(R.tone(f)))
        sc = R.spectral_convergence(S.start(mag), mag)
        np.random.seed(0)
        angles = S.random_angles(mag.shape)
        r0 = R.spectral_convergence(R.griffin_lim(mag, angles, 0), mag)
        r16 = R.spectral_convergence(R.griffin_lim(mag, angles, 16), mag)
        print("tone %d Hz: SPSI start %.3f, random start %.3f, after 16 plain iterations %.3f (table %.2f, %.2f, %.2f)"
              % (f, sc, r0, r16, t_spsi, t_r0, t_r16))
        assert sc <= 0.25 * r0, (f, sc, r0)
        assert sc <= r16, (f, sc, r16)


def test_low_tones_stay_voiced(basis):
    """DESIGN 7g's chain: m = B S, 100 NNLS steps, the start, one inverse, YIN; against the random start after 60 plain iterations"""
    pinv = np.linalg.pinv(basis.astype(np.float64))
    for f in (70, 100, 125):
        M = R.nnls(basis.astype(np.float64) @ R.frame_magnitudes(R.tone(f)), basis, pinv, 100)
        share = S.voiced_share(Y.yin(S.start(M))['f0'])
        np.random.seed(0)
        rand = S.voiced_share(Y.yin(R.griffin_lim(M, S.random_angles(M.shape), 60))['f0'])
        print("tone %d Hz: voiced share SPSI start %.2f, random start after 60 iterations %.2f" % (f, share, rand))
        assert share >= rand, (f, share, rand)
        if f in (70, 100):
            assert share > rand, (f, share, rand)


def test_wrappers(tmp_path):
    import torch
    import evaluate
    import hparams as HP
    from audio_processing import griffin_lim
    from layers import TacotronSTFT
    from stft import STFT
    from synthesizer import VOCODERS, GriffinLimVocoder, Synthesizer, build_arg_parser
    taco = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    mag = torch.ones(1, 513, 8)
    with pytest.raises(ValueError, match="angles"):
        griffin_lim(mag, STFT(1024, 256, 1024), 2, angles=torch.zeros(1, 513, 8), init='spsi')
    for bad in ('pghi', None, 'SPSI', 0):
        with pytest.raises(ValueError, match="init"):
            griffin_lim(mag, STFT(1024, 256, 1024), 2, init=bad)
        with pytest.raises(ValueError, match="init"):
            GriffinLimVocoder(taco, init=bad)
    assert VOCODERS == ('griffin_lim', 'griffin_lim_fast', 'spsi')
    v = GriffinLimVocoder.named('spsi', taco)
    assert (v.init, v.n_iters, v.momentum, v.inversion, v.inversion_iters) == ('spsi', 0, 0.0, 'nnls', 100)
    v = GriffinLimVocoder.named('spsi', taco, speed=0.8, pitch=2.0)
    assert (v.init, v.n_iters, v.speed, v.pitch) == ('spsi', 0, 0.8, 2.0)
    # the two names from before construct what they did, and the plain constructor draws its phases
    v = GriffinLimVocoder.named('griffin_lim', taco)
    assert (v.init, v.n_iters, v.momentum, v.inversion, v.inversion_iters) == ('random', 60, 0.0, 'pinv', 100)
    v = GriffinLimVocoder.named('griffin_lim_fast', taco)
    assert (v.init, v.n_iters, v.momentum, v.inversion, v.inversion_iters) == ('random', 60, 0.99, 'nnls', 100)
    assert GriffinLimVocoder(taco).init == 'random'
    with pytest.raises(ValueError, match="'spsi'"):
        Synthesizer(HP.create_hparams()).load(str(tmp_path / 'no_such_checkpoint'), vocoder='waveglow')
    assert build_arg_parser().parse_args(['--load_path', 'x', '--vocoder', 'spsi']).vocoder == 'spsi'
    base = ['--load_path', 'x', '--filelist_path', 'y', '--out', 'z']
    assert evaluate.parse_args(base + ['--prosody', '--vocoder', 'spsi']).vocoder == 'spsi'
    assert evaluate.parse_args(base).vocoder == 'griffin_lim'


def test_the_entry_points_are_declared():
    import t2v_hip
    assert 't2v_spsi' in t2v_hip.EXPORTS and 't2v_spsi_scratch_bytes' in t2v_hip.EXPORTS
    assert callable(t2v_hip.spsi_phase)
