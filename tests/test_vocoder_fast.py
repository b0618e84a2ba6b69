"""NNLS mel inversion and fast Griffin-Lim, CPU side: the fp64 restatement of tests/vocoder_ref.py against the properties the
GPU tests lean on (a non-increasing objective, the residuals of DESIGN 7i's table, momentum 0 = plain Griffin-Lim), the
two-tap form of the filterbank, and the argument errors of the Python wrappers that need no GPU."""
import os

import numpy as np
import pytest

import vocoder_ref as R
from test_vocoder import griffin_lim64, reference_angles

# DESIGN 7i, CPU fp64: ||B M - m|| / ||m|| after 200 projected-gradient steps from the clipped pinv; m = B S, S the unpadded
# frame magnitudes of a 2 s five-harmonic tone (amplitudes 1 / k)
TABLE_PG200 = {91: 1.7e-4, 125: 8.4e-3, 139: 4.5e-3, 220: 1.1e-3}
TABLE_PINV = {91: 8.5e-2, 125: 1.2e-1, 139: 1.2e-1, 220: 9.9e-2}


@pytest.fixture(scope='module')
def basis():
    from layers import slaney_mel_filterbank
    return slaney_mel_filterbank(16000, 1024, 80, 0.0, 8000.0).astype(np.float32)


@pytest.fixture(scope='module')
def pinv(basis):
    return np.linalg.pinv(basis.astype(np.float64))


@pytest.fixture(scope='module')
def tone_mels(basis):
    return {f: basis.astype(np.float64) @ R.frame_magnitudes(R.tone(f)) for f in TABLE_PG200}


def _rel_residual(basis, M, m):
    return float(np.linalg.norm(basis.astype(np.float64) @ M - m) / np.linalg.norm(m))


def test_objective_never_increases(basis, pinv, tone_mels):
    for f, m in tone_mels.items():
        trace = []
        R.nnls(m[:, ::8], basis, pinv, 200, trace=trace)
        t = np.array(trace)
        assert len(t) == 201 and np.all(t[1:] <= t[:-1] * (1 + 1e-12)), (f, np.max(t[1:] / t[:-1]))
        assert t[-1] < 0.05 * t[0], (f, t[0], t[-1])


def test_residuals_of_the_design_table(basis, pinv, tone_mels):
    for f, m in tone_mels.items():
        r0 = _rel_residual(basis, R.nnls(m, basis, pinv, 0), m)
        r200 = _rel_residual(basis, R.nnls(m, basis, pinv, 200), m)
        print("tone %d Hz: clipped pinv %.3g, after 200 steps %.3g (table %.2g, %.2g)" % (f, r0, r200, TABLE_PINV[f], TABLE_PG200[f]))
        assert abs(r200 - TABLE_PG200[f]) <= 0.1 * TABLE_PG200[f], (f, r200)
        assert abs(r0 - TABLE_PINV[f]) <= 0.1 * TABLE_PINV[f], (f, r0)


def test_zero_iterations_is_the_clipped_pinv(basis, pinv, tone_mels):
    m = tone_mels[125][:, :20]
    M0 = R.nnls(m, basis, pinv, 0)
    assert np.array_equal(M0, R.clipped_pinv(m, pinv))
    assert np.abs(M0 - np.maximum(pinv @ m, 0)).max() <= 1e-12 * M0.max()
    assert M0.min() == 0.0                  # the clip is active: the problem is constrained on these inputs


def test_ordered_sums_equal_the_dense_iteration(basis, pinv, tone_mels):
    """the kernel's order of summation against B^T (B M - m) as the algorithm is written; the two differ only in L, which
    the kernel takes as one float (2^-24 relative on the step length)"""
    m = tone_mels[220][:, :20]
    a, b = R.nnls(m, basis, pinv, 50), R.nnls_dense(m, basis, pinv, 50)
    assert np.abs(a - b).max() <= 1e-6 * b.max()
    M = R.clipped_pinv(m, pinv)
    assert np.abs(R.apply_basis(basis, M) - basis.astype(np.float64) @ M).max() <= 1e-13 * m.max()


def test_two_tap_form_of_the_basis(basis):
    import torch
    import t2v_hip
    t = t2v_hip.two_tap_basis(torch.from_numpy(basis))
    lo, w0, w1 = R.bin_taps(basis)
    assert np.array_equal(t['lo'].numpy(), lo) and np.array_equal(t['w0'].numpy(), w0) and np.array_equal(t['w1'].numpy(), w1)
    start, length, _ = R.filter_rows(basis)
    assert np.array_equal(t['start'].numpy(), start) and np.array_equal(t['len'].numpy(), length)
    assert t['lo'].dtype == torch.int32 and int(t['lo'].min()) >= 0 and int(t['lo'].max()) <= 78
    assert int((t['start'] + t['len']).max()) <= 513
    assert t['L'] == R.lipschitz(basis) and abs(t['L'] - 1.7166e-3) < 1e-7
    assert np.nonzero(basis.sum(0) == 0)[0].tolist() == [0, 512]            # the two bins no filter covers
    # a basis without the structure is refused: a third filter on one bin, a gap inside a filter is fine (weights 0)
    bad = basis.copy()
    bad[40, int(start[10])] = 0.5
    with pytest.raises(ValueError):
        t2v_hip.two_tap_basis(torch.from_numpy(bad))
    with pytest.raises(ValueError):
        R.bin_taps(bad)
    with pytest.raises(ValueError):
        t2v_hip.two_tap_basis(torch.from_numpy(basis[:, :512]))


def test_momentum_zero_is_plain_griffin_lim(golden_dir):
    g = np.load(os.path.join(golden_dir, 'griffin_lim.npz'))
    mag = g['magnitude'].astype(np.float64)
    angles = reference_angles(int(g['seed']), (1,) + mag.shape)[0].astype(np.float64)
    for n in (0, 1, 8):
        want, got = griffin_lim64(mag, angles, n), R.griffin_lim(mag, angles, n, momentum=0.0)
        assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), n
    # and momentum does something: the first iteration has tprev = 0, the second does not
    a, b = R.griffin_lim(mag, angles, 1, 0.99), R.griffin_lim(mag, angles, 1, 0.0)
    assert np.array_equal(a, b)
    a, b = R.griffin_lim(mag, angles, 2, 0.99), R.griffin_lim(mag, angles, 2, 0.0)
    assert np.linalg.norm(a - b) > 1e-3 * np.linalg.norm(b)


def test_fast_griffin_lim_converges_further_on_the_golden_clip(golden_dir):
    """the order test_vocoder_fast_gpu.py asserts of the kernels, shown by the reference itself on the same input"""
    g = np.load(os.path.join(golden_dir, 'griffin_lim.npz'))
    mag = g['magnitude'].astype(np.float64)
    angles = reference_angles(int(g['seed']), (1,) + mag.shape)[0].astype(np.float64)
    plain = R.spectral_convergence(R.griffin_lim(mag, angles, 60, 0.0), mag)
    fast = R.spectral_convergence(R.griffin_lim(mag, angles, 60, 0.99), mag)
    print("spectral convergence at 60 iterations: plain %.5f, momentum 0.99 %.5f" % (plain, fast))
    assert fast < 0.75 * plain, (fast, plain)


def test_wrappers_refuse_bad_arguments(tmp_path):
    import torch
    from audio_processing import griffin_lim
    from layers import TacotronSTFT
    from stft import STFT
    from synthesizer import GriffinLimVocoder, Synthesizer, build_arg_parser
    import evaluate
    import hparams as HP
    taco = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    with pytest.raises(ValueError, match="method"):
        taco.mel_to_magnitude(torch.zeros(1, 80, 8), method='lstsq')
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match="momentum"):
            griffin_lim(torch.ones(1, 513, 8), STFT(1024, 256, 1024), 2, momentum=bad)
        with pytest.raises(ValueError, match="momentum"):
            GriffinLimVocoder(taco, momentum=bad)
    with pytest.raises(ValueError, match="inversion"):
        GriffinLimVocoder(taco, inversion='lstsq')
    v = GriffinLimVocoder(taco)
    assert (v.n_iters, v.momentum, v.inversion, v.inversion_iters) == (60, 0.0, 'pinv', 100)
    with pytest.raises(ValueError, match="'griffin_lim', 'griffin_lim_fast'"):
        Synthesizer(HP.create_hparams()).load(str(tmp_path / 'no_such_checkpoint'), vocoder='waveglow')
    assert build_arg_parser().parse_args(['--load_path', 'x', '--vocoder', 'griffin_lim_fast']).vocoder == 'griffin_lim_fast'
    base = ['--load_path', 'x', '--filelist_path', 'y', '--out', 'z']
    assert evaluate.parse_args(base).vocoder == 'griffin_lim'
    assert evaluate.parse_args(base + ['--prosody', '--vocoder', 'griffin_lim_fast']).vocoder == 'griffin_lim_fast'
    with pytest.raises(SystemExit):
        evaluate.parse_args(base + ['--vocoder', 'waveglow'])
