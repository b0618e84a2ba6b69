"""Griffin-Lim vocoder and the reference's STFT surface on the GPU (csrc/vocoder.hip): STFT.transform / inverse /
forward and griffin_lim against the reference's own outputs (tests/golden/griffin_lim.npz) and the fp64 restatement of
test_vocoder.py, ragged batches, the mel -> waveform chain and Synthesizer(vocoder='griffin_lim')."""
import os

import numpy as np
import pytest
import torch

from test_vocoder import griffin_lim64, istft64, reference_angles, spectral_convergence, stft64

pytestmark = pytest.mark.gpu

# fp64 restatement of test_end_to_end_mel_chain's chain, computed on the CPU build machine (stft64 / griffin_lim64 of
# test_vocoder.py, mel_basis = slaney_mel_filterbank(16000, 1024, 80, 0, 8000), 60 iterations from the seed-7 angles):
# mean |log-mel(GL output) - log-mel(clip)| = 0.0990 (peak |sample| 0.846; at 30 iterations 0.1075)
E2E_FP64_MEAN_ABS_DLOGMEL = 0.0990


@pytest.fixture(scope='module')
def gl_golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'griffin_lim.npz'))


@pytest.fixture(scope='module')
def stft_fn():
    from stft import STFT
    return STFT(1024, 256, 1024)


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def test_transform_matches_reference(gl_golden, stft_fn):
    g = gl_golden
    x = torch.from_numpy(g['clip'].astype(np.float32) / 32768.0)[None].cuda()
    mag, phase = stft_fn.transform(x)
    assert mag.is_cuda and mag.shape == (1, 513, g['magnitude'].shape[1]) and phase.shape == mag.shape
    mag, phase = mag[0].cpu().numpy(), phase[0].cpu().numpy()
    ref_mag, ref_phase = g['magnitude'], g['phase']
    assert np.abs(mag - ref_mag).max() <= 1e-4 * ref_mag.max()
    sel = ref_mag > 1e-3 * ref_mag.max()
    assert sel.sum() > 1000
    assert np.abs(np.exp(1j * phase[sel]) - np.exp(1j * ref_phase[sel])).max() < 2e-3
    assert np.all(np.abs(phase) <= np.pi)
    # CPU input: computed on the GPU, returned on the CPU
    mag_c, _ = stft_fn.transform(x.cpu())
    assert not mag_c.is_cuda and np.array_equal(mag_c[0].numpy(), mag)


def test_inverse_matches_reference(gl_golden, stft_fn):
    g = gl_golden
    mag, phase = torch.from_numpy(g['magnitude'])[None], torch.from_numpy(g['phase'])[None]
    y = stft_fn.inverse(mag.cuda(), phase.cuda())
    assert y.is_cuda and y.shape == (1, 1, 256 * (mag.size(2) - 1))
    y = y[0, 0].cpu().numpy()
    ref = g['inverse']
    y64 = istft64(g['magnitude'].astype(np.float64), g['phase'].astype(np.float64))
    assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    assert _rms(y - y64) <= _rms(ref - y64) + 1e-6 * _rms(y64), (_rms(y - y64), _rms(ref - y64))


def test_round_trip_reconstructs_signal(stft_fn):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 12800, generator=g) - 0.5
    y = stft_fn.forward(x.cuda())
    assert y.shape == (2, 1, 12800) and stft_fn.magnitude.shape == (2, 513, 51)
    err = (y[:, 0].cpu() - x)[:, 1024:-1024].abs().max().item()
    assert err <= 1e-5, err


def test_griffin_lim_matches_reference(gl_golden, stft_fn):
    from audio_processing import griffin_lim
    g = gl_golden
    seed, n_iters = int(g['seed']), int(g['n_iters'])
    mag = torch.from_numpy(g['magnitude'])[None].cuda()
    np.random.seed(seed)
    y = griffin_lim(mag, stft_fn, n_iters)
    assert y.is_cuda and y.shape == (1, 256 * (mag.size(2) - 1))
    y = y[0].cpu().numpy()
    m64 = g['magnitude'].astype(np.float64)
    y64 = griffin_lim64(m64, reference_angles(seed, (1,) + m64.shape)[0].astype(np.float64), n_iters)
    rel = np.linalg.norm(y - y64) / np.linalg.norm(y64)
    assert rel <= 2 * float(g['gl_rel_l2_vs_fp64']), (rel, float(g['gl_rel_l2_vs_fp64']))
    sc, sc_ref = spectral_convergence(y, m64), spectral_convergence(g['griffin_lim'].astype(np.float64), m64)
    assert abs(sc - sc_ref) <= 0.01 * sc_ref, (sc, sc_ref)
    # explicit angles: the same starting point, the same result
    a = torch.from_numpy(reference_angles(seed, tuple(mag.shape)))
    y2 = griffin_lim(mag, stft_fn, n_iters, angles=a.cuda())[0].cpu().numpy()
    assert np.array_equal(y2, y)


def test_ragged_batch_equals_single_calls(gl_golden, stft_fn):
    from audio_processing import griffin_lim
    mag_all = torch.from_numpy(gl_golden['magnitude'])
    Ts = [65, 40, 23]
    g = torch.Generator().manual_seed(5)
    mags = [mag_all[:, 3 * i:3 * i + T] * (1.0 + 0.1 * i) for i, T in enumerate(Ts)]
    angs = [(torch.rand(513, T, generator=g) * 2 - 1) * np.pi for T in Ts]
    M = torch.zeros(3, 513, max(Ts))
    A = torch.full((3, 513, max(Ts)), 7.0)          # junk past each length must not matter
    for i, T in enumerate(Ts):
        M[i, :, :T], A[i, :, :T] = mags[i], angs[i]
    M[1, :, Ts[1]:] = 5.0
    lengths = torch.tensor(Ts)
    out = griffin_lim(M.cuda(), stft_fn, 12, angles=A.cuda(), lengths=lengths).cpu()
    assert out.shape == (3, 256 * (max(Ts) - 1))
    for i, T in enumerate(Ts):
        one = griffin_lim(mags[i][None].cuda(), stft_fn, 12, angles=angs[i][None].cuda())[0].cpu()
        n = 256 * (T - 1)
        assert (out[i, :n] - one).abs().max().item() <= 1e-6
        assert torch.all(out[i, n:] == 0)
    # the inverse and the transform take lengths too
    inv = stft_fn.inverse(M.cuda(), A.cuda(), lengths=lengths)[:, 0].cpu()
    for i, T in enumerate(Ts):
        n = 256 * (T - 1)
        one = stft_fn.inverse(mags[i][None].cuda(), angs[i][None].cuda())[0, 0].cpu()
        assert (inv[i, :n] - one).abs().max().item() <= 1e-6 and torch.all(inv[i, n:] == 0)
    sig = torch.zeros(3, 256 * (max(Ts) - 1))
    for i, T in enumerate(Ts):
        sig[i, :256 * (T - 1)] = out[i, :256 * (T - 1)]
    m2, p2 = stft_fn.transform(sig.cuda(), lengths=torch.tensor([256 * (T - 1) for T in Ts]))
    for i, T in enumerate(Ts):
        mo, po = stft_fn.transform(sig[i:i + 1, :256 * (T - 1)].cuda())
        assert torch.equal(m2[i, :, :T], mo[0]) and torch.equal(p2[i, :, :T], po[0])
        assert torch.all(m2[i, :, T:] == 0) and torch.all(p2[i, :, T:] == 0)


def test_end_to_end_mel_chain(gl_golden):
    """speech clip -> HIP mel -> mel_to_magnitude -> 60 Griffin-Lim iterations -> HIP mel again.  The vocoder's samples
    are not clipped: they may exceed +-1 slightly, so the second mel takes them through the float path unchecked."""
    from audio_processing import griffin_lim
    from layers import TacotronSTFT
    taco = TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)
    clip = torch.from_numpy(gl_golden['clip'].astype(np.int64)).to(torch.int16)[None].cuda()
    mel = taco.mel_spectrogram(clip, scale=1.0 / 32768.0)
    mag = taco.mel_to_magnitude(mel)
    P = np.linalg.pinv(taco.mel_basis.double().numpy())
    want = np.maximum(P @ np.exp(mel[0].double().cpu().numpy()), 0)
    assert np.abs(mag[0].cpu().numpy() - want).max() <= 1e-5 * want.max()
    np.random.seed(int(gl_golden['seed']))
    y = griffin_lim(mag, taco.stft_fn, 60)
    assert torch.isfinite(y).all()
    import t2v_hip        # (mel_spectrogram asserts |y| <= 1; the front end kernel itself takes any float samples)
    mel2 = t2v_hip.mel_frontend(y.contiguous(), torch.tensor([y.size(1)]), taco._tables(y.device))
    assert mel2.shape == mel.shape
    d = (mel2 - mel).abs().mean().item()
    assert d <= 1.5 * E2E_FP64_MEAN_ABS_DLOGMEL, d


def test_synthesizer_writes_griffin_lim_wav(tmp_path):
    import hparams as HP
    import train as TR
    from scipy.io.wavfile import read
    from synthesizer import GriffinLimVocoder, Synthesizer
    hp = HP.create_hparams("max_decoder_steps=40")
    torch.manual_seed(1234)
    model = TR.load_model(hp)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd['decoder.gate_layer.linear_layer.bias'].fill_(-1e3)        # never stops: decodes max_decoder_steps frames
    ck = str(tmp_path / 'ckpt_1')
    torch.save({'iteration': 1, 'state_dict': sd, 'optimizer': {}, 'learning_rate': 1e-3}, ck)
    np.savez(Synthesizer.centroid_cache_path(ck, 'x_test.txt'), zs=np.zeros((4, hp.z_latent_dim), np.float32),
             emotions=np.arange(4))
    syn = Synthesizer(hp).load(ck, vocoder='griffin_lim', filelist_path='x_test.txt')
    assert isinstance(syn.vocoder, GriffinLimVocoder) and syn.vocoder.n_iters == 60
    path = str(tmp_path / 'x.wav')
    mel, _ = syn.synthesize("안녕하세요", path)
    assert mel.size(2) == 40
    sr, data = read(path)
    assert sr == 16000 and data.shape == (39 * 256,) and np.all(np.isfinite(data))
    assert not os.path.exists(path + '.npy')
