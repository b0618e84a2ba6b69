"""NNLS mel inversion (k_mel_to_mag_nnls) and fast Griffin-Lim (k_gl_iter_fast) on the GPU against the fp64 restatement
of tests/vocoder_ref.py.

Error rule of the value tests (the convention of tests/test_tsne_gpu.py): kernel error <= 4 x max(error of the same
restatement run in fp32 numpy, one fp32 rounding of the reference).  The projected-gradient iteration is a composition of
non-expansive maps (I - B^T B / L has norm <= 1, so has the projection), so rounding does not amplify: the error after n
steps is at most n times one step's rounding, and the fp32 restatement, which sums in the kernel's order, measures that."""
import os

import numpy as np
import pytest
import torch

import vocoder_ref as R
from test_vocoder import reference_angles

pytestmark = pytest.mark.gpu

HALF_ULP = 2.0 ** -24
T_STRIDE = 53
NNLS_ITERS = (0, 1, 100)


@pytest.fixture(scope='module')
def gl_golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'griffin_lim.npz'))


@pytest.fixture(scope='module')
def taco():
    from layers import TacotronSTFT
    return TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)


@pytest.fixture(scope='module')
def stft_fn(taco):
    return taco.stft_fn


@pytest.fixture(scope='module')
def mel_case(gl_golden, taco):
    """five rows of 50, 17, 16, 15 and 1 frames (a workgroup owns 16) in one batch at stride 53, NaN past each length: log
    mels (fp32) of the golden clip and of two tones, with the fp64 reference and the fp32 yardstick of every iteration count"""
    basis = taco.mel_basis.numpy()
    pinv32 = np.linalg.pinv(basis.astype(np.float64)).astype(np.float32)     # the table TacotronSTFT hands the kernel
    B64 = basis.astype(np.float64)
    src = {'clip': gl_golden['magnitude'].astype(np.float64),
           't100': 0.05 * np.abs(R.stft(R.tone(100.0, 1.0))), 't220': 0.05 * np.abs(R.stft(R.tone(220.0, 1.0)))}
    rows = [('clip', 0, 50), ('clip', 48, 17), ('t100', 0, 16), ('t220', 3, 15), ('t100', 30, 1)]
    lengths = [n for _, _, n in rows]
    mel = np.full((len(rows), 80, T_STRIDE), np.nan, dtype=np.float32)
    for b, (name, t0, n) in enumerate(rows):
        mel[b, :, :n] = np.log(np.maximum(B64 @ src[name][:, t0:t0 + n], 1e-5)).astype(np.float32)
    cat = np.concatenate([mel[b, :, :n] for b, n in enumerate(lengths)], axis=1)          # (80, 99) valid frames
    ref = {n: R.nnls(np.exp(cat.astype(np.float64)), basis, pinv32, n) for n in NNLS_ITERS}
    yard = {n: R.nnls(np.exp(cat), basis, pinv32, n, dtype=np.float32) for n in NNLS_ITERS}
    assert yard[100].dtype == np.float32
    return dict(mel=mel, lengths=lengths, cat=cat, ref=ref, yard=yard, basis=basis, m64=np.exp(cat.astype(np.float64)))


def _valid(out, lengths):
    """(B, 513, T) device tensor -> (513, sum lengths) numpy of the valid frames, rows in order"""
    o = out.cpu().numpy()
    return np.concatenate([o[b, :, :n] for b, n in enumerate(lengths)], axis=1)


@pytest.fixture(scope='module')
def nnls_out(mel_case, taco):
    """the kernel's outputs for every iteration count, computed once; the input is checked to be untouched"""
    c = mel_case
    mel = torch.from_numpy(c['mel']).cuda()
    before = mel.clone()
    out = {n: taco.mel_to_magnitude(mel, c['lengths'], method='nnls', n_iters=n) for n in NNLS_ITERS}
    out['pinv'] = taco.mel_to_magnitude(mel, c['lengths'])
    assert torch.equal(mel.view(torch.int32), before.view(torch.int32))
    return mel, out


def test_nnls_matches_fp64(mel_case, nnls_out):
    c, (_, out) = mel_case, nnls_out
    for n in NNLS_ITERS:
        ref = c['ref'][n]
        scale = ref.max()
        e_k = np.abs(_valid(out[n], c['lengths']).astype(np.float64) - ref).max() / scale
        e_y = np.abs(c['yard'][n].astype(np.float64) - ref).max() / scale
        print("nnls n_iters %3d: max |err| / max M kernel %.3g, fp32 numpy %.3g, ratio %.3g" % (n, e_k, e_y, e_k / max(e_y, HALF_ULP)))
        assert e_k <= 4 * max(e_y, HALF_ULP), (n, e_k, e_y)
        assert out[n].dtype == torch.float32 and out[n].shape == (5, 513, T_STRIDE)


def test_nnls_lowers_every_frames_mel_residual(mel_case, nnls_out):
    c, (_, out) = mel_case, nnls_out
    m = c['m64']
    r_pinv = R.mel_residual(c['basis'], _valid(out['pinv'], c['lengths']), m)
    r_nnls = R.mel_residual(c['basis'], _valid(out[100], c['lengths']), m)
    r_ref = R.mel_residual(c['basis'], c['ref'][100], m)
    slack = 1e-5 * np.sqrt(np.sum(m * m, axis=0))
    print("mel residual over %d frames: pinv %.4g, nnls(100) %.4g (fp64 reference %.4g), ratio %.3g; worst frame nnls / pinv %.3g"
          % (len(r_pinv), r_pinv.sum(), r_nnls.sum(), r_ref.sum(), r_nnls.sum() / r_pinv.sum(), np.max(r_nnls / np.maximum(r_pinv, 1e-300))))
    assert np.all(r_nnls <= r_pinv + slack), np.max(r_nnls - r_pinv - slack)
    assert r_nnls.sum() <= 0.5 * r_pinv.sum(), (r_nnls.sum(), r_pinv.sum())
    assert torch.equal(out[0], out['pinv'])                 # n_iters = 0: the clipped pinv's bits
    assert float(out[100].min()) >= 0.0


def test_nnls_rows_do_not_depend_on_the_batch(mel_case, nnls_out, taco):
    c, (mel, out) = mel_case, nnls_out
    lengths, full = c['lengths'], out[100]
    for b, n in enumerate(lengths):
        assert torch.all(full[b, :, n:] == 0), b
        alone = taco.mel_to_magnitude(mel[b:b + 1, :, :n].contiguous(), [n], method='nnls')
        assert alone.shape == (1, 513, n) and torch.equal(alone[0], full[b, :, :n]), b
    order = [3, 0, 4, 2, 1]
    rev = taco.mel_to_magnitude(mel[order].contiguous(), [lengths[i] for i in order], method='nnls')
    for j, i in enumerate(order):
        assert torch.equal(rev[j], full[i]), i
    big = torch.full((9, 80, T_STRIDE + 11), float('nan'), device='cuda')
    big[2:7, :, 4:4 + T_STRIDE] = mel
    before = big.clone()
    via = taco.mel_to_magnitude(big[2:7, :, 4:4 + T_STRIDE], lengths, method='nnls')            # a strided view
    assert torch.equal(via, full)
    wide = taco.mel_to_magnitude(big[2:7, :, 4:], lengths, method='nnls')                        # another stride
    assert torch.equal(wide[:, :, :T_STRIDE], full) and torch.all(wide[:, :, T_STRIDE:] == 0)
    assert torch.equal(big.view(torch.int32), before.view(torch.int32))
    # the t2v_hip entry with the basis tensor itself (the two-tap form built per call) and with CPU input
    import t2v_hip
    P = taco._pinv[str(mel.device)]
    direct = t2v_hip.mel_to_magnitude_nnls(mel, lengths, taco.mel_basis, P)
    assert torch.equal(direct, full)
    cpu = taco.mel_to_magnitude(mel.cpu(), lengths, method='nnls', n_iters=100)
    assert not cpu.is_cuda and torch.equal(cpu, full.cpu())


@pytest.fixture(scope='module')
def gl_case(gl_golden):
    mag = gl_golden['magnitude']
    angles = reference_angles(int(gl_golden['seed']), (1,) + mag.shape)[0]
    return mag, angles


def test_fast_griffin_lim_matches_fp64(gl_case, stft_fn):
    from audio_processing import griffin_lim
    mag, angles = gl_case
    m64, a64 = mag.astype(np.float64), angles.astype(np.float64)
    M, A = torch.from_numpy(mag)[None].cuda(), torch.from_numpy(angles)[None].cuda()
    # 8 iterations: the waveform itself (over many iterations the phase of near-empty bins diverges chaotically)
    y = griffin_lim(M, stft_fn, 8, angles=A, momentum=0.99)
    assert y.is_cuda and y.shape == (1, 256 * (mag.shape[1] - 1))
    y = y[0].cpu().numpy().astype(np.float64)
    ref = R.griffin_lim(m64, a64, 8, 0.99)
    yard = R.griffin_lim(mag, angles, 8, 0.99, dtype=np.float32)
    assert yard.dtype == np.float32
    e_k = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    e_y = np.linalg.norm(yard.astype(np.float64) - ref) / np.linalg.norm(ref)
    print("fast Griffin-Lim, 8 iterations: rel L2 kernel %.3g, fp32 numpy %.3g, ratio %.3g" % (e_k, e_y, e_k / e_y))
    assert e_k <= 4 * max(e_y, HALF_ULP), (e_k, e_y)
    # 60 iterations: the spectral convergence, against the reference's and against the plain iteration's
    y60 = griffin_lim(M, stft_fn, 60, angles=A, momentum=0.99)[0].cpu().numpy()
    p60 = griffin_lim(M, stft_fn, 60, angles=A)[0].cpu().numpy()
    sc, sc_plain = R.spectral_convergence(y60, m64), R.spectral_convergence(p60, m64)
    sc_ref = R.spectral_convergence(R.griffin_lim(m64, a64, 60, 0.99), m64)
    print("spectral convergence at 60 iterations: kernel %.5f, fp64 %.5f, plain kernel %.5f" % (sc, sc_ref, sc_plain))
    assert np.isfinite(y60).all() and abs(sc - sc_ref) <= 0.01 * sc_ref, (sc, sc_ref)
    assert sc < sc_plain, (sc, sc_plain)        # the reference shows this order on this clip (tests/test_vocoder_fast.py)


def test_momentum_zero_is_the_plain_call_and_runs_repeat(gl_case, stft_fn):
    from audio_processing import griffin_lim
    import t2v_hip
    mag, angles = gl_case
    M, A = torch.from_numpy(mag)[None].cuda(), torch.from_numpy(angles)[None].cuda()
    plain = griffin_lim(M, stft_fn, 12, angles=A)
    assert torch.equal(griffin_lim(M, stft_fn, 12, angles=A, momentum=0.0), plain)
    fast = griffin_lim(M, stft_fn, 12, angles=A, momentum=0.99)
    assert torch.equal(griffin_lim(M, stft_fn, 12, angles=A, momentum=0.99), fast)
    assert not torch.equal(fast, plain)
    # one iteration has no previous transform yet: the plain iteration's result
    assert torch.equal(griffin_lim(M, stft_fn, 1, angles=A, momentum=0.5), griffin_lim(M, stft_fn, 1, angles=A))
    # the C entry with momentum 0 is t2v_griffin_lim
    lib = t2v_hip.load_library()
    tb = stft_fn.tables(M.device)
    n = torch.tensor([mag.shape[1]], dtype=torch.int32, device='cuda')
    out = torch.empty_like(plain)
    scratch = torch.empty(lib.t2v_griffin_lim_fast_scratch_bytes(1, mag.shape[1]), dtype=torch.uint8, device='cuda')
    p = t2v_hip._p
    rc = lib.t2v_griffin_lim_fast(p(M), p(A), p(n), 1, mag.shape[1], 1024, 256, 12, 0.0, p(tb['window']), p(tb['tw512']),
                                  p(tb['tw1024']), p(scratch), p(out), out.size(1), t2v_hip._stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, plain)


def test_ragged_fast_batch_equals_single_calls(gl_golden, stft_fn, taco):
    from audio_processing import griffin_lim
    from synthesizer import GriffinLimVocoder
    mag_all = torch.from_numpy(gl_golden['magnitude'])
    Ts = [4, 21, 50]
    g = torch.Generator().manual_seed(5)
    mags = [mag_all[:, 5 * i:5 * i + T] * (1.0 + 0.1 * i) for i, T in enumerate(Ts)]
    angs = [(torch.rand(513, T, generator=g) * 2 - 1) * np.pi for T in Ts]
    M = torch.zeros(3, 513, max(Ts))
    A = torch.full((3, 513, max(Ts)), 7.0)          # junk past each length must not matter
    for i, T in enumerate(Ts):
        M[i, :, :T], A[i, :, :T] = mags[i], angs[i]
    M[1, :, Ts[1]:] = 5.0
    out = griffin_lim(M.cuda(), stft_fn, 12, angles=A.cuda(), lengths=torch.tensor(Ts), momentum=0.99).cpu()
    assert out.shape == (3, 256 * (max(Ts) - 1))
    for i, T in enumerate(Ts):
        one = griffin_lim(mags[i][None].cuda(), stft_fn, 12, angles=angs[i][None].cuda(), momentum=0.99)[0].cpu()
        n = 256 * (T - 1)
        assert (out[i, :n] - one).abs().max().item() <= 1e-6, i
        assert torch.all(out[i, n:] == 0)
    # the vocoder: a ragged batch against item-by-item calls under the same np.random seed
    voc = GriffinLimVocoder(taco, n_iters=12, momentum=0.99, inversion='nnls')
    mel = torch.full((3, 80, max(Ts)), float('nan'))
    basis = taco.mel_basis.double()
    for i, T in enumerate(Ts):
        mel[i, :, :T] = torch.log(torch.clamp(basis @ mags[i].double(), min=1e-5)).float()
    mel = mel.cuda()
    np.random.seed(11)
    wavs = voc.batch(mel, Ts)
    np.random.seed(11)
    for i, T in enumerate(Ts):
        one = voc(mel[i:i + 1, :, :T].contiguous())[0]
        assert wavs[i].shape == one.shape == (256 * (T - 1),)
        assert torch.isfinite(one).all() and (wavs[i] - one).abs().max().item() <= 1e-6, i
    # the options do not change which phases are drawn
    np.random.seed(11)
    GriffinLimVocoder(taco, n_iters=1).batch(mel, Ts)
    a = np.random.rand()
    np.random.seed(11)
    voc.batch(mel, Ts)
    assert np.random.rand() == a


def test_c_entries_refuse_bad_arguments(taco, stft_fn):
    import t2v_hip
    lib = t2v_hip.load_library()
    p, T, B = t2v_hip._p, 8, 2
    dev = torch.device('cuda')
    mel = torch.zeros(B, 80, T, device=dev)
    mag = torch.empty(B, 513, T, device=dev)
    n = torch.full((B,), T, dtype=torch.int32, device=dev)
    taco.mel_to_magnitude(mel, method='nnls', n_iters=1)                    # fills the per-device tables
    P, tp = taco._pinv[str(mel.device)], taco._taps[str(mel.device)]

    def nnls(mel_=mel, P_=P, lo=tp['lo'], w0=tp['w0'], w1=tp['w1'], st=tp['start'], ln=tp['len'], L=tp['L'], it=3, n_=n, B_=B,
             ts=T, nm=80, out=mag):
        q = lambda x: None if x is None else p(x)
        return lib.t2v_mel_to_magnitude_nnls(q(mel_), q(P_), q(lo), q(w0), q(w1), q(st), q(ln), L, it, q(n_), B_, ts, nm, q(out),
                                             t2v_hip._stream())

    assert nnls() == 0
    assert nnls(nm=79) == -1 and nnls(nm=81) == -1                                              # T2V_ERR_DIMS
    for kw in (dict(mel_=None), dict(P_=None), dict(lo=None), dict(w0=None), dict(w1=None), dict(st=None), dict(ln=None),
               dict(n_=None), dict(out=None), dict(B_=0), dict(ts=0), dict(it=-1), dict(L=0.0), dict(L=-1.0), dict(L=float('nan'))):
        assert nnls(**kw) == -2, kw                                                             # T2V_ERR_ARG
    tb = stft_fn.tables(dev)
    ang = torch.zeros(B, 513, T, device=dev)
    out = torch.empty(B, 256 * (T - 1), device=dev)
    scratch = torch.empty(lib.t2v_griffin_lim_fast_scratch_bytes(B, T), dtype=torch.uint8, device=dev)
    assert lib.t2v_griffin_lim_fast_scratch_bytes(B, T) > lib.t2v_griffin_lim_scratch_bytes(B, T) + B * T * 513 * 8 - 1

    def gl(momentum=0.5, n_fft=1024, B_=B, it=2, sc=scratch):
        return lib.t2v_griffin_lim_fast(p(mag), p(ang), p(n), B_, T, n_fft, 256, it, momentum, p(tb['window']), p(tb['tw512']),
                                        p(tb['tw1024']), None if sc is None else p(sc), p(out), out.size(1), t2v_hip._stream())

    mag.fill_(1.0)
    assert gl() == 0 and gl(momentum=0.0) == 0
    assert gl(n_fft=800) == -1
    for kw in (dict(momentum=1.0), dict(momentum=-0.01), dict(momentum=float('nan')), dict(B_=0), dict(it=-1), dict(sc=None)):
        assert gl(**kw) == -2, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        t2v_hip.griffin_lim(mag, ang, None, tb, 2, momentum=1.0)
    with pytest.raises(ValueError):
        t2v_hip.mel_to_magnitude_nnls(mel, None, taco.mel_basis, P, n_iters=-1)


def test_synthesizer_loads_the_fast_vocoder(tmp_path):
    import hparams as HP
    import train as TR
    from scipy.io.wavfile import read
    from synthesizer import GriffinLimVocoder, Synthesizer, parse_args
    hp = HP.create_hparams("max_decoder_steps=40")
    torch.manual_seed(1234)
    model = TR.load_model(hp)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd['decoder.gate_layer.linear_layer.bias'].fill_(-1e3)        # never stops: decodes max_decoder_steps frames
    ck = str(tmp_path / 'ckpt_1')
    torch.save({'iteration': 1, 'state_dict': sd, 'optimizer': {}, 'learning_rate': 1e-3}, ck)
    np.savez(Synthesizer.centroid_cache_path(ck, 'x_test.txt'), zs=np.zeros((4, hp.z_latent_dim), np.float32),
             emotions=np.arange(4))
    syn = Synthesizer(hp).load(ck, vocoder='griffin_lim_fast', filelist_path='x_test.txt')
    v = syn.vocoder
    assert isinstance(v, GriffinLimVocoder) and (v.n_iters, v.momentum, v.inversion, v.inversion_iters) == (60, 0.99, 'nnls', 100)
    path = str(tmp_path / 'x.wav')
    mel, _ = syn.synthesize("안녕하세요", path)
    assert mel.size(2) == 40
    sr, data = read(path)
    assert sr == 16000 and data.shape == (39 * 256,) and np.all(np.isfinite(data))
    v = Synthesizer(hp).load(ck, vocoder='griffin_lim', filelist_path='x_test.txt').vocoder
    assert isinstance(v, GriffinLimVocoder) and (v.n_iters, v.momentum, v.inversion) == (60, 0.0, 'pinv')
    with pytest.raises(ValueError, match="'griffin_lim', 'griffin_lim_fast'"):
        Synthesizer(hp).load(ck, vocoder='waveglow', filelist_path='x_test.txt')
    assert parse_args(['--load_path', ck, '--text', 'x', '--vocoder', 'griffin_lim_fast']).vocoder == 'griffin_lim_fast'
