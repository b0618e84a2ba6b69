"""The phase start from magnitudes on the GPU (csrc/phase_init.hip k_spsi_scan, k_spsi_assign) against the integer-turn
restatement of tests/spsi_ref.py, and what stands on it: griffin_lim(init='spsi'), vocoder 'spsi'.

Error rule of the value test.  The kernels and the restatement do the same integer arithmetic on the same fp64 offsets, so bit
equality is expected and printed; what is asserted allows each rounded advance to differ by one unit (frame m has summed m + 1
of them, and one more unit for the offset of the assignment) plus the fp32 rounding of a phase below pi:
circular distance <= 2 pi (m + 2) 2^-30 + 2^-22 rad at frame m.  Measured on an MI355X: 0 of 488 376 elements differ in their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import spsi_ref as S
import vocoder_ref as R
import yin_ref as Y

pytestmark = pytest.mark.gpu

T, T_STRIDE = 130, 136
LENGTHS = [130, 65, 64, 63, 4, 1, 0]            # the scan's chunk of 64 frames from both sides, its carry, and an empty row
CHUNK = 65                                      # bins per wave of k_spsi_assign
EDGES = [CHUNK * w for w in range(1, 8)]        # the first bin of every chunk but the lowest


def _ramp(points):
    ks, vs = zip(*points)
    return np.interp(np.arange(S.BINS), ks, vs).astype(np.float32)


def _spikes(at):
    """1 everywhere (plateaus: no peaks) but the (bin, value) pairs"""
    fr = np.ones(S.BINS, dtype=np.float32)
    for k, v in at:
        fr[k] = v
    return fr


def crafted_frames():
    """frames that exercise the rules, in the order they are planted into row 0 from frame 3"""
    return [
        np.full(S.BINS, 0.75, dtype=np.float32),                                        # equal magnitudes: no peak, +0
        np.zeros(S.BINS, dtype=np.float32),                                             # zeros: no peak, +0
        _ramp([(0, 1.0), (1, 2.0), (512, 0.5)]),                                        # one peak, at bin 1
        _ramp([(0, 0.5), (511, 2.0), (512, 1.0)]),                                      # one peak, at bin 511
        _ramp([(0, 1.0), (64, 3.0), (65, 2.0), (66, 2.5), (512, 0.5)]),                 # peaks at 64 and 66: bin 65 ties -> 64
        _ramp([(0, 5.0), (50, 1.0), (100, 3.0), (101, 3.0), (200, 1.0), (300, 2.0), (511, 1.0), (512, 9.0)]),   # a plateau; peak 300
        _spikes([(e - 1, 3.0) for e in EDGES] + [(e + 1, 2.0) for e in EDGES]),         # peaks on both sides of every chunk edge
        _spikes([(e, 3.0) for e in EDGES] + [(e - 2, 2.0) for e in EDGES]),             # the edge bin itself and two below
        _spikes([(e, 2.0) for e in EDGES]),                                             # a chunk's first bin alone
        _spikes([(e - 1, 2.0) for e in EDGES]),                                         # a chunk's last bin alone
        _spikes([(e - 1, 2.0) for e in EDGES[::2]] + [(e, 2.0) for e in EDGES[1::2]]),  # chunks without a peak of their own
        _spikes([(511, 2.0)]), _spikes([(1, 2.0)]), _spikes([(256, 2.0), (258, 2.0)]),
    ]


def make_batch():
    """(mag (7, 513, 136) fp32, NaN at and past each length; log-normal magnitudes, the crafted frames in row 0)"""
    rs = np.random.RandomState(20151130)
    mag = np.full((len(LENGTHS), S.BINS, T_STRIDE), np.nan, dtype=np.float32)
    for b, n in enumerate(LENGTHS):
        mag[b, :, :n] = np.exp(rs.randn(S.BINS, n)).astype(np.float32)
    for i, fr in enumerate(crafted_frames()):
        mag[0, :, 3 + i] = fr
    mag[0, :, 70] = crafted_frames()[6]                   # and once behind the carry
    return mag


def raw_spsi(mag, lengths, t_frames):
    """t2v_spsi itself (the wrapper takes no empty row and no T below the stride): mag (B, 513, stride) device tensor"""
    import t2v_hip
    lib = t2v_hip.load_library()
    B, _, stride = mag.shape
    n = torch.tensor(lengths, dtype=torch.int32, device=mag.device)
    out = torch.full_like(mag, float('nan'))
    scratch = torch.empty(lib.t2v_spsi_scratch_bytes(B, stride), device=mag.device, dtype=torch.uint8)
    rc = lib.t2v_spsi(C.c_void_p(mag.data_ptr()), C.c_void_p(n.data_ptr()), B, t_frames, stride, C.c_void_p(out.data_ptr()),
                      C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def batch():
    mag = make_batch()
    ref = S.spsi_batch(mag, LENGTHS)
    dev = torch.from_numpy(mag).cuda()
    before = dev.clone()
    out = raw_spsi(dev, LENGTHS, T)
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32))
    return dict(mag=mag, ref=ref, dev=dev, out=out)


@pytest.fixture(scope='module')
def taco():
    from layers import TacotronSTFT
    return TacotronSTFT(1024, 256, 1024, 80, 16000, 0.0, 8000.0)


def test_kernel_matches_the_restatement(batch):
    out, ref = batch['out'].cpu().numpy(), batch['ref']
    assert out.dtype == np.float32 and out.shape == ref.shape
    for b, n in enumerate(LENGTHS):
        assert not out[b, :, n:].view(np.int32).any(), b            # exactly +0 at and past the length
    d = out.astype(np.float64) - ref.astype(np.float64)
    d = np.abs(d - 2.0 * np.pi * np.round(d / (2.0 * np.pi)))
    bound = 2.0 * np.pi * (np.arange(T_STRIDE) + 2) * 2.0 ** -30 + 2.0 ** -22
    differ = int(np.count_nonzero(out.view(np.int32) != ref.view(np.int32)))
    print("k_spsi against the restatement: %d of %d elements differ in their bits, largest circular distance %.3g rad, "
          "largest distance / bound %.3g" % (differ, out.size, d.max(), (d / bound[None, None, :]).max()))
    assert np.all(d <= bound[None, None, :]), float((d / bound[None, None, :]).max())
    assert out.min() >= np.float32(-np.pi) and out.max() < np.float32(np.pi)
    # the crafted frames did what they were made for: no peak -> +0, the tie -> the lower peak
    assert not out[0, :, 3:5].view(np.int32).any()
    pk = S.peaks(batch['mag'][0, :, 7:8])[:, 0]
    assert np.flatnonzero(pk).tolist() == [64, 66] and S.nearest_peak(pk)[65] == 64


def test_rows_do_not_depend_on_the_batch(batch):
    import t2v_hip
    dev, full = batch['dev'], batch['out']
    live = [b for b, n in enumerate(LENGTHS) if n >= 1]
    for b in live:
        n = LENGTHS[b]
        alone = t2v_hip.spsi_phase(dev[b:b + 1, :, :n].contiguous())
        assert alone.shape == (1, 513, n) and torch.equal(alone[0].view(torch.int32), full[b, :, :n].view(torch.int32)), b
    order = [3, 0, 5, 2, 4, 1]
    rev = t2v_hip.spsi_phase(dev[order].contiguous(), [LENGTHS[i] for i in order])
    for j, i in enumerate(order):
        assert torch.equal(rev[j].view(torch.int32), full[i].view(torch.int32)), i
    big = torch.full((9, 513, T_STRIDE + 14), float('nan'), device='cuda')
    big[1:7, :, 5:5 + T_STRIDE] = dev[:6]
    before = big.clone()
    via = t2v_hip.spsi_phase(big[1:7, :, 5:5 + T_STRIDE], LENGTHS[:6])                  # a strided view
    assert torch.equal(via.view(torch.int32), full[:6].view(torch.int32))
    wide = t2v_hip.spsi_phase(big[1:7, :, 5:], LENGTHS[:6])                             # another stride
    assert torch.equal(wide[:, :, :T_STRIDE].view(torch.int32), full[:6].view(torch.int32))
    assert not wide[:, :, T_STRIDE:].view(torch.int32).any()
    assert torch.equal(big.view(torch.int32), before.view(torch.int32))
    assert torch.equal(raw_spsi(dev, LENGTHS, T).view(torch.int32), full.view(torch.int32))     # and twice the same bits
    with pytest.raises(ValueError):
        t2v_hip.spsi_phase(dev, LENGTHS)                                                # an empty row
    with pytest.raises(ValueError):
        t2v_hip.spsi_phase(dev[:, :512], LENGTHS)


def test_griffin_lim_from_the_start(taco):
    import t2v_hip
    from audio_processing import griffin_lim
    stft = taco.stft_fn
    mag = np.stack([0.05 * np.abs(R.stft(R.tone(100.0, 1.0))), 0.05 * np.abs(R.stft(R.tone(220.0, 1.0)))]).astype(np.float32)
    mag = torch.from_numpy(mag).cuda()
    lengths = [mag.size(2), 40]
    np.random.seed(5)
    state = np.random.get_state()
    got = griffin_lim(mag, stft, 0, lengths=lengths, init='spsi')
    now = np.random.get_state()
    assert state[0] == now[0] and np.array_equal(state[1], now[1]) and state[2:] == now[2:]
    want = t2v_hip.istft(mag, t2v_hip.spsi_phase(mag, lengths), lengths, stft.tables(mag.device))
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got.abs().max()) > 0 and not got[1, 39 * 256:].any()
    # iterating from the start runs, draws nothing, and differs from the start alone
    it = griffin_lim(mag, stft, 2, lengths=lengths, init='spsi', momentum=0.99)
    now = np.random.get_state()
    assert np.array_equal(state[1], now[1]) and state[2] == now[2]
    assert it.shape == got.shape and bool(torch.isfinite(it).all()) and not torch.equal(it, got)
    # init='random' is the call without the keyword
    np.random.seed(6)
    a = griffin_lim(mag, stft, 2, lengths=lengths)
    np.random.seed(6)
    b = griffin_lim(mag, stft, 2, lengths=lengths, init='random')
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_spectral_convergence_on_the_device(taco):
    from audio_processing import griffin_lim
    mag64 = np.abs(R.stft(R.tone(125)))
    mag = torch.from_numpy(mag64.astype(np.float32)).cuda()[None]
    y = griffin_lim(mag, taco.stft_fn, 0, init='spsi')[0].cpu().numpy()
    np.random.seed(0)
    y_rand = griffin_lim(mag, taco.stft_fn, 0)[0].cpu().numpy()
    sc, sc_ref, sc_rand = (R.spectral_convergence(v, mag64) for v in (y, S.start(mag64), y_rand))
    print("tone 125 Hz, 0 iterations: spectral convergence device %.5f, fp64 restatement %.5f, random start %.5f" % (sc, sc_ref, sc_rand))
    assert abs(sc - sc_ref) <= 0.01 * sc_ref, (sc, sc_ref)
    assert sc <= 0.25 * sc_rand, (sc, sc_rand)


def test_low_tones_stay_voiced_through_the_vocoder(taco):
    import t2v_hip
    from synthesizer import GriffinLimVocoder
    basis = taco.mel_basis.numpy()
    B64 = basis.astype(np.float64)
    pinv = np.linalg.pinv(B64)
    spsi, fast = GriffinLimVocoder.named('spsi', taco), GriffinLimVocoder.named('griffin_lim_fast', taco)
    for f in (70, 100, 125):
        m = B64 @ R.frame_magnitudes(R.tone(f))
        ref = S.voiced_share(Y.yin(S.start(R.nnls(m, basis, pinv, 100)))['f0'])
        mel = torch.from_numpy(np.log(np.maximum(m, 1e-5)).astype(np.float32)).cuda()[None]
        share = {}
        for name, voc in (('spsi', spsi), ('fast', fast)):
            np.random.seed(0)
            y = voc(mel)
            assert y.shape == (1, (mel.size(2) - 1) * 256)
            hz = t2v_hip.f0(y.contiguous(), [y.size(1)])[0].cpu().numpy()
            share[name] = S.voiced_share(hz)
        print("tone %d Hz: voiced share 'spsi' %.3f (fp64 chain %.3f), 'griffin_lim_fast' %.3f" % (f, share['spsi'], ref, share['fast']))
        assert share['spsi'] >= ref - 0.05, (f, share, ref)
        assert share['spsi'] >= share['fast'], (f, share)


def test_knobs_and_batch(taco):
    from synthesizer import GriffinLimVocoder
    basis = taco.mel_basis.numpy().astype(np.float64)
    mags = [0.05 * np.abs(R.stft(R.tone(f, 0.5)))[:, :n] for f, n in ((110.0, 32), (180.0, 21), (260.0, 9))]
    lengths = [m.shape[1] for m in mags]
    mel = torch.zeros(3, 80, max(lengths))
    for b, m in enumerate(mags):
        mel[b, :, :lengths[b]] = torch.from_numpy(np.log(np.maximum(basis @ m, 1e-5)).astype(np.float32))
    mel = mel.cuda()
    voc = GriffinLimVocoder(taco, init='spsi', n_iters=0, speed=0.8, pitch=2)
    rand = GriffinLimVocoder(taco, n_iters=0, speed=0.8, pitch=2)
    state = np.random.get_state()
    got = voc.batch(mel, lengths)
    now = np.random.get_state()
    assert np.array_equal(state[1], now[1]) and state[2] == now[2]
    np.random.seed(1)
    want_counts = [w.numel() for w in rand.batch(mel, lengths)]
    assert [g.numel() for g in got] == want_counts
    for b in (2, 0, 1):                                    # no draws: the order of the calls does not matter
        alone = voc(mel[b:b + 1, :, :lengths[b]].contiguous())
        assert alone.shape == (1, want_counts[b]), b
        assert torch.equal(alone[0].view(torch.int32), got[b].view(torch.int32)), b
        assert float(got[b].abs().max()) > 0
