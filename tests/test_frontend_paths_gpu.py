"""Every path of k_mel_frontend (csrc/frontend.hip) against the fp64 reference of tests/frontend_ref.py, at round-off scale.

(a) parity, bank by bank: seven filterbanks, four that take the LDS-tap mel loop and three that take the CSR loop
    (registers_path is asserted per bank, so both loops are known to run), one ragged batch (lengths 513, 767 | 768, 1025, 1537,
    3584 | 3840 | 4096 for T = 15 | 16 | 17, and 20 * 1024 + 1 for interior frames), signals noise, steptone, halfbin, clicks,
    faint; each row over its own T_b, exactly 0.0 past it, the same bits on a second run;
(b) a stepped tone that visits every bin 1 .. 511;
(c) the paired-load path and the general load path give the same bits: N even, N odd (odd rows leave the paired path), and
    each row alone at B = 1, float32 and int16;
(d) int16 with scale 2^-15 equals float input int16 / 32768 bit for bit; scale 1 / 32767 passes compare();
(e) pad columns are never read; (f) t_stride above and below T_max, and the C entry point writing into the middle of a
    NaN-filled buffer; (g) silence and a full-scale square wave; (h) refused calls launch nothing;
(i) the device results against a MUTATED fp64 reference must FAIL by at least 10 bounds — nothing in the kernel is altered.

The metric and the bound (K = 16) are in tests/frontend_ref.py; no entry of any comparison is left out.  Every case prints
its worst entry next to floor and bound before it asserts (pytest -s); profiles/frontend_parity.txt is that table from an
MI355X.  The kernel's error in this metric on a device was unknown before that table.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_ref as R

pytestmark = pytest.mark.gpu

LENS = R.LENS
PARITY_SIGNALS = ('noise', 'steptone', 'halfbin', 'clicks', 'faint')
LOG_CLAMP = np.float32(np.log(np.float32(1e-5)))

_STFT, _CASE, _OUT = {}, {}, {}


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    _STFT.clear()
    _CASE.clear()
    _OUT.clear()


def _stft(bank):
    import layers
    if bank not in _STFT:
        _STFT[bank] = layers.TacotronSTFT(1024, 256, 1024, 80, *bank[:3])
    return _STFT[bank]


def _case(bank, sig):
    """the fp64 reference, floor and bounds of (bank, signal) on the ragged batch: computed once, shared, never modified"""
    if (bank, sig) not in _CASE:
        _CASE[bank, sig] = R.case(_stft(bank).mel_basis, sig)
    return _CASE[bank, sig]


def _run(bank, wav, lens, scale=1.0):
    import t2v_hip
    out = _stft(bank).mel_spectrogram(wav.cuda(), lengths=torch.tensor(lens), scale=scale)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    return out.cpu()


def _device(bank, sig):
    if (bank, sig) not in _OUT:
        _OUT[bank, sig] = _run(bank, _case(bank, sig).wav, LENS)
    return _OUT[bank, sig]


def _judge(title, c, out, mutation=None):
    ratio, err, bnd, where = c.judge(out, mutation)
    print('%s err %.2e floor %.2e K 16 bound %.2e err / bound %.3g at %s' % (title, err, c.floor, bnd, ratio, where))
    return ratio


def _zero_past(out, lens):
    for b, n in enumerate(lens):
        T = n // 256 + 1
        if T < out.shape[2]:
            assert float(out[b, :, T:].abs().max()) == 0.0, b


def _int16(wav):
    return torch.round(wav * 32767.0).to(torch.int16)


# ------------------------------------------------------------------------------------------------ (a) parity, bank by bank
@pytest.mark.parametrize("sig", PARITY_SIGNALS)
@pytest.mark.parametrize("bank", R.BANKS, ids=R.bank_name)
def test_parity_bank_by_bank(bank, sig):
    assert R.registers_path(_stft(bank)) is bank[3]         # which mel loop this bank runs
    c = _case(bank, sig)
    out = _device(bank, sig)
    assert out.shape == (len(LENS), 80, max(LENS) // 256 + 1)
    ratio = _judge('frontend parity %-13s %-4s %-8s' % (R.bank_name(bank), 'regs' if bank[3] else 'csr', sig), c, out)
    assert ratio < 1
    _zero_past(out, LENS)
    assert torch.equal(out, _run(bank, c.wav, LENS))        # a second run has the same bits


def test_both_mel_loops_ran():
    assert [b[3] for b in R.BANKS].count(False) == 3 and [b[3] for b in R.BANKS].count(True) == 4
    assert all(R.registers_path(_stft(b)) is b[3] for b in R.BANKS)


# ------------------------------------------------------------------------------------------------ (b) every bin
def test_a_stepped_tone_over_every_bin():
    """B = 7 rows of 73 one-segment tones: bins 1 .. 511, each on its own 1024 samples (tests/test_frontend_ref.py)"""
    lens = (73 * 1024,) * 7
    c = R.Case(_stft(R.DEFAULT_BANK).mel_basis, R.batch('steptone', lens, k0_step=73), lens)
    out = _run(R.DEFAULT_BANK, c.wav, lens)
    assert _judge('frontend parity %-13s regs all-bins' % R.bank_name(R.DEFAULT_BANK), c, out) < 1


# ------------------------------------------------------------------------------------------------ (c) the two load paths
@pytest.mark.parametrize("dtype", ['float32', 'int16'])
@pytest.mark.parametrize("sig", ['noise', 'steptone'])
def test_load_paths_agree_bit_for_bit(sig, dtype):
    """an interior frame takes the paired loads only when b * N + base is even: with N odd every odd row takes the general
    path for all its frames (the 20 * 1024 + 1 row sits in row 1).  Both form sample * scale * window in the same order."""
    N = max(LENS) + 1
    assert N % 2 == 0 and LENS[1] == max(LENS)
    conv, scale = (_int16, 1.0 / 32767.0) if dtype == 'int16' else ((lambda w: w), 1.0)
    even = conv(R.batch(sig, LENS, N=N, k0_step=57))
    odd = torch.cat((even, torch.zeros(len(LENS), 1, dtype=even.dtype)), 1)
    a, b = _run(R.DEFAULT_BANK, even, LENS, scale), _run(R.DEFAULT_BANK, odd, LENS, scale)
    assert a.shape == b.shape
    for r, n in enumerate(LENS):
        T = n // 256 + 1
        assert torch.equal(a[r], b[r]), (r, n)
        alone = _run(R.DEFAULT_BANK, even[r:r + 1, :n].contiguous(), (n,), scale)
        assert alone.shape == (1, 80, T) and torch.equal(alone[0], a[r, :, :T]), (r, n)


# ------------------------------------------------------------------------------------------------ (d) int16
def test_int16_with_a_power_of_two_scale_equals_float():
    pcm = _int16(R.batch('noise', LENS))
    a = _run(R.DEFAULT_BANK, pcm, LENS, 1.0 / 32768.0)
    b = _run(R.DEFAULT_BANK, pcm.float() / 32768.0, LENS)
    assert torch.equal(a, b)


@pytest.mark.parametrize("bank", [R.DEFAULT_BANK, R.FALLBACK_BANK], ids=R.bank_name)
def test_int16_with_scale_1_over_32767_passes(bank):
    pcm = _int16(R.batch('noise', LENS))
    s = float(np.float32(1.0 / 32767.0))                    # the value the kernel multiplies by
    c = R.Case(_stft(bank).mel_basis, pcm.double() * s, LENS)
    out = _run(bank, pcm, LENS, 1.0 / 32767.0)
    assert _judge('frontend parity %-13s %-4s int16 noise' % (R.bank_name(bank), 'regs' if bank[3] else 'csr'), c, out) < 1
    _zero_past(out, LENS)


# ------------------------------------------------------------------------------------------------ (e) pad columns
@pytest.mark.parametrize("dtype", ['float32', 'int16'])
def test_pad_columns_are_never_read(dtype):
    N = max(LENS) + 3
    wav = R.batch('noise', LENS, N=N)
    fill = (1.0 - 2.0 * (torch.arange(N) % 2).float())[None, :].expand(len(LENS), N)        # alternating +-1: legal samples
    past = torch.arange(N)[None, :] >= torch.tensor(LENS)[:, None]
    dirty = torch.where(past, fill, wav)
    assert float(dirty[0, LENS[0]:].abs().min()) == 1.0
    if dtype == 'int16':
        wav, dirty, scale = _int16(wav), _int16(dirty), 1.0 / 32767.0
        assert int(dirty[0, LENS[0]:].abs().min()) == 32767
    else:
        scale = 1.0
    assert torch.equal(_run(R.DEFAULT_BANK, wav, LENS, scale), _run(R.DEFAULT_BANK, dirty, LENS, scale))


# ------------------------------------------------------------------------------------------------ (f) t_stride
def _frontend(bank, wav, lens, t_stride):
    import t2v_hip
    dev = torch.device('cuda:0')
    out = t2v_hip.mel_frontend(wav.to(dev), torch.tensor(lens), _stft(bank)._tables(dev), 1.0, t_stride=t_stride)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    return out.cpu()


def test_t_stride_above_and_below_T_max():
    c = _case(R.DEFAULT_BANK, 'noise')
    plain = _device(R.DEFAULT_BANK, 'noise')
    T_max = plain.shape[2]
    for extra in (5, 16, 17):                               # 17: a whole workgroup beyond every utterance
        out = _frontend(R.DEFAULT_BANK, c.wav, LENS, T_max + extra)
        assert out.shape == (len(LENS), 80, T_max + extra)
        assert torch.equal(out[:, :, :T_max], plain), extra
        _zero_past(out, LENS)
    for t_stride in (T_max - 1, 1):
        out = _frontend(R.DEFAULT_BANK, c.wav, LENS, t_stride)
        assert out.shape == (len(LENS), 80, t_stride) and torch.equal(out, plain[:, :, :t_stride]), t_stride


def _abi_args(bank, wav, lens, out, t_stride, **over):
    """the argument list of t2v_mel_frontend as t2v_hip.mel_frontend forms it; `over` replaces arguments by name"""
    import t2v_hip
    t = _stft(bank)._tables(wav.device)
    p = t2v_hip._p
    n = torch.tensor(lens, dtype=torch.int64, device=wav.device)
    args = dict(wav_f32=p(wav), wav_i16=None, n_samples=p(n), B=wav.shape[0], n_stride=wav.shape[1], scale=1.0, n_fft=1024,
                hop=256, n_mel=80, window=p(t['window']), tw512=p(t['tw512']), tw1024=p(t['tw1024']), mel_start=p(t['mel_start']),
                mel_len=p(t['mel_len']), mel_w=p(t['mel_w']), maxw=int(t['maxw']), mel_out=p(out), t_stride=t_stride,
                stream=t2v_hip._stream())
    assert set(over) <= set(args)
    args.update(over)
    return list(args.values()), n            # (n is returned to keep it alive across the call)


def test_the_c_entry_point_writes_only_its_output():
    import t2v_hip
    lib = t2v_hip.load_library()
    dev = torch.device('cuda:0')
    c = _case(R.DEFAULT_BANK, 'noise')
    wav = c.wav.to(dev)
    T_max = max(LENS) // 256 + 1
    size, guard = len(LENS) * 80 * T_max, 4096
    buf = torch.full((guard + size + guard,), float('nan'), device=dev)
    args, keep = _abi_args(R.DEFAULT_BANK, wav, LENS, buf[guard:guard + size], T_max)
    assert lib.t2v_mel_frontend(*args) == 0
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    host = buf.cpu()
    assert bool(torch.isnan(host[:guard]).all()) and bool(torch.isnan(host[guard + size:]).all())
    assert torch.equal(host[guard:guard + size].view(len(LENS), 80, T_max), _device(R.DEFAULT_BANK, 'noise'))


# ------------------------------------------------------------------------------------------------ (g) silence, full scale
@pytest.mark.parametrize("bank", [R.DEFAULT_BANK, R.FALLBACK_BANK], ids=R.bank_name)
def test_silence_is_the_clamp_on_both_mel_loops(bank):
    assert R.registers_path(_stft(bank)) is bank[3]
    out = _run(bank, R.batch('silence', LENS), LENS)
    worst = max(float((out[b, :, :n // 256 + 1] - LOG_CLAMP).abs().max()) for b, n in enumerate(LENS))
    print('frontend silence %-13s %-4s largest |out - log(1e-5)| %.3g ulps of an fp32 in [8, 16)'
          % (R.bank_name(bank), 'regs' if bank[3] else 'csr', worst * 2.0 ** 20))
    assert worst <= 2.0 ** -20
    _zero_past(out, LENS)


@pytest.mark.parametrize("bank", [R.DEFAULT_BANK, R.FALLBACK_BANK], ids=R.bank_name)
def test_a_full_scale_square_wave_passes(bank):
    c = _case(bank, 'square')
    assert float(c.wav[1].abs().min()) == 1.0
    assert _judge('frontend parity %-13s %-4s square  ' % (R.bank_name(bank), 'regs' if bank[3] else 'csr'), c, _device(bank, 'square')) < 1


# ------------------------------------------------------------------------------------------------ (h) refusals
def test_a_refused_call_launches_nothing():
    import t2v_hip
    lib = t2v_hip.load_library()
    dev = torch.device('cuda:0')
    lens = (1537, 1025)
    wav = R.batch('noise', lens).to(dev)
    tables = _stft(R.DEFAULT_BANK)._tables(dev)
    with pytest.raises(ValueError):
        t2v_hip.mel_frontend(wav, torch.tensor([1537, 512]), tables)            # reflect padding needs more than 512 samples
    with pytest.raises(ValueError):
        t2v_hip.mel_frontend(wav, torch.tensor([1538, 1025]), tables)           # n > N
    with pytest.raises(ValueError):
        _stft(R.DEFAULT_BANK).mel_spectrogram(wav, lengths=torch.tensor([1537, 512]))
    T_max = 7
    out = torch.full((2, 80, T_max), float('nan'), device=dev)
    for over in (dict(n_fft=512), dict(hop=128), dict(n_mel=64), dict(mel_out=None), dict(B=0)):
        args, keep = _abi_args(R.DEFAULT_BANK, wav, lens, out, T_max, **over)
        assert lib.t2v_mel_frontend(*args) != 0, over
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), over
    t2v_hip.check_async_errors()
    # and the same arguments, un-refused, do write it
    args, keep = _abi_args(R.DEFAULT_BANK, wav, lens, out, T_max)
    assert lib.t2v_mel_frontend(*args) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ (i) mutations must fail
@pytest.mark.parametrize("mutation,bank,sig", R.MUTATED, ids=R.MUTATED_IDS)
def test_a_mutated_reference_is_seen(mutation, bank, sig):
    """CPU-side mutations of the REFERENCE: against each the unmutated kernel's output is at least 10 bounds out"""
    if sig == 'tone':
        c = R.mutation_case(_stft(bank).mel_basis, mutation, sig)
        out = _run(bank, c.wav, c.lens)
        assert _judge('frontend parity %-13s %-4s tone on bin %d' % (R.bank_name(bank), 'regs' if bank[3] else 'csr',
                                                                    R.tap_bin(c.bank, mutation)[1]), c, out) < 1
    else:
        c, out = _case(bank, sig), _device(bank, sig)
    ratio = _judge('frontend mutation %-9s %-13s %-8s' % (mutation, R.bank_name(bank), sig), c, out, mutation)
    assert ratio >= 10
    print('mutation asserted on %s %s %s: err / bound %.3g' % (mutation, R.bank_name(bank), sig, ratio))
