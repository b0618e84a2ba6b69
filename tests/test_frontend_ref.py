"""The front-end reference of tests/frontend_ref.py against itself and against what the repository already trusts: no GPU.
These are the conditions that make the bounds of tests/test_frontend_paths_gpu.py mean something:

  - in fp64 its spectrum is a dense 1024-point DFT matrix product, to 1e-12 of the frame's 1-norm;
  - the mels the reference implementation recorded (tests/golden/mel_frontend.npz: speech, noise) pass compare(): the
    reference is that implementation's operation, not merely a plausible one;
  - oracle/t2v_oracle.mel_spectrogram (fp32) passes compare() on noise;
  - every mutation stands at least 100 bounds (K = 16) above the reference on the cases the device test uses it on;
  - for each of the seven filterbanks the device test runs, registers_path() says which mel loop the kernel takes, and the
    CSR tables (start, len, rows) rebuild mel_basis exactly.

Every figure is printed (pytest -s)."""
import math
import os

import numpy as np
import pytest
import torch

import frontend_ref as R

F32, F64 = torch.float32, torch.float64
MARGIN = 100.0
LENS = R.LENS

_STFT = {}


def _stft(bank):
    import layers
    if bank not in _STFT:
        _STFT[bank] = layers.TacotronSTFT(1024, 256, 1024, 80, *bank[:3])
    return _STFT[bank]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    _STFT.clear()


def test_signals_are_seeded_and_in_range():
    for name in ('noise', 'steptone', 'halfbin', 'clicks', 'square', 'faint', 'silence'):
        a, b = R.signal(name, 4097, seed=3, k0=5), R.signal(name, 4097, seed=3, k0=5)
        assert torch.equal(a, b) and a.dtype == F32 and float(a.abs().max()) <= 1.0, name
    assert bool((R.signal('square', 999).abs() == 1).all()) and float(R.signal('silence', 999).abs().max()) == 0.0
    c = R.signal('clicks', 4000)
    assert sorted(torch.nonzero(c).flatten().tolist()) == [1, 511, 512, 4000 - 513, 4000 - 2]
    # steptone: B = 7 rows of 73 segments visit bins 1 .. 511, each once, and a segment sits ON its bin
    bins = [1 + (73 * b + j) % 511 for b in range(7) for j in range(73)]
    assert sorted(bins) == list(range(1, 512))
    x = R.signal('steptone', 73 * 1024, seed=2, k0=146)
    spec = torch.fft.rfft(x[5 * 1024:6 * 1024].double()).abs()
    assert int(spec.argmax()) == 1 + 146 + 5 and float(spec.sum() - spec.max()) < 1e-3 * float(spec.max())


def test_the_fp64_spectrum_is_a_dense_dft():
    i = torch.arange(1024, dtype=F64)
    ang = 2 * math.pi * (i[:, None] * torch.arange(513, dtype=F64)[None, :] % 1024) / 1024
    for name, n in (('noise', 1537), ('halfbin', 2048), ('clicks', 1025), ('square', 1300)):
        y = R.signal(name, n, seed=4)
        xw = R.frames(y, n, F64)
        dense = torch.sqrt((xw @ torch.cos(ang)) ** 2 + (xw @ torch.sin(ang)) ** 2).t()
        ref = R.mel(y, n, torch.eye(513)[:80], F64)
        err = float(((ref.mag - dense).abs() / xw.abs().sum(1)[None, :]).max())
        print('%s n %d: fp64 rfft magnitude minus dense DFT, largest / ||xw||_1: %.2e' % (name, n, err))
        assert ref.mag.shape == (513, n // 256 + 1) and err <= 1e-12
        # the frames themselves: reflect pad with the edge sample excluded, frame t starts at 256 t - 512
        yp = torch.nn.functional.pad(y.double()[None, None], (512, 512), mode='reflect')[0, 0]
        assert torch.equal(xw, yp.unfold(0, 1024, 256) * R.window(F64))
        assert torch.equal(ref.norm, xw.norm(dim=1))


def _golden_case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, 'mel_frontend.npz'))
    bank = torch.from_numpy(g['mel_basis'])
    wav = torch.from_numpy(g[name + '_wav']).float() / 32768.0
    return R.Case(bank, wav[None], (wav.numel(),)), torch.from_numpy(g[name + '_mel'])


@pytest.mark.parametrize("name", ['speech', 'noise'])
def test_the_recorded_reference_mels_pass(name, golden_dir):
    c, recorded = _golden_case(golden_dir, name)
    assert float((c.bank - _stft(R.DEFAULT_BANK).mel_basis).abs().max()) < 1e-7
    ratio, err, bnd, where = c.judge(recorded[None])
    of_scale = float(((torch.exp(recorded.double()) - c.ref[0].mel.clamp(min=R.CLAMP)).abs() / R.scale(c.bank, c.ref[0])).max())
    print('golden %s: err %.2e floor %.2e bound %.2e err / bound %.3g at %s; largest err / scale %.2e'
          % (name, err, c.floor, bnd, ratio, where, of_scale))
    assert ratio < 1


def test_the_fp32_oracle_passes_on_noise():
    import t2v_oracle as O
    bank = _stft(R.DEFAULT_BANK).mel_basis
    wav = R.batch('noise', LENS)
    c = R.Case(bank, wav, LENS)
    out = torch.zeros(len(LENS), 80, max(LENS) // 256 + 1)
    for b, n in enumerate(LENS):
        out[b, :, :n // 256 + 1] = O.mel_spectrogram(wav[b:b + 1, :n], mel_basis=bank)[0]
    ratio, err, bnd, where = c.judge(out)
    print('t2v_oracle.mel_spectrogram on noise: err %.2e floor %.2e bound %.2e err / bound %.3g at %s' % (err, c.floor, bnd, ratio, where))
    assert ratio < 1


@pytest.mark.parametrize("mutation,bank,sig", R.MUTATED, ids=R.MUTATED_IDS)
def test_every_mutation_stands_100_bounds_above_the_reference(mutation, bank, sig):
    """on the reference alone: log of the fp64 reference held against the mutated fp64 reference, under the device test's bound"""
    c = R.mutation_case(_stft(bank).mel_basis, mutation, sig)
    out = torch.zeros(len(c.lens), 80, max(c.lens) // 256 + 1, dtype=F64)
    for b, n in enumerate(c.lens):
        out[b, :, :n // 256 + 1] = torch.log(c.ref[b].mel.clamp(min=R.CLAMP))
    clean = c.judge(out)[0]
    ratio, err, bnd, where = c.judge(out, mutation)
    print('mutation %-9s %-14s %-8s moved %.2e floor %.2e bound %.2e ratio %.3g at %s (un-mutated: %.3g)'
          % (mutation, R.bank_name(bank), sig, err, c.floor, bnd, ratio, where, clean))
    assert clean < 1e-6 and ratio >= MARGIN
    assert c.floor < 2e-6           # the floor is at round-off: 100 bounds up is not 100 large floors up


def test_the_tap_mutations_name_the_taps_they_claim():
    basis = _stft(R.FALLBACK_BANK).mel_basis
    t = _stft(R.FALLBACK_BANK)._host_tables
    m, k = R.tap_bin(basis, 'tap21')
    assert m < 64 and t['mel_len'][m] >= 21 and k == t['mel_start'][m] + 20 and float(basis[m, k]) > 0
    m, k = R.tap_bin(basis, 'tap41')
    assert m >= 64 and t['mel_len'][m] >= 41 and k == t['mel_start'][m] + 40 and float(basis[m, k]) > 0
    basis = _stft(R.DEFAULT_BANK).mel_basis
    t = _stft(R.DEFAULT_BANK)._host_tables
    assert R.tap_bin(basis, 'tap_last') == (40, t['mel_start'][40] + t['mel_len'][40] - 1)
    assert R.tap_bin(basis, 'tap_first') == (70, t['mel_start'][70])
    with pytest.raises(ValueError):
        R.tap_bin(basis, 'tap21')               # no such tap in a bank of the registers path


# widest filter of lanes 0..63 and of 64..79, per bank
WIDTHS = {R.BANKS[0]: (20, 37), R.BANKS[1]: (14, 27), R.BANKS[2]: (19, 35), R.BANKS[3]: (7, 12),
          R.BANKS[4]: (21, 41), R.BANKS[5]: (21, 42), R.BANKS[6]: (22, 50)}


@pytest.mark.parametrize("bank", R.BANKS, ids=R.bank_name)
def test_filterbank_tables(bank):
    stft = _stft(bank)
    t = stft._host_tables
    start, ln, rows = t['mel_start'], t['mel_len'], t['mel_w']
    print('bank %s: widest filter of 0..63 %d, of 64..79 %d, maxw %d, registers path %s'
          % (R.bank_name(bank), ln[:64].max(), ln[64:].max(), stft._maxw, R.registers_path(stft)))
    assert (int(ln[:64].max()), int(ln[64:].max())) == WIDTHS[bank]
    assert R.registers_path(stft) is bank[3]
    assert rows.shape == (80, stft._maxw) and int(ln.max()) <= stft._maxw and int(ln.min()) >= 1
    assert int(start.min()) >= 0 and int((start + ln).max()) <= 513           # the CSR loop reads mag[start .. start + len)
    rebuilt = np.zeros((80, 513), dtype=np.float32)
    for m in range(80):
        rebuilt[m, start[m]:start[m] + ln[m]] = rows[m, :ln[m]]
        assert not rows[m, ln[m]:].any()
    assert np.array_equal(rebuilt, stft.mel_basis.numpy())


def test_three_banks_take_the_csr_loop():
    assert sum(1 for b in R.BANKS if not b[3]) == 3 and len(R.BANKS) == 7
