"""t2v_hip.f0 (csrc/f0.hip) against the fp64 numpy YIN of tests/yin_ref.py: values, determinism, non-default ranges, the
three containers of the lengths, and the errors.

Tolerances (derived, not measured).  Every d and every running sum of d is a sum of at most W + tau_max non-negative fp32
terms, so |d' - ref| <= eta d' with eta = (W + tau_max + 8) 2^-23 (1.5e-4 for the default range), twice the first-order
bound.  Voicing and the lag must equal the reference's on every compared frame and the aperiodicity lies within eta
relative.  The partial derivatives of delta in a, b, c = d'(tau - 1 .. tau + 1) are each at most 1 / den in magnitude
(den = a - 2b + c), so |f0 - ref| / f0 <= 6 eta max(a, b, c) / (den tau); without a parabola (a neighbour outside the lag
range) f0 = 16000 / tau in both, up to the fp32 quotient.
A frame is not compared where the decision, not the arithmetic, is in doubt: where the reference's margin (the smallest
distance of a d' from the threshold, or between two neighbours in the descent) is below 1e-4, the error bound on d' near the
threshold being 1.5e-5, or where den < 1e-3.  At most 5 % of a case's frames (one seeded batch) may be left out.

Rows: the lengths 1, 255, 256, 257, 1023, 1024, 1291 (= W + tau_max), 4096, 24000 twice, and 2900 / 3100 / 3400 samples =
12 / 13 / 14 frames around the 13 frames a workgroup owns, all of yin_ref.glide_signal's recipe, whose silent and noise-only
stretches cover most of a short row; so the short lengths appear once more as the plain start of a long glide.  One batch of
stride 24003, NaN past each length."""
import functools

import numpy as np
import pytest
import torch

import yin_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 255, 256, 257, 1023, 1024, 1291, 4096, 24000, 24000, 2900, 3100, 3400]
PLAIN = [1023, 1024, 1291, 2900, 3100, 3400, 4096]          # the same lengths again, voiced throughout
STRIDE = 24003
SEEDS = (0, 1, 2)


def _eta(tau_max):
    return (yin_ref.W + tau_max + 8) * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _batch(seed):
    """(y (B, STRIDE) with NaN past each length, lengths): row b's signal is seeded by (seed, b)"""
    lengths = LENGTHS + PLAIN
    y = torch.full((len(lengths), STRIDE), float('nan'))
    for b, n in enumerate(lengths):
        if b < len(LENGTHS):
            x = yin_ref.glide_signal(n, 100 * seed + b)
        else:
            x = yin_ref.harmonic_tone(110.0, 24000, harmonics=6, amp=0.2, phase_seed=seed)[:n].astype(np.float32)
            x = x + (0.003 * np.random.RandomState(1000 + 100 * seed + b).randn(n)).astype(np.float32)
        y[b, :n] = torch.from_numpy(x)
    return y, lengths


@functools.lru_cache(maxsize=None)
def _reference(seed, fmin=60.0, fmax=500.0, threshold=0.1):
    y, lengths = _batch(seed)
    return [yin_ref.yin(y[b, :n].numpy(), fmin, fmax, threshold) for b, n in enumerate(lengths)]


def _compare(hz, ap, refs, lengths, tau_max, what):
    """asserts the tolerances of the module docstring on every compared frame; returns (frames, excluded, voiced)"""
    eta = _eta(tau_max)
    hz, ap = hz.cpu().double().numpy(), ap.cpu().double().numpy()
    total = excluded = voiced = 0
    worst_ap = worst_f0 = 0.0
    for b, (n, r) in enumerate(zip(lengths, refs)):
        T = n // 256 + 1
        assert len(r['f0']) == T
        assert (hz[b, T:] == 0).all() and (ap[b, T:] == 1).all(), (what, b, "padding past the row's frames must be 0 / 1")
        for t in range(T):
            total += 1
            if r['margin'][t] < 1e-4 or (r['tau'][t] > 0 and np.isfinite(r['den'][t]) and r['den'][t] < 1e-3):
                excluded += 1
                continue
            if r['tau'][t] == 0:
                assert hz[b, t] == 0 and ap[b, t] == 1, (what, b, t, hz[b, t], ap[b, t])
                continue
            voiced += 1
            assert hz[b, t] > 0, (what, b, t, "voiced in the reference", r['f0'][t])
            tau = int(r['tau'][t])
            assert abs(ap[b, t] - r['aperiodicity'][t]) <= eta * r['aperiodicity'][t], (what, b, t, ap[b, t], r['aperiodicity'][t])
            if np.isfinite(r['den'][t]):
                bound = 6 * eta * max(r['a'][t], r['b'][t], r['c'][t]) / (r['den'][t] * tau)
            else:
                bound = 2.0 ** -23
            rel = abs(hz[b, t] - r['f0'][t]) / r['f0'][t]
            # a lag other than the reference's moves f0 by at least 1 / (tau + 2) relative, far outside the bound
            assert rel <= bound, (what, b, t, hz[b, t], r['f0'][t], rel, bound, tau)
            assert round(16000.0 / hz[b, t]) in (tau - 1, tau, tau + 1)
            worst_f0 = max(worst_f0, rel / bound)
            if r['aperiodicity'][t] > 0:
                worst_ap = max(worst_ap, abs(ap[b, t] - r['aperiodicity'][t]) / (eta * r['aperiodicity'][t]))
    print("%s: %d frames, %d voiced, %d excluded (%.1f %%), worst f0 err / bound %.3f, worst aperiodicity err / bound %.3f"
          % (what, total, voiced, excluded, 100.0 * excluded / total, worst_f0, worst_ap))
    assert excluded <= 0.05 * total, (what, excluded, total)
    return total, excluded, voiced


@pytest.mark.parametrize("seed", SEEDS)
def test_batch_matches_fp64(seed):
    import t2v_hip
    y, lengths = _batch(seed)
    hz, ap = t2v_hip.f0(y.cuda(), lengths, return_aperiodicity=True)
    assert hz.shape == ap.shape == (len(lengths), 24000 // 256 + 1)
    refs = _reference(seed)
    total, excluded, voiced = _compare(hz, ap, refs, lengths, 267, "seed %d" % seed)
    assert voiced >= 0.3 * total
    long_ref = refs[8]
    print("seed %d, 24000 samples: %d of %d frames voiced in the reference" % (seed, (long_ref['tau'] > 0).sum(), len(long_ref['tau'])))
    z0 = 24000 // 6
    silent = [t for t in range(len(long_ref['tau'])) if 256 * t - 512 >= z0 and 256 * t + 512 + 267 <= z0 + 3000]
    assert silent and all(float(hz[8, t]) == 0 and float(ap[8, t]) == 1 for t in silent)      # digital silence: unvoiced


def test_each_row_alone_and_twice_gives_the_same_bits():
    import t2v_hip
    y, lengths = _batch(0)
    hz, ap = t2v_hip.f0(y.cuda(), lengths, return_aperiodicity=True)
    again = t2v_hip.f0(y.cuda(), lengths, return_aperiodicity=True)
    assert again[0].cpu().numpy().tobytes() == hz.cpu().numpy().tobytes()
    assert again[1].cpu().numpy().tobytes() == ap.cpu().numpy().tobytes()
    hz, ap = hz.cpu(), ap.cpu()
    for b, n in enumerate(lengths):
        # alone, cut to its own length: another stride, no padding, another place in the grid
        h1, a1 = t2v_hip.f0(y[b:b + 1, :n].contiguous().cuda(), [n], return_aperiodicity=True)
        T = n // 256 + 1
        assert h1.shape == (1, T)
        assert h1.cpu().numpy().tobytes() == hz[b:b + 1, :T].contiguous().numpy().tobytes(), (b, n)
        assert a1.cpu().numpy().tobytes() == ap[b:b + 1, :T].contiguous().numpy().tobytes(), (b, n)
    # a sub-batch in another order
    pick = [9, 3, 12, 8]
    h2 = t2v_hip.f0(y[pick].cuda(), [lengths[b] for b in pick]).cpu()
    assert h2.numpy().tobytes() == hz[pick].contiguous().numpy().tobytes()


@pytest.mark.parametrize("fmin,fmax,threshold", [(80.0, 400.0, 0.15), (40.0, 1000.0, 0.1)])
def test_non_default_range_matches_fp64(fmin, fmax, threshold):
    import t2v_hip
    y, lengths = _batch(1)
    hz, ap = t2v_hip.f0(y.cuda(), lengths, fmin, fmax, threshold, return_aperiodicity=True)
    tau_max = yin_ref.lags(fmin, fmax)[1]
    assert tau_max == t2v_hip.f0_lags(fmin, fmax)[1]
    _compare(hz, ap, _reference(1, fmin, fmax, threshold), lengths, tau_max, "fmin %g fmax %g threshold %g" % (fmin, fmax, threshold))


def test_steady_tones_on_the_device():
    """the four tones of tests/test_prosody.py through the kernel, within the bound asserted of the reference there"""
    import t2v_hip
    from test_prosody import TONE_BOUND, TONES
    y = torch.stack([torch.from_numpy(yin_ref.harmonic_tone(f, 12000).astype(np.float32)) for f in TONES])
    hz = t2v_hip.f0(y.cuda(), [12000] * len(TONES)).cpu().double().numpy()
    for b, f in enumerate(TONES):
        inner = hz[b, 3:-3]
        print("%.1f Hz: max rel err %.3e" % (f, np.abs(inner / f - 1).max()))
        assert (inner > 0).all() and np.abs(inner / f - 1).max() <= TONE_BOUND


def test_length_containers_agree():
    import t2v_hip
    y, lengths = _batch(2)
    yd = y.cuda()
    a = t2v_hip.f0(yd, lengths).cpu()
    b = t2v_hip.f0(yd, torch.tensor(lengths)).cpu()
    c = t2v_hip.f0(yd, torch.tensor(lengths, dtype=torch.int32).cuda()).cpu()
    assert a.numpy().tobytes() == b.numpy().tobytes() == c.numpy().tobytes()


def test_errors_leave_the_library_usable():
    import t2v_hip
    y, lengths = _batch(0)
    yd = y[:3].contiguous().cuda()
    n3 = lengths[:3]
    good = t2v_hip.f0(yd, n3, return_aperiodicity=True)
    for bad in (dict(lengths=[0, 255, 256]), dict(lengths=[1, 255, STRIDE + 1]), dict(lengths=[1, 255]),
                dict(lengths=[1.0, 255.0, 256.0]), dict(fmin=39.0), dict(fmax=1001.0), dict(fmin=500.0, fmax=500.0),
                dict(fmin=300.0, fmax=200.0), dict(threshold=0.0), dict(threshold=1.0)):
        kw = dict(lengths=n3)
        kw.update(bad)
        with pytest.raises(ValueError, match=r"\d"):
            t2v_hip.f0(yd, **kw)
    with pytest.raises(ValueError):
        t2v_hip.f0(yd[0], [1])                                                  # not (B, S)
    with pytest.raises(ValueError):
        t2v_hip.f0(yd.double(), n3)
    lib = t2v_hip.load_library()
    n = torch.tensor(n3, dtype=torch.int32).cuda()
    T = STRIDE // 256 + 1
    hz, ap = torch.zeros(3, T).cuda(), torch.zeros(3, T).cuda()
    args = lambda tau_min, tau_max, out_stride, B=3: (t2v_hip._p(yd), t2v_hip._p(n), STRIDE, B, tau_min, tau_max, 0.1,
                                                      t2v_hip._p(hz), t2v_hip._p(ap), out_stride, t2v_hip._stream())
    assert lib.t2v_f0_yin(*args(32, 401, T)) == -1                              # T2V_ERR_DIMS: tau_max > T2V_F0_MAX_LAG
    assert lib.t2v_f0_yin(*args(0, 267, T)) == -1
    assert lib.t2v_f0_yin(*args(267, 267, T)) == -1
    assert lib.t2v_f0_yin(*args(32, 267, T - 1)) == -2                          # T2V_ERR_ARG: out_stride < y_stride / 256 + 1
    assert lib.t2v_f0_yin(*args(32, 267, T, B=0)) == -2
    assert lib.t2v_f0_yin(t2v_hip._p(yd), None, STRIDE, 3, 32, 267, 0.1, t2v_hip._p(hz), t2v_hip._p(ap), T, t2v_hip._stream()) == -2
    assert lib.t2v_f0_yin(*args(32, 267, T)) == 0
    torch.cuda.synchronize()
    assert hz[:, :good[0].size(1)].cpu().numpy().tobytes() == good[0].cpu().numpy().tobytes()
    after = t2v_hip.f0(yd, n3, return_aperiodicity=True)
    assert after[0].cpu().numpy().tobytes() == good[0].cpu().numpy().tobytes()
    assert after[1].cpu().numpy().tobytes() == good[1].cpu().numpy().tobytes()
    t2v_hip.check_async_errors()
