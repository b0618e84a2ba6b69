"""tests/ema_ref.py against itself (no GPU): the fp64 oracle against closed forms, and the numpy fp32 emulation against the
oracle on the very cases of the GPU tests and on the longer trial; every figure ema_ref.EMUL records is re-measured here, so
K_EMA stays what the emulation says and never what a kernel gives."""
import math

import numpy as np
import pytest
import torch

import adam_ref as A
import ema_ref as R

SIZES = (1, 3, 4, 7, A.CLIP_SWEEP + 4, 2 * A.CLIP_SWEEP + 3075)
REGIMES = ('active_late_wd', 'active_first')


def test_rate_is_rounded_once_from_the_double():
    r = R.rate32(0.9999)
    assert r == float(np.float32(1e-4)) and abs(r - 1e-4) < 1e-4 * 2.0 ** -24
    lazy = float(np.float32(1.0) - np.float32(0.9999))            # 1 - fp32(0.9999): what the kernel must NOT run at
    assert 1.5e-4 < abs(lazy - 1e-4) / 1e-4 < 1.8e-4
    assert R.rate32(0.5) == 0.5 and R.rate32(0.0) == 1.0


def test_warmup_is_tensorflows_decay_written_as_a_rate():
    for t in (0, 1, 5, 89989, 89990, 89991, 10 ** 6):
        tf_decay = min(0.9999, (1.0 + t) / (10.0 + t))
        assert abs((1.0 - R.rate_t(R.rate32(0.9999), True, t)) - tf_decay) < 1e-11
        assert R.rate_t(0.25, False, t) == 0.25
    assert R.rate_t(R.rate32(0.9999), True, 0) == 0.9 and R.rate_t(R.rate32(0.9999), True, 10 ** 6) == R.rate32(0.9999)


def test_oracle_follows_the_closed_form_on_constant_weights():
    gen = torch.Generator().manual_seed(5)
    p, s0 = torch.randn(1000, generator=gen).float(), torch.randn(1000, generator=gen).float()
    rate = R.rate32(0.99)
    s = s0.double()
    for t in range(50):
        s, sc = R.ema_ref(s, p, rate, False, t)
        assert bool((sc >= s.abs() - 1e-12).all())
    want = p.double() + (1.0 - rate) ** 50 * (s0.double() - p.double())
    assert float((s - want).abs().max()) < 1e-13
    s1, _ = R.ema_ref(s0, p, rate, True, 0)                      # first warm-up update: nine tenths of the way
    assert float((s1 - (0.1 * s0.double() + 0.9 * p.double())).abs().max()) < 1e-15
    assert s0.dtype == torch.float32 and p.dtype == torch.float32            # the inputs are left alone


def test_worst_ratio_reads_as_the_bound_does():
    ref, scale = torch.tensor([1.0, 2.0], dtype=torch.float64), torch.tensor([1.0, 4.0], dtype=torch.float64)
    got = ref + torch.tensor([3.0, -8.0], dtype=torch.float64) * R.EPS32
    assert R.worst_ratio(got, ref, scale) == 3.0 and R.worst_ratio(got, ref, scale, t=2) == 1.5
    assert R.worst_ratio(ref, ref, torch.zeros(2)) == 0.0 and R.worst_ratio(got, ref, torch.zeros(2)) == float('inf')
    assert R.worst_ratio(torch.tensor([float('nan'), 2.0]), ref, scale) == float('inf')
    assert float(R.bound(scale, 3)[1]) == R.K_EMA * 3 * R.EPS32 * 4.0


_P_NEW = {}


def _p_new(n, regime):
    """the fp32 weights a step of the case leaves (adam_ref's fp32 emulation of the kernel)"""
    if (n, regime) not in _P_NEW:
        p, g, m, v, h = A.kernel_case(n, regime)
        _P_NEW[(n, regime)] = (p, A.clip_adam_emul32(p, g, m, v, **h)[0])
    return _P_NEW[(n, regime)]


def test_emulation_of_the_single_step_cases_stays_within_its_recorded_figure():
    worst = 0.0
    rate = R.rate32(R.DECAY)
    for n in SIZES:
        for regime in REGIMES:
            p0, p1 = _p_new(n, regime)
            s0 = R.shadow_for(p0)
            for warmup, t in R.STEP_CASES:
                ref, scale = R.ema_ref(s0, p1, rate, warmup, t)
                got = R.ema_emul32(s0.numpy(), p1.numpy(), rate, warmup, t)
                assert got.dtype == np.float32
                worst = max(worst, R.worst_ratio(torch.from_numpy(got), ref, scale))
    print('single step: emulation worst ratio %.3f' % worst)
    assert 0.0 < worst <= R.EMUL['step']


@pytest.mark.parametrize('no_grad', [False, True])
def test_emulation_along_the_toy_trajectories_stays_within_its_recorded_figure(no_grad):
    """the shadow of adam_ref's fp32 Adam trajectory: decay 0.99 with warm-up and 0.9999 without, 20 steps"""
    steps = list(A.flat_adam_emul32(A.toy_params(), A.toy_grads(no_grad=no_grad), lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0))
    weights = [torch.cat([t.reshape(-1) for t in st[0]]).float() for st in steps]
    start = torch.cat([t.reshape(-1) for t in A.toy_params()]).float()
    worst = max(R.trajectory_ratio(weights, 0.99, True, s0=start), R.trajectory_ratio(weights, 0.9999, False, s0=start))
    print('toy no_grad=%s: emulation worst ratio %.3f' % (no_grad, worst))
    assert 0.0 < worst <= R.EMUL['toy']


@pytest.mark.parametrize('warmup', [False, True])
def test_emulation_of_the_long_trial_stays_within_its_recorded_figure(warmup):
    weights = R.trial_weights(70001, 200)
    worst = max(R.trajectory_ratio(weights, d, warmup) for d in (0.5, 0.99, 0.9999))
    print('trial warmup=%s: emulation worst ratio %.3f' % (warmup, worst))
    assert 0.0 < worst <= R.EMUL['trial_warmup' if warmup else 'trial']


def test_k_is_twice_the_worst_recorded_figure():
    assert R.K_EMA == 2.0 * max(R.EMUL.values()) and set(R.EMUL) == {'step', 'toy', 'trial', 'trial_warmup'}
    assert math.isfinite(R.K_EMA) and R.K_EMA >= 2.0
