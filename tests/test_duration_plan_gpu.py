"""The length regulator on the device (t2v_hip.duration_plan, csrc/plan.hip) against the integer definition of
tests/plan_ref.py: exact equality at the symbol counts where the scan changes shape (one wave, one chunk of 256, the carry into
the next chunk, several chunks), at plan widths 1, 64 and 1000, ragged n_ids, fractional rates that hit the .5 ties, rows of
zeros and refused rows; and a row equals the same row run alone."""
import numpy as np
import pytest
import torch

import plan_ref as P

pytestmark = pytest.mark.gpu

SYMBOLS = (1, 63, 64, 65, 255, 256, 257, 560, 1025)
WIDTHS = (1, 64, 1000)


def _durations(B, S, seed):
    """quarters of a frame in 0 .. 3 (so sums of rates 0.5, 1.5, 2.5 land on .5 ties), one row of zeros when B > 1; ragged"""
    g = np.random.default_rng(seed)
    dur = (g.integers(0, 13, (B, S)) / 4).astype(np.float32)
    n_ids = [S] + [int(x) for x in g.integers(0, S + 1, B - 1)]
    if B > 1:
        dur[1] = 0
        n_ids[1] = S
        n_ids[B - 1] = max(1, S // 2)
    return dur, n_ids


def _run(dur, n_ids, T_max, rate=None):
    import t2v_hip
    d = torch.from_numpy(dur).cuda()
    r = torch.from_numpy(rate).cuda() if isinstance(rate, np.ndarray) else rate
    out = t2v_hip.duration_plan(d, n_ids, T_max, rate=r)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    return out.plan.cpu(), out.n_plan.cpu()


def _same(got, want):
    return torch.equal(got[0], torch.from_numpy(want[0])) and torch.equal(got[1], torch.from_numpy(want[1]))


@pytest.mark.parametrize("S", SYMBOLS)
def test_plan_equals_the_integer_definition(S):
    for B in (1, 5):
        dur, n_ids = _durations(B, S, 100 * S + B)
        per_symbol = (np.random.default_rng(S).integers(1, 7, (B, S)) / 2).astype(np.float32)      # 0.5 .. 3.0: .5 ties
        for T_max in WIDTHS:
            for rate in (None, 0.5, 1.5, per_symbol):
                got, want = _run(dur, n_ids, T_max, rate), P.regulate(dur, n_ids, T_max, rate)
                assert got[0].dtype == torch.int32 and got[0].shape == (B, T_max) and got[1].shape == (B,)
                assert _same(got, want), (S, B, T_max, rate if not isinstance(rate, np.ndarray) else 'per symbol')
            if B > 1:
                assert want[1][1] == 0 and not want[0][1].any()                    # the row of zeros: an empty plan
        # a row's output equals the same row run alone
        if B > 1:
            full = _run(dur, n_ids, 64, per_symbol)
            for b in range(B):
                one = _run(dur[b:b + 1], n_ids[b:b + 1], 64, per_symbol[b:b + 1])
                assert torch.equal(one[0][0], full[0][b]) and one[1][0] == full[1][b], (S, b)


def test_ties_and_truncation_as_the_reference_states_them():
    got = _run(np.full((1, 4), 0.5, np.float32), [4], 6)
    assert got[1].tolist() == [2] and got[0][0].tolist() == [0, 2, 2, 2, 2, 2]
    got = _run(np.array([[2.0 ** -17, 3 * 2.0 ** -17, 1.0]], np.float32), [3], 4)
    assert got[1].tolist() == [1] and got[0][0].tolist() == [2, 2, 2, 2]
    got = _run(np.full((1, 8), 2.0 ** 20, np.float32), [8], 5)                     # the largest admitted duration
    assert got[1].tolist() == [5] and not got[0].any()
    dur = np.full((1, 1025), 2.0 ** 20, np.float32)                                # 2^30 frames in all: clamped to the width
    assert _same(_run(dur, [1025], 1000), P.regulate(dur, [1025], 1000))


def test_refused_rows_raise_and_name_the_row():
    """the C entry marks a refused row with n_plan = -1 and leaves the others alone; the wrapper raises naming the row"""
    import t2v_hip
    base = np.ones((6, 300), np.float32)
    base[1, 299] = -0.25
    base[2, 2] = np.nan
    base[3, 0] = np.inf
    base[4, 257] = 2.0 ** 20 + 1
    want = P.regulate(base, [300] * 6, 64)
    assert want[1].tolist() == [64, -1, -1, -1, -1, 64]
    with pytest.raises(ValueError, match=r"row 1, 2, 3, 4\b"):
        t2v_hip.duration_plan(torch.from_numpy(base).cuda(), [300] * 6, 64)
    # the library itself: the good rows of the same launch are what they are alone
    lib = t2v_hip.load_library()
    d = torch.from_numpy(base).cuda()
    L = torch.full((6,), 300, dtype=torch.int32).cuda()
    plan = torch.full((6, 64), -7, dtype=torch.int32).cuda()
    n = torch.full((6,), -7, dtype=torch.int32).cuda()
    assert lib.t2v_duration_plan(t2v_hip._p(d), 300, t2v_hip._p(L), None, 0, 0, 6, 300, 64, t2v_hip._p(plan), 64, t2v_hip._p(n),
                                 t2v_hip._stream()) == 0
    torch.cuda.synchronize()
    assert _same((plan.cpu(), n.cpu()), want)
    # a rate can refuse a row too; a bad symbol past n_ids is not read
    with pytest.raises(ValueError, match="row 0"):
        t2v_hip.duration_plan(torch.ones(1, 3).cuda(), [3], 4, rate=-1.0)
    out = t2v_hip.duration_plan(torch.tensor([[1.0, 1.0, float('nan')]]).cuda(), [2], 4)
    assert out.n_plan.tolist() == [2] and out.plan[0].tolist() == [0, 1, 1, 1]


def test_arguments_are_checked_before_the_launch():
    import t2v_hip
    d = torch.ones(2, 3).cuda()
    for bad in (dict(dur=d.cpu()), dict(dur=d.double()), dict(dur=d[0]), dict(n_ids=[3]), dict(n_ids=[3, 4]), dict(T_max=0),
                dict(T_max=2.5), dict(rate=torch.ones(2, 2).cuda()), dict(rate=torch.ones(2, 3)),
                dict(dur=torch.ones(1, t2v_hip.PLAN_MAX_SYMBOLS + 1).cuda(), n_ids=[1])):
        a = dict(dur=d, n_ids=[3, 2], T_max=8, rate=None)
        a.update(bad)
        with pytest.raises((ValueError, t2v_hip.T2VHipError)):
            t2v_hip.duration_plan(a['dur'], a['n_ids'], a['T_max'], rate=a['rate'])
