"""A condition on the inputs of tests/test_align_grad_gpu.py, checked on the oracle alone (no GPU): with the committed scale of
wa, the fp64 oracle with the alignment term and the fp64 oracle without it are further apart than the parity bound in `grad` and
in `d_memory` — so a device pass that dropped the alignment gradient could not pass the parity test — while the forward
quantities are the same."""
import pytest
import torch

import aligngrad_ref as R
import steer_ref as S

F64 = torch.float64


@pytest.mark.parametrize("case", R.CASES, ids=['B%d-Tin%d-T%d' % c[:3] for c in R.CASES])
def test_alignment_term_moves_the_gradients_by_more_than_the_parity_bound(case):
    ref = R.oracle_with_align(case, F64, R.SCALE[case])
    without = S.oracle(case, F64)
    dist = S.compare(without, ref)
    bound = S.bounds(R.floor_with_align(case), ref, 16.0)
    for q in S.QUANTITIES:
        print('alignment term %s %-8s distance %.3e bound %.3e' % (case[:3], q, dist[q][0], bound[q]))
    assert dist['grad'][0] > bound['grad'] and dist['d_memory'][0] > bound['d_memory'], (dist, bound)
    assert dist['mel'][0] == 0 and dist['gate'][0] == 0 and dist['align'][0] == 0


def test_wa_is_nonzero_everywhere_and_zero_scale_is_the_plain_oracle():
    case = R.CASES[0]
    w = R.wa(case, R.SCALE[case])
    assert w.shape == (case[0], case[2], case[1]) and (w != 0).all()
    assert torch.equal(w, R.wa(case, R.SCALE[case]))                # fixed seed
    a, b = R.oracle_with_align(case, F64, 0.0), S.oracle(case, F64)
    assert all(torch.equal(a[3][k], b[3][k]) for k in b[3]) and torch.equal(a[4], b[4])
    # alpha is exactly 0 past an item's length: a gradient there has nothing to act on
    n = case[3][1]
    assert n < case[1] and a[2][1, :, n:].abs().max().item() == 0.0
