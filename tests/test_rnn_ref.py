"""The step references of tests/rnn_ref.py against themselves: no GPU.  These are the conditions that make the bounds of
tests/test_recurrent_edges_gpu.py mean something:

  - in fp64 the BiLSTM reference is nn.LSTM on pack_padded_sequence(enforce_sorted=False) / pad_packed_sequence, and the GRU
    reference is nn.GRU, to 1e-12 for the output and every gradient, on every case torch accepts; a zero-length item, which torch
    does not accept, is the batch without it plus exact zeros for its row and its dx;
  - the saved tensors have the layout the kernels write (gates / cells at time t, nothing past a length);
  - every mutation moves at least one asserted quantity 100 bounds (K = 16) away, on the cases the device test uses it on.

Every figure is printed (pytest -s)."""
import pytest
import torch
from torch import nn

import rnn_ref as R

F32, F64 = torch.float32, torch.float64
K = 16.0
MARGIN = 100.0
TOL = 1e-12


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    R.oracle.cache_clear()
    R.floor.cache_clear()


def _torch_lstm(x, wo, lens, params):
    lstm = nn.LSTM(512, R.H, 1, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for k, p in lstm.named_parameters():
            p.copy_(params[k].double())
    xx = x.double().requires_grad_(True)
    packed = nn.utils.rnn.pack_padded_sequence(xx, torch.tensor(lens), batch_first=True, enforce_sorted=False)
    y, _ = nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=x.shape[1])
    (y * wo.double()).sum().backward()
    return {'y': y.detach(), 'dx': xx.grad, 'grad': {k: p.grad for k, p in lstm.named_parameters()}}


def _check(title, res, ref, tol=TOL):
    for q, (e, where) in R.compare(res, ref).items():
        print('%s %-6s err %.2e at %s' % (title, q, e, where))
        assert e <= tol, (title, q, e, where)


def test_case_tables():
    assert [c.B for c in R.LSTM_SWEEP] == list(range(1, 17)) == [c.B for c in R.GRU_SWEEP] == [c.B for c in R.GRU_LEN_SWEEP]
    for c in R.LSTM_SWEEP[1:]:
        assert min(c.lens) == 1 and max(c.lens) == c.T == 6 and list(c.lens) != sorted(c.lens, reverse=True)
    for c in R.GRU_LEN_SWEEP[1:]:
        assert min(c.steps) == 1 and max(c.steps) == c.T == 5 and list(c.steps) != sorted(c.steps, reverse=True)
    # no length or step count above T, anywhere: the kernels form addresses from them
    assert all(len(c.lens) == c.B and 0 <= min(c.lens) and max(c.lens) <= c.T for c in R.LSTM_CASES)
    assert all(c.steps is None or (len(c.steps) == c.B and 1 <= min(c.steps) and max(c.steps) <= c.T) for c in R.GRU_CASES)
    assert len(set(c.name for c in R.LSTM_CASES)) == len(R.LSTM_CASES) and len(set(c.name for c in R.GRU_CASES)) == len(R.GRU_CASES)
    assert {c.B for c in R.LSTM_EDGES} == {5, 11} and R.case('long-T84-B11').lens.count(84) == 2
    assert max(R.case('T9-longest6-B5').lens) == 6 == max(R.case('T9-longest6-B11').lens)
    assert all(c.lens.count(0) == 1 and c.lens[2] == 0 for c in R.LSTM_EDGES if c.name.startswith('zero-length'))
    assert all(list(c.lens) == sorted(c.lens) for c in R.LSTM_EDGES if c.name.startswith('ascending'))
    # the items a mutation acts on at step 1 are still running then
    for m, c in R.LSTM_MUTATED:
        assert min(c.lens) < c.T
        assert c.lens[-1] >= 2 if m in ('neighbour_row', 'one_unit') else c.lens[0] >= 2 if m == 'drop_cell' else True
    assert sorted(c.B for m, c in R.LSTM_MUTATED if m == 'neighbour_row') == [5, 9, 12, 13]
    assert sorted(c.B for m, c in R.GRU_MUTATED if m == 'neighbour_row') == [5, 9, 12, 13]
    assert all(c.B == 11 for m, c in R.LSTM_MUTATED if m in ('drop_cell', 'one_unit'))
    # the same inputs every time
    a, b = R.lstm_inputs(R.LSTM_SWEEP[4]), R.lstm_inputs(R.LSTM_SWEEP[4])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    p = R.lstm_inputs(R.case('bias40-B7'))[2]
    assert (p['bias_ih_l0'][256:384] == 40).all() and (p['bias_ih_l0'][384:512] == -40).all()
    assert (p['bias_ih_l0_reverse'][:128] == 40).all() and (p['bias_ih_l0_reverse'][128:256] == -40).all()


@pytest.mark.parametrize("c", [c for c in R.LSTM_CASES if min(c.lens) > 0],
                         ids=lambda c: c.name)
def test_bilstm_reference_is_packed_nn_lstm(c):
    x, wo, params = R.lstm_inputs(c)
    ref = R.oracle(c, F64)
    _check('bilstm %s vs nn.LSTM' % c.name, _torch_lstm(x, wo, c.lens, params), ref)
    lens = torch.tensor(c.lens)
    past = torch.arange(c.T)[None, :] >= lens[:, None]
    assert float(ref['y'][past].abs().max() if past.any() else 0) == 0.0
    for q in ('gates', 'cells', 'dg'):
        assert ref[q].shape[:3] == (2, c.B, c.T)
        assert float(ref[q][:, past].abs().max() if past.any() else 0) == 0.0


def test_bilstm_saved_tensors_are_the_kernels_layout():
    """gates (2, B, T, i|f|g|o) and cells (2, B, T, 256) at TIME t in both directions: rebuilt from them alone,
    y[b, t] = o * tanh(c), and c = f * c_prev + i * g with c_prev the cell at t - 1 (forward) or t + 1 (reverse)"""
    c = R.case('sweep-B9')
    ref = R.oracle(c, F64)
    H = R.H
    g, cells = ref['gates'], ref['cells']
    assert (g[..., 3 * H:] * torch.tanh(cells) - torch.stack((ref['y'][..., :H], ref['y'][..., H:]))).abs().max().item() < 1e-15
    for b, n in enumerate(c.lens):
        for d in (0, 1):
            for t in range(n):
                tp = t - 1 if d == 0 else t + 1
                prev = cells[d, b, tp] if 0 <= tp < n else torch.zeros(H, dtype=F64)
                want = g[d, b, t, H:2 * H] * prev + g[d, b, t, :H] * g[d, b, t, 2 * H:3 * H]
                assert (want - cells[d, b, t]).abs().max().item() < 1e-15, (d, b, t)


@pytest.mark.parametrize("c", [c for c in R.LSTM_EDGES if c.name.startswith('zero-length')], ids=lambda c: c.name)
def test_a_zero_length_item_is_the_batch_without_it(c):
    b = c.lens.index(0)
    rest = [i for i in range(c.B) if i != b]
    ref, sub = R.oracle(c, F64), R.without(c, b)
    x, wo, params = R.lstm_inputs(c)
    _check('bilstm %s without item %d vs nn.LSTM' % (c.name, b),
           _torch_lstm(x[rest], wo[rest], [c.lens[i] for i in rest], params), sub)
    picked = {q: (ref[q][:, rest] if q in ('gates', 'cells', 'dg') else ref[q] if q == 'grad' else ref[q][rest]) for q in ref}
    _check('bilstm %s vs the batch without item %d' % (c.name, b), picked, sub)
    assert float(ref['y'][b].abs().max()) == 0.0 and float(ref['dx'][b].abs().max()) == 0.0
    assert all(float(ref[q][:, b].abs().max()) == 0.0 for q in ('gates', 'cells', 'dg'))


@pytest.mark.parametrize("c", R.GRU_CASES, ids=lambda c: c.name)
def test_gru_reference_is_nn_gru(c):
    x, wo, params = R.gru_inputs(c)
    ref = R.oracle(c, F64)
    gru = nn.GRU(R.H, R.H, batch_first=True).double()
    with torch.no_grad():
        for k, p in gru.named_parameters():
            p.copy_(params[k].double())
    xx = x.double().requires_grad_(True)
    out, _ = gru(xx)
    steps = torch.tensor(c.steps if c.steps is not None else (c.T,) * c.B)
    last = out[torch.arange(c.B), steps - 1]
    res = {'h_last': last.detach(), 'hs': torch.cat((torch.zeros(c.B, 1, R.H, dtype=F64), out.detach()), 1)}
    if c.steps is None:
        (last * wo.double()).sum().backward()
        res.update(dx=xx.grad, grad={k: p.grad for k, p in gru.named_parameters()})
    _check('gru %s vs nn.GRU' % c.name, res, ref)
    # gsave = r, z, n, hn: the next state rebuilt from it alone
    r, z, n = ref['gsave'].unbind(2)
    assert ((1 - z) * n + z * ref['hs'][:, :-1] - ref['hs'][:, 1:]).abs().max().item() < 1e-15
    w_hh, b_hh = params['weight_hh_l0'].double(), params['bias_hh_l0'].double()
    assert (ref['hs'][:, :-1] @ w_hh[2 * R.H:].t() + b_hh[2 * R.H:] - ref['hn']).abs().max().item() < 1e-12 * max(1.0, c.whh_scale * 4)
    assert c.steps is None or 'dx' not in ref


@pytest.mark.parametrize("mutation,c", R.LSTM_MUTATED + R.GRU_MUTATED, ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_mutation_stands_100_bounds_above_the_reference(mutation, c):
    """on the reference alone: mutated fp64 minus fp64, against the K = 16 bound of the device test"""
    ref, floors = R.oracle(c, F64), R.floor(c)
    bound = R.bounds(floors, ref, K)
    err = R.compare(R.oracle(c, F64, mutation), ref)
    kind = 'bilstm' if isinstance(c, R.LstmCase) else 'gru'
    ratios = {}
    for q, (e, where) in err.items():
        ratios[q] = e / bound[q]
        print('%s mutation %-14s %-16s %-6s moved %.2e floor %.2e bound %.2e ratio %.3g at %s'
              % (kind, mutation, c.name, q, e, floors[q], bound[q], ratios[q], where))
    assert max(ratios.values()) >= MARGIN, ratios
    if mutation == 'steps_T':           # only what is read out differs
        assert ratios['hs'] == 0.0 and ratios['h_last'] >= MARGIN
    # the floors themselves are at round-off: a mutation 100 bounds up is not a mutation 100 large floors up
    assert max(floors.values()) < 2e-5, floors


@pytest.mark.parametrize("c", R.LSTM_SATURATED + R.GRU_SATURATED, ids=lambda c: ('bilstm-' if isinstance(c, R.LstmCase) else 'gru-') + c.name)
def test_saturated_cases_saturate_and_stay_finite(c):
    ref, floors = R.oracle(c, F64), R.floor(c)
    for q, t in ref.items():
        for v in (t.values() if isinstance(t, dict) else (t,)):
            assert torch.isfinite(v).all(), q
    print('%s floors %s' % (c.name, {k: '%.2e' % v for k, v in floors.items()}))
    act = ref['gates'] if isinstance(c, R.LstmCase) else ref['gsave']
    lo, hi = (act.abs() < 1e-3).double().mean().item(), (act.abs() > 1 - 1e-3).double().mean().item()
    print('%s activations within 1e-3 of 0: %.3f, of +-1: %.3f' % (c.name, lo, hi))
    assert hi > 0.02, (lo, hi)
