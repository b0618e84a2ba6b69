"""The cooperative recurrences outside the decoder against the fp64 step references of tests/rnn_ref.py, at round-off scale:
k_bilstm_fwd<4|8|12|16> / k_bilstm_bwd (csrc/bilstm.hip) through t2v_hip.BiLSTM, k_gru_fwd / k_gru_bwd (csrc/refenc.hip,
csrc/refenc_fwd.inc) through t2v_hip.GRULast, and k_gru_fwd_len, the ragged inference instance, through its C entry point
called as t2v_hip.refenc_ragged calls it.

(a) every batch width B = 1 .. 16 of all three, unsorted lengths / step counts that hold both 1 and T;
(b) length and T edges at B = 5 and 11 (the <8> and <12> forward instantiations): T = 1, T = 2, every length 1 under T = 7,
    three trailing steps with nobody active, ascending lengths, a zero-length item, 84 steps; GRU at T = 1, 2, 19, B = 9, 13;
(c) saturated gates: x * 6 with W_hh * 4, a gate block biased to +-40, and one biased to +-100, past the overflow of the
    exp inside sigmoidf_ / tanhf_ (csrc/t2v_common.h) — nothing saved may be NaN or inf;
(d) the device results of (a) - (c) against a MUTATED fp64 reference (a reverse direction that starts at T - 1, a last item that
    reads its neighbour's row, a cell state or a single cell unit lost once, h_last read after T steps) must FAIL — nothing in
    the kernels is altered;
(e) bit-identical reruns, BiLSTM.prepare, save=False, non-contiguous x.

Besides the outputs and gradients every case reads what the kernels save (gates, cells; hs, gsave: off grad_fn.keep) and the gate
gradients they hand to the weight-gradient GEMMs (dg; dgi, dgh: from the backward entry point on those saved tensors).

Bounds.  floor = fp32 reference minus fp64 reference, per case and quantity (rnn_ref.floor).  A quantity passes below
K * max(floor, 4 * 2^-24 * scale), K = 16, the rule of test_decoder_steered_gpu.py.  Outputs, states and saved activations are
absolute with scale 1: they are bounded by 1 and the kernels' sigmoid / tanh carry ~1e-7 absolute by design, so no small-signal
relative bound is asserted.  Cell states and hn = W_hn h + b_hn, which are not bounded by 1, are absolute with scale =
max |reference|.  dx, the gate gradients and each parameter gradient are relative to their tensor's largest reference entry.

Every case prints its worst values next to floor, K and bound before it asserts (pytest -s); profiles/recurrent_edges_parity.txt
is that table from an MI355X.  No case hands a kernel a length or step count above T: addresses are formed from it.
"""
import pytest
import torch

import rnn_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K = 16.0
H = R.H

_DEVICE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    R.oracle.cache_clear()
    R.floor.cache_clear()


def _cpu(t):
    return {k: _cpu(v) for k, v in t.items()} if isinstance(t, dict) else t.detach().cpu()


# ------------------------------------------------------------------------------------------------ the kernels on a case
def _bilstm_apply(x, lens, P, save=True):
    import t2v_hip
    return t2v_hip.BiLSTM.apply(x, lens, *[P[n] for n in R.LSTM_NAMES], save)


def _lstm_run(c):
    """BiLSTM.apply + backward on the case's inputs; every compared quantity on the host.  gates / cells are zeroed past
    each length, where the kernels write nothing (the arenas are torch.empty)."""
    import t2v_hip
    x, wo, params = R.lstm_inputs(c)
    dev = torch.device('cuda:0')
    P = {k: v.clone().to(dev).requires_grad_(True) for k, v in params.items()}
    gx = x.to(dev).requires_grad_(True)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=dev)
    dy = wo.to(dev)
    y = _bilstm_apply(gx, lens, P)
    keep = y.grad_fn.keep
    whh, chunks = keep[4], keep[6]
    assert len(chunks) == 1
    gates, cells = chunks[0][2], chunks[0][3]
    (y * dy).sum().backward()
    # the gate gradients the reverse kernel hands to the GEMMs: the same entry point on the same saved tensors
    lib = t2v_hip.load_library()
    dg = torch.empty(2, c.B, c.T, 4 * H, device=dev)
    dgx = torch.empty(2 * 2 * 2 * 16 * 16 * H, device=dev)
    sync = torch.empty(3, device=dev, dtype=torch.int32)
    t2v_hip._check(lib.t2v_bilstm_bwd(t2v_hip._p(whh), t2v_hip._p(lens), t2v_hip._p(dy), t2v_hip._p(gates), t2v_hip._p(cells),
                                      t2v_hip._p(dg), t2v_hip._p(dgx), t2v_hip._p(sync), c.B, c.T, t2v_hip._stream()),
                   't2v_bilstm_bwd')
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    t2v_hip.bilstm_check(sync)
    assert all(p.grad is not None for p in P.values())
    valid = (torch.arange(c.T)[None, :] < torch.tensor(c.lens)[:, None])[None, :, :, None]
    return {'y': _cpu(y), 'gates': torch.where(valid, _cpu(gates), torch.zeros(())), 'cells': torch.where(valid, _cpu(cells), torch.zeros(())),
            'dg': _cpu(dg), 'dx': _cpu(gx.grad), 'grad': {k: _cpu(p.grad) for k, p in P.items()}}


def _gru_run(c):
    """GRULast.apply + backward on the case's inputs"""
    import t2v_hip
    x, wo, params = R.gru_inputs(c)
    dev = torch.device('cuda:0')
    P = {k: v.clone().to(dev).requires_grad_(True) for k, v in params.items()}
    gx = x.to(dev).requires_grad_(True)
    dh = wo.to(dev)
    out = t2v_hip.GRULast.apply(gx, *[P[n] for n in R.GRU_NAMES])
    keep = out.grad_fn.keep
    whh, hs, gsave = keep[2], keep[3], keep[4]
    assert len(keep[6]) == 1
    (out * dh).sum().backward()
    lib = t2v_hip.load_library()
    dgi, dgh = torch.empty(c.B, c.T, 3 * H, device=dev), torch.empty(c.B, c.T, 3 * H, device=dev)
    xchg = torch.empty(2 * 16 * 3 * H, device=dev)
    sync = torch.empty(2, device=dev, dtype=torch.int32)
    t2v_hip._check(lib.t2v_gru_bwd(t2v_hip._p(whh), t2v_hip._p(hs), t2v_hip._p(gsave), t2v_hip._p(dh), t2v_hip._p(dgi),
                                   t2v_hip._p(dgh), t2v_hip._p(xchg), t2v_hip._p(sync), c.B, c.T, t2v_hip._stream()), 't2v_gru_bwd')
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert int(sync[1].item()) == 0
    return {'h_last': _cpu(out), 'hs': _cpu(hs), 'gsave': _cpu(gsave)[:, :, :3], 'hn': _cpu(gsave)[:, :, 3], 'dgi': _cpu(dgi),
            'dgh': _cpu(dgh), 'dx': _cpu(gx.grad), 'grad': {k: _cpu(p.grad) for k, p in P.items()}}


def _gru_len_run(c):
    """t2v_gru_fwd_len alone, called as refenc_ragged calls it (input projection on the HIP GEMM, no gsave).  h_last starts
    as NaN: a row the kernel does not write shows."""
    import t2v_hip
    x, _, params = R.gru_inputs(c)
    dev = torch.device('cuda:0')
    w_ih, w_hh, b_ih, b_hh = (params[n].to(dev) for n in R.GRU_NAMES)
    assert 1 <= min(c.steps) and max(c.steps) <= c.T
    steps = torch.tensor(c.steps, dtype=torch.int32, device=dev)
    lib = t2v_hip.load_library()
    gi = t2v_hip.gemm(x.to(dev).view(c.B * c.T, H), w_ih, b_ih).view(c.B, c.T, 3 * H)
    hs = torch.empty(c.B, c.T + 1, H, device=dev)
    h_last = torch.full((c.B, H), float('nan'), device=dev)
    xchg = torch.empty(2 * 16 * H, device=dev)
    sync = torch.empty(2, device=dev, dtype=torch.int32)
    t2v_hip._check(lib.t2v_gru_fwd_len(t2v_hip._p(gi), t2v_hip._p(w_hh), t2v_hip._p(b_hh), t2v_hip._p(hs), None, t2v_hip._p(xchg),
                                       t2v_hip._p(sync), t2v_hip._p(steps), t2v_hip._p(h_last), c.B, c.T, t2v_hip._stream()),
                   't2v_gru_fwd_len')
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert int(sync[1].item()) == 0
    return {'h_last': _cpu(h_last), 'hs': _cpu(hs)}


def _run(c):
    return _lstm_run(c) if isinstance(c, R.LstmCase) else _gru_len_run(c) if c.steps is not None else _gru_run(c)


def _device(c):
    """the device's quantities of a case, computed once: (d) and (e) look at them again"""
    if c not in _DEVICE:
        _DEVICE[c] = _run(c)
    return _DEVICE[c]


def _kind(c):
    return 'bilstm' if isinstance(c, R.LstmCase) else 'gru_len' if c.steps is not None else 'gru'


def _judge(title, res, ref, floors):
    """prints one row per quantity; returns ({quantity: error / bound}, the rows over their bound)"""
    err, bound = R.compare(res, ref), R.bounds(floors, ref, K)
    ratio, failed = {}, []
    for q in R.ORDER:
        if q not in err:
            continue
        e, where = err[q]
        row = '%s %-6s err %.2e floor %.2e K %g bound %.2e at %s' % (title, q, e, floors[q], K, bound[q], where)
        print(row)
        ratio[q] = e / bound[q]
        if not e < bound[q]:
            failed.append(row)
    return ratio, failed


def _finite(res):
    for q, t in res.items():
        for v in (t.values() if isinstance(t, dict) else (t,)):
            assert torch.isfinite(v).all(), q


def _exact_zeros_past_lengths(c, res):
    for b, n in enumerate(c.lens):
        if n < c.T:
            assert float(res['y'][b, n:].abs().max()) == 0.0, b
            assert float(res['dg'][:, b, n:].abs().max()) == 0.0, b


def _parity(c):
    res = _device(c)
    _finite(res)
    _, failed = _judge('%s parity %s' % (_kind(c), c.name), res, R.oracle(c, F64), R.floor(c))
    assert not failed, failed
    return res


# ------------------------------------------------------------------------------------------------ (a) width sweep
@pytest.mark.parametrize("c", R.LSTM_SWEEP, ids=lambda c: c.name)
def test_bilstm_every_width(c):
    """y, gates, cells, dg, dx and the eight parameter gradients at B = 1 .. 16, T = 6; y and dg exactly zero past each length"""
    _exact_zeros_past_lengths(c, _parity(c))


@pytest.mark.parametrize("c", R.GRU_SWEEP, ids=lambda c: c.name)
def test_gru_every_width(c):
    """h_last, hs, gsave, dgi, dgh, dx and the four parameter gradients at B = 1 .. 16, T = 3"""
    res = _parity(c)
    assert torch.equal(res['h_last'], res['hs'][:, c.T]) and float(res['hs'][:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("c", R.GRU_LEN_SWEEP, ids=lambda c: c.name)
def test_gru_fwd_len_every_width(c):
    """h_last[b] against the fp64 state after steps[b] steps, and every state, at B = 1 .. 16, T = 5"""
    res = _parity(c)
    for b, n in enumerate(c.steps):
        assert torch.equal(res['h_last'][b], res['hs'][b, n]), b


# ------------------------------------------------------------------------------------------------ (b) length and T edges
@pytest.mark.parametrize("c", [c for c in R.LSTM_EDGES if min(c.lens) > 0], ids=lambda c: c.name)
def test_bilstm_length_and_T_edges(c):
    _exact_zeros_past_lengths(c, _parity(c))


@pytest.mark.parametrize("c", [c for c in R.LSTM_EDGES if min(c.lens) == 0], ids=lambda c: c.name)
def test_bilstm_zero_length_item(c):
    """the item's y, dx and dg rows are exactly 0; every other item and every parameter gradient are those of the batch
    without it (tests/test_rnn_ref.py: the reference of the whole batch is that reference to 1e-12)"""
    res = _parity(c)
    _exact_zeros_past_lengths(c, res)
    b = c.lens.index(0)
    assert float(res['dx'][b].abs().max()) == 0.0
    rest = [i for i in range(c.B) if i != b]
    picked = {q: (res[q][:, rest] if q in ('gates', 'cells', 'dg') else res[q] if q == 'grad' else res[q][rest]) for q in res}
    _, failed = _judge('bilstm parity %s without item %d' % (c.name, b), picked, R.without(c, b), R.floor(c))
    assert not failed, failed


@pytest.mark.parametrize("c", R.GRU_EDGES, ids=lambda c: c.name)
def test_gru_T_edges(c):
    _parity(c)


# ------------------------------------------------------------------------------------------------ (c) saturation
@pytest.mark.parametrize("c", R.LSTM_SATURATED, ids=lambda c: c.name)
def test_bilstm_saturated_gates(c):
    res = _parity(c)                # (finite everywhere: _parity)
    _exact_zeros_past_lengths(c, res)
    if c.bias:                      # the biased gate blocks sit at exactly 1 and 0, where an item runs
        run = (torch.arange(c.T)[None, :] < torch.tensor(c.lens)[:, None])
        f = res['gates'][0][run][:, H:2 * H]
        assert (f[:, :H // 2] == 1).all() and (f[:, H // 2:] < 1e-15).all()


@pytest.mark.parametrize("c", R.GRU_SATURATED, ids=lambda c: c.name)
def test_gru_saturated_gates(c):
    _parity(c)


# ------------------------------------------------------------------------------------------------ (d) mutations must fail
@pytest.mark.parametrize("mutation,c", R.LSTM_MUTATED + R.GRU_MUTATED,
                         ids=['%s-%s-%s' % (_kind(c), m, c.name) for m, c in R.LSTM_MUTATED + R.GRU_MUTATED])
def test_a_mutated_reference_is_seen(mutation, c):
    """CPU-side mutations of the REFERENCE: against each the unmutated kernels' results are over the bound of the parity test"""
    ratio, _ = _judge('%s mutation %s %s' % (_kind(c), mutation, c.name), _device(c), R.oracle(c, F64, mutation), R.floor(c))
    if mutation == 'steps_T':           # the states themselves are untouched, what is read out is not
        assert ratio['hs'] < 1 < ratio['h_last'], ratio
        print('mutation asserted on %s %s %s: err / bound %.3g' % (mutation, c.name, 'h_last', ratio['h_last']))
    else:
        q = max(ratio, key=ratio.get)
        assert ratio[q] > 1, ratio
        print('mutation asserted on %s %s %s: err / bound %.3g' % (mutation, c.name, q, ratio[q]))


# ------------------------------------------------------------------------------------------------ (e) reproducibility, host paths
def _same_bits(a, b):
    for q in a:
        if isinstance(a[q], dict):
            assert all(torch.equal(a[q][k], b[q][k]) for k in a[q]), q
        else:
            assert torch.equal(a[q], b[q]), q


@pytest.mark.parametrize("c", R.LSTM_SWEEP + R.GRU_SWEEP + R.GRU_LEN_SWEEP, ids=lambda c: '%s-%s' % (_kind(c), c.name))
def test_a_second_run_has_the_same_bits(c):
    _same_bits(_device(c), _run(c))


def _lstm_on_device(c):
    x, wo, params = R.lstm_inputs(c)
    P = {k: v.clone().cuda().requires_grad_(True) for k, v in params.items()}
    return x.cuda(), wo.cuda(), P, torch.tensor(c.lens, dtype=torch.int32, device='cuda')


def test_bilstm_prepare_gives_the_same_bits_and_is_consumed():
    import t2v_hip
    c = R.case('sweep-B12')
    x, wo, P, lens = _lstm_on_device(c)
    prep = [P[n] for n in ('weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')]
    key = id(P['weight_hh_l0'])
    t2v_hip.BiLSTM._prep.pop(key, None)
    t2v_hip.BiLSTM.prepare(*prep)
    assert key in t2v_hip.BiLSTM._prep
    gx = x.clone().requires_grad_(True)
    y = _bilstm_apply(gx, lens, P)
    assert key not in t2v_hip.BiLSTM._prep                  # consumed
    (y * wo).sum().backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    plain = _device(c)                                      # apply alone, same inputs
    assert torch.equal(y.detach().cpu(), plain['y']) and torch.equal(gx.grad.cpu(), plain['dx'])
    assert all(torch.equal(P[k].grad.cpu(), plain['grad'][k]) for k in P)
    # nothing stale: after an in-place change of weight_hh the next apply uses the new weights
    with torch.no_grad():
        P['weight_hh_l0'].mul_(0.5)
    y2 = _bilstm_apply(x, lens, P, False)
    fresh = {k: v.detach().clone() for k, v in P.items()}
    y3 = _bilstm_apply(x, lens, fresh, False)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert torch.equal(y2, y3) and not torch.equal(y2[..., :H], y.detach()[..., :H])
    assert torch.equal(y2[..., H:], y.detach()[..., H:])    # the reverse direction's weights did not change


def test_bilstm_backward_without_saved_activations_raises():
    import t2v_hip
    c = R.case('sweep-B5')
    x, wo, P, lens = _lstm_on_device(c)
    y = _bilstm_apply(x.requires_grad_(True), lens, P, False)
    with pytest.raises(t2v_hip.T2VHipError):
        (y * wo).sum().backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()


def test_non_contiguous_x_equals_its_contiguous_copy():
    import t2v_hip
    c = R.case('sweep-B7', R.LSTM_SWEEP)
    x, wo, P, lens = _lstm_on_device(c)
    xt = x.transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)         # (B, T, 512) view of a (T, B, 512) tensor
    assert not xt.is_contiguous()
    y = _bilstm_apply(xt, lens, P)
    (y * wo).sum().backward()
    torch.cuda.synchronize()
    plain = _device(c)
    assert torch.equal(y.detach().cpu(), plain['y']) and torch.equal(xt.grad.cpu(), plain['dx'])
    c = R.case('sweep-B7', R.GRU_SWEEP)
    x, wo, params = R.gru_inputs(c)
    P = [params[n].cuda().requires_grad_(True) for n in R.GRU_NAMES]
    xt = x.cuda().transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    assert not xt.is_contiguous()
    out = t2v_hip.GRULast.apply(xt, *P)
    (out * wo.cuda()).sum().backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    plain = _device(c)
    assert torch.equal(out.detach().cpu(), plain['h_last']) and torch.equal(xt.grad.cpu(), plain['dx'])
