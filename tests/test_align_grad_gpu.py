"""The decoder's reverse passes with an upstream gradient of the alignments, against the fp64 oracle.

The loss is sum(mel * wm) + sum(gate * wg) + sum(align * wa) on the steered inputs of tests/steer_ref.py (tests/aligngrad_ref.py:
wa is non-zero everywhere, also past an item's length, and tests/test_aligngrad_ref.py shows on the oracle alone that the term
moves grad and d_memory by thousands of parity bounds).  Seven shapes reach every form of the attention backward — 16-, 32- and
96-position slices on four and eight waves, the launch-per-step kernel, the one-launch pass behind a launch-per-step forward, and
a batch of 18 that runs as chunks of 16 and 2 — on every engine pair a shape qualifies for.

(a) parity: every quantity within steer_ref.bounds(floor_with_align, ref, 16) of the fp64 oracle with the term;
(b) seen: the same device results against the fp64 oracle WITHOUT the term are over the bound in grad and d_memory;
(c) zero is exact: wa = 0 as a tensor gives the bits of a loss without the term (no alignment gradient at all);
(d) layouts: the gradient as a (B, T, T_in) contiguous tensor (copied) and as a view of (T, B, T_in) storage (taken as it is);
(e) the bf16 engines: error against the fp64 oracle at most twice that of the same engine without the term.

Every row is printed next to its floor and bound before it is asserted (pytest -s); profiles/align_grad_parity.txt is that table
from an MI355X."""
import pytest
import torch

import aligngrad_ref as R
import steer_ref as S
from test_decoder_steered_gpu import ENGINES, _engines, _id

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K = 16.0
KERNELS = {'persistent': 'k_achain_bwd', 'launch-per-step': 'k_lstm_bwd256 + k_attn_cell_bwd'}

PARITY = [(c, e) for c in R.CASES for e in _engines(c)]
ZERO = [(c, e) for c in R.CASES[:3] for e in _engines(c)]

_DEVICE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    S.oracle.cache_clear()
    R.oracle_with_align.cache_clear()


def _run(case, engine, monkeypatch, wa, direct=False, bwd_kernel=None):
    """The HIP decoder on the steered inputs, loss sum(mel * wm) + sum(gate * wg) [+ sum(align * wa)]: (mel, gate, align,
    {parameter: gradient}, d memory) on the host.  wa: None (no alignment term) or a device tensor (B, T, T_in); direct: wa is
    handed to autograd as the gradient of the alignments itself, in the strides it has."""
    import model as M
    import t2v_hip
    fwd, bwd, fwd_mode, bwd_mode = ENGINES[engine]
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent', fwd)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent_bwd', bwd)
    dec, memory, mels, lengths, wm, wg = S.inputs(case)
    dev = torch.device('cuda:0')
    dec = dec.to(dev).train()
    dec.p_attention_dropout = dec.p_decoder_dropout = 0.0
    dec._calls = 0
    mem = memory.to(dev).requires_grad_(True)
    mel, gate, align = dec(mem, mels.to(dev), lengths.to(dev))
    assert t2v_hip.DecoderCore.last_mode == fwd_mode
    loss = (mel * wm.to(dev)).sum() + (gate * wg.to(dev)).sum()
    if wa is None:
        loss.backward()
    elif direct:
        torch.autograd.backward([loss, align], [None, wa])
    else:
        (loss + (align * wa).sum()).backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert t2v_hip.DecoderCore.last_bwd_mode == bwd_mode
    assert t2v_hip.DecoderCore.last_bwd_kernel == (bwd_kernel or KERNELS[bwd_mode])
    assert len(t2v_hip.DecoderCore.chunk_bwd_kernels) == (case[0] + 15) // 16
    assert all(p.grad is not None for p in dec.parameters())
    grads = {n: p.grad.cpu() for n, p in dec.named_parameters()}
    return (mel.detach().cpu(), gate.detach().cpu(), align.detach().cpu(), grads, mem.grad.cpu())


def _with_term(case, engine, monkeypatch):
    if (case, engine) not in _DEVICE:
        _DEVICE[case, engine] = _run(case, engine, monkeypatch, R.wa(case, R.SCALE[case]).cuda())
    return _DEVICE[case, engine]


def _judge(title, res, ref, floors):
    """prints one row per quantity; returns {quantity: error / bound}"""
    err, bound = S.compare(res, ref), S.bounds(floors, ref, K)
    ratio = {}
    for q in S.QUANTITIES:
        e, where = err[q]
        print('%s %-8s err %.2e floor %.2e K %g bound %.2e at %s' % (title, q, e, floors[q], K, bound[q], where))
        ratio[q] = e / bound[q]
    return ratio


def _same_gradients(a, b):
    return all(torch.equal(a[3][n], b[3][n]) for n in a[3]) and torch.equal(a[4], b[4]) and set(a[3]) == set(b[3])


# ------------------------------------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("case,engine", PARITY, ids=['%s-%s' % (_id(c), e) for c, e in PARITY])
def test_alignment_gradient_matches_oracle(case, engine, monkeypatch):
    """every quantity within 16 * max(floor, 4 * 2^-24 * scale) of the fp64 oracle whose loss has the alignment term"""
    ref = R.oracle_with_align(case, F64, R.SCALE[case])
    res = _with_term(case, engine, monkeypatch)
    ratio = _judge('align-grad parity %s %s' % (_id(case), engine), res, ref, R.floor_with_align(case))
    assert max(ratio.values()) < 1, ratio


# ------------------------------------------------------------------------------------------------ (b) the term is seen
@pytest.mark.parametrize("case,engine", PARITY, ids=['%s-%s' % (_id(c), e) for c, e in PARITY])
def test_oracle_without_the_term_is_over_the_bound(case, engine, monkeypatch):
    """the same device results against the fp64 oracle without the alignment term: grad and d_memory over the parity bound,
    the forward quantities within it"""
    res = _with_term(case, engine, monkeypatch)
    ratio = _judge('align-grad seen   %s %s' % (_id(case), engine), res, S.oracle(case, F64), R.floor_with_align(case))
    assert max(ratio['mel'], ratio['gate'], ratio['align']) < 1, ratio
    assert ratio['grad'] > 1 and ratio['d_memory'] > 1, ratio


# ------------------------------------------------------------------------------------------------ (c) zero is exact
@pytest.mark.parametrize("case,engine", ZERO, ids=['%s-%s' % (_id(c), e) for c, e in ZERO])
def test_zero_alignment_gradient_changes_no_bit(case, engine, monkeypatch):
    """wa = 0 passed as a tensor (the kernels with the operand) against a loss without the term (the pointer-less kernels)"""
    plain = _run(case, engine, monkeypatch, None)
    zero = _run(case, engine, monkeypatch, torch.zeros(case[0], case[2], case[1], device='cuda:0'))
    assert _same_gradients(plain, zero)
    assert all(torch.equal(plain[i], zero[i]) for i in range(3))


# ------------------------------------------------------------------------------------------------ (d) layouts
@pytest.mark.parametrize("engine", _engines(R.CASES[1]))
def test_both_layouts_of_the_alignment_gradient_give_the_same_bits(engine, monkeypatch):
    """(B, T, T_in) contiguous: one copy into the kernels' layout; a (B, T, T_in) view of (T, B, T_in) storage: handed on as it is"""
    import t2v_hip
    case = R.CASES[1]
    handed = []
    inner = t2v_hip.DecoderCore._dal_chunk

    def spy(dalign, b0, B, Bt):
        out = inner(dalign, b0, B, Bt)
        handed.append((dalign.data_ptr(), out.data_ptr(), out.is_contiguous(), tuple(out.shape)))
        return out
    monkeypatch.setattr(t2v_hip.DecoderCore, '_dal_chunk', staticmethod(spy))
    w = R.wa(case, R.SCALE[case]).cuda()
    w_tb = w.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert w.is_contiguous() and not w_tb.is_contiguous() and torch.equal(w, w_tb)
    a = _run(case, engine, monkeypatch, w, direct=True)
    b = _run(case, engine, monkeypatch, w_tb, direct=True)
    assert _same_gradients(a, b)
    (src_a, dst_a, c_a, shape_a), (src_b, dst_b, c_b, shape_b) = handed
    assert shape_a == shape_b == (case[2], case[0], case[1]) and c_a and c_b
    assert src_a == w.data_ptr() and dst_a != src_a                 # copied
    assert src_b == w_tb.data_ptr() and dst_b == src_b              # not copied
    # and through the loss, as the parity test gives it
    assert _same_gradients(a, _with_term(case, engine, monkeypatch))


# ------------------------------------------------------------------------------------------------ (e) bf16 engines
BF16_CASES = ((3, 16, 6, (16, 11, 5)), (7, 40, 9, (40, 35, 30, 25, 20, 15, 10)), (16, 84, 12, tuple(range(84, 36, -3))),
              (16, 225, 5, tuple(range(225, 97, -8))))


@pytest.mark.parametrize("case", BF16_CASES, ids=[_id(c) for c in BF16_CASES])
def test_bf16_engines_carry_the_alignment_gradient(case, monkeypatch):
    """bf16_run, persistent16 forced (k_dec_train_persist16 + k_bwd_persist16).  The fp64 oracle has no bf16 form, so the yardstick
    is the engine itself: e0 = its error against the fp64 oracle without the term, e = with the term against the oracle with it,
    both as steer_ref.compare measures.  e <= 2 * max(e0, fp32 bound): the term adds one fp32 addend on a path that is otherwise
    the same, and the bf16 rounding of the gate gradients scales with the gradient, which compare divides out."""
    import t2v_hip
    B, T_in, T = case[:3]
    assert len(case[3]) == B
    if not t2v_hip.load_library().t2v_decoder_bwd_persist16_fits(B, T_in, T):
        pytest.skip('k_bwd_persist16 does not take this shape on this device')
    old = t2v_hip.bf16_enabled()
    t2v_hip.set_bf16(True)
    try:
        monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent16', 'force')
        monkeypatch.setitem(ENGINES, 'bf16', (True, True, 'persistent', 'persistent'))
        scale = 1.0
        plain = _run(case, 'bf16', monkeypatch, None, bwd_kernel='k_bwd_persist16')
        assert t2v_hip.DecoderCore.last_kernel == 'k_dec_train_persist16'
        term = _run(case, 'bf16', monkeypatch, R.wa(case, scale).cuda(), bwd_kernel='k_bwd_persist16')
    finally:
        t2v_hip.set_bf16(old)
    ref = R.oracle_with_align(case, F64, scale)
    e0 = S.compare(plain, S.oracle(case, F64))
    e = S.compare(term, ref)
    bound = S.bounds(R.floor_with_align(case, scale), ref, K)
    failed = []
    for q in S.QUANTITIES:
        limit = 2.0 * max(e0[q][0], bound[q])
        row = 'align-grad bf16 %s %-8s e %.2e e0 %.2e fp32 bound %.2e limit %.2e at %s' % (_id(case), q, e[q][0], e0[q][0], bound[q], limit,
                                                                                        e[q][1])
        print(row)
        if not e[q][0] <= limit:
            failed.append(row)
    assert not failed, failed
    # the term is seen here as well: the run without it is over the limit against this oracle — in d_memory (in `grad` the worst
    # tensor's bf16 error, a Prenet weight's, is as large as the term itself)
    far = S.compare(plain, ref)['d_memory'][0]
    print('align-grad bf16 %s d_memory of the run without the term against this oracle: %.2e' % (_id(case), far))
    assert far > 2.0 * max(e0['d_memory'][0], bound['d_memory'])
