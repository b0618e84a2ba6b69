"""Dropout ON against the oracle.  The device's keep-masks are a pure function of (seed, stream, t, idx); tests/drop_ref.py
restates that function on the host, so the oracle can be run with the very masks the kernels draw:

(a) the replica is the device's function: zero patterns of ConvBNAct1d outputs and of the decoder's saved h rows, exactly;
(b) decoder core, LSTM state dropout on, forward and every gradient against the fp64 oracle with the replayed masks, on
    both fp32 engine pairs (persistent forward + one-launch reverse pass, launch-per-step forward + launch-per-step BPTT);
(c) the comparison of (b) sees a c mask taken at the wrong step and a mask indexed with the wrong item;
(d) ConvBNAct1d with dropout on: output, dx, dw, dgamma, dbeta against fp64 with the replayed mask, both convolution forms.

Bounds are those of the dropout-off tests (test_decoder_core_matches_oracle, test_conv_bn_act_matches_torch); absolute forward
bounds are multiplied by 1 / (1 - p), the one factor dropout adds to kept values.  Prenet dropout is off (M.drop_rate = 0:
LinearHIP's mask backward has its own test) and there is no training engine here, so seeds are the by-value ones.

Every case prints its worst values next to the bounds before it asserts (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import drop_ref as R

pytestmark = pytest.mark.gpu

SEED_MASK = 0x7FFFFFFFFFFFFFFF

# (B, T_in, T_out, lengths): the smallest shapes that reach each branch — T = 1 never takes the `t > 0` guard of the c mask,
# 300 symbols take the long attention form, 20 items run as chunks of 16 + 4 (chunk seed, chunk-local item index)
DEC_SHAPES = [(3, 20, 12, (20, 17, 9)), (6, 84, 24, (84, 80, 71, 66, 50, 37)), (1, 33, 7, (33,)), (3, 17, 1, (17, 5, 1)),
              (2, 300, 4, (300, 211)), (20, 33, 3, tuple(range(33, 13, -1)))]
DEC_RATES = [(s, 0.1, 0.1) for s in range(len(DEC_SHAPES))] + [(0, 0.5, 0.25), (1, 0.5, 0.25)]
# forward engine / reverse engine pairs (DecoderCore.persistent, .persistent_bwd, expected last_mode, last_bwd_mode)
ENGINES = {'persistent+achain': (True, True, 'persistent', 'persistent'),
           'launch-per-step+steps': (False, False, 'launch-per-step', 'launch-per-step')}
# the one-launch kernels take B <= 6; larger batches are the launch-per-step loop's
DEC_CASES = sorted((s, pa, pd, e) for s, pa, pd in DEC_RATES for e in ENGINES if e != 'persistent+achain' or DEC_SHAPES[s][0] <= 6)


def _call_seed(dec, call=1):
    return (int(dec.dropout_seed) * 1000003 + call) & SEED_MASK


def _setup(shape):
    """the harness of test_decoder_core_matches_oracle (it switches the Prenet dropout off for good: put back here, the
    device run switches it off for its own duration)"""
    import model as M
    import test_decoder_gpu as TD
    B, T_in, T, lens = DEC_SHAPES[shape]
    old = M.drop_rate
    try:
        return TD._setup(B, T_in, T, list(lens))
    finally:
        M.drop_rate = old


def _correct_keeps(seed, B, T, p_att, p_dec):
    return R.decoder_state_keeps(seed, 0, B, T, p_att, p_dec)


def _c_shifted_keeps(seed, B, T, p_att, p_dec):
    """mutation: the c masks of step t taken from step t + 1"""
    k = R.decoder_state_keeps(seed, 0, B, T + 1, p_att, p_dec)
    return [dict(k[t], att_c=k[t + 1]['att_c'], dec_c=k[t + 1]['dec_c']) for t in range(T)]


def _item_shifted_keeps(seed, B, T, p_att, p_dec):
    """mutation: the masks of item b taken at idx = (b + 1) * 1024 + u (B + 1 <= 16: one chunk, one seed)"""
    k = R.decoder_state_keeps(seed, 0, B + 1, T, p_att, p_dec)
    return [{n: m[1:] for n, m in k[t].items()} for t in range(T)]


KEEPS = {'correct': _correct_keeps, 'c-shifted': _c_shifted_keeps, 'item-shifted': _item_shifted_keeps}


@functools.lru_cache(maxsize=3)
def _oracle(shape, p_att, p_dec, keeps='correct'):
    """fp64 oracle of one case with the replayed keep-masks: (mel, gate, align, {parameter: gradient}, d memory).  Shared by the
    engines of a case (DEC_CASES keeps them next to each other) and never modified."""
    import t2v_oracle as O
    hp, M, dec, memory, mels, lengths, wm, wg = _setup(shape)
    B, T = memory.shape[0], mels.shape[2]
    sd = {'decoder.' + k: v.detach().double().requires_grad_(True) for k, v in dec.state_dict().items()}
    mem = memory.double().requires_grad_(True)
    drop = {'lstm': KEEPS[keeps](_call_seed(dec), B, T, p_att, p_dec)}
    mel, gate, align = O.decoder_forward(sd, mem, mels.double(), lengths, p_att=p_att, p_dec=p_dec, drop=drop)
    ((mel * wm.double()).sum() + (gate * wg.double()).sum()).backward()
    grads = {k[len('decoder.'):]: v.grad for k, v in sd.items()}
    return mel.detach(), gate.detach(), align.detach(), grads, mem.grad


def _device(shape, p_att, p_dec, engine, monkeypatch, keep_last=False):
    """the HIP decoder on the same inputs: (mel, gate, align, {parameter: gradient}, d memory) on the host, + the saved XS"""
    import model as M
    import t2v_hip
    fwd, bwd, fwd_mode, bwd_mode = ENGINES[engine]
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent', fwd)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent_bwd', bwd)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'keep_last', keep_last)
    for name in ('last_call', 'last_persist', 'last_bwd', 'last_bwd_persist'):
        monkeypatch.setattr(t2v_hip.DecoderCore, name, None)
    hp, M, dec, memory, mels, lengths, wm, wg = _setup(shape)
    dev = torch.device('cuda:0')
    dec = dec.to(dev).train()
    dec.p_attention_dropout, dec.p_decoder_dropout = p_att, p_dec
    dec._calls = 0
    mem = memory.to(dev).requires_grad_(True)
    mel, gate, align = dec(mem, mels.to(dev), lengths.to(dev))
    assert t2v_hip.DecoderCore.last_mode == fwd_mode
    XS = t2v_hip.DecoderCore.last_call[3][4].cpu() if keep_last else None
    ((mel * wm.to(dev)).sum() + (gate * wg.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert t2v_hip.DecoderCore.last_bwd_mode == bwd_mode
    assert all(p.grad is not None for p in dec.parameters())
    grads = {n: p.grad.cpu() for n, p in dec.named_parameters()}
    return mel.detach().cpu(), gate.detach().cpu(), align.detach().cpu(), grads, mem.grad.cpu(), XS


def _worst(dev, ref):
    """largest |dev - ref| and where"""
    d = (dev.double() - ref).abs()
    i = int(d.argmax())
    return d.flatten()[i].item(), tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))


def _grad_rel(dev, ref):
    """as test_decoder_core_matches_oracle: the largest difference relative to the largest reference entry; a reference
    gradient that is identically zero is compared absolutely (d / 1e-3 < 2e-3  <=>  d < 2e-6)"""
    d, where = _worst(dev, ref)
    s = ref.abs().max().item()
    return (d / (s + 1e-6) if s > 0 else d / 1e-3), where


# --------------------------------------------------------------------------------------------- (a) replica == device
CONV_SEED, CONV_STREAM, CONV_T = 0x5DEECE66D1234567 & SEED_MASK, 3, 11


def _conv_inputs(B, Cin, Cout, T, KS):
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    wo = torch.randn(B, Cout, T, generator=g)
    return x, w, b, gamma, beta, wo


@pytest.mark.parametrize("B,Cin,Cout,T,KS", [(2, 33, 70, 129, 3), (1, 64, 64, 2, 5)])
def test_conv_bn_act_draws_the_replicas_mask(B, Cin, Cout, T, KS):
    """act = none: a kept element is gamma * xhat + beta, never exactly 0 — the zeros of the output are the dropped elements"""
    import t2v_hip
    x, w, b, gamma, beta, _ = _conv_inputs(B, Cin, Cout, T, KS)
    dev = 'cuda'
    out = t2v_hip.ConvBNAct1d.apply(x.to(dev), w.to(dev), b.to(dev), gamma.to(dev), beta.to(dev), torch.zeros(Cout, device=dev),
                                    torch.ones(Cout, device=dev), True, t2v_hip.ACT_NONE, 0.5, CONV_SEED, CONV_STREAM, CONV_T)
    keep = R.conv_keep(CONV_SEED, CONV_STREAM, CONV_T, B, Cout, T, 0.5)
    assert torch.equal(out.cpu() == 0, ~keep)
    # and the mask follows stream and t
    assert not torch.equal(keep, R.conv_keep(CONV_SEED, CONV_STREAM + 1, CONV_T, B, Cout, T, 0.5))
    assert not torch.equal(keep, R.conv_keep(CONV_SEED, CONV_STREAM, CONV_T + 1, B, Cout, T, 0.5))


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_decoder_draws_the_replicas_h_masks(engine, monkeypatch):
    """the saved rows XS[t + 1][:, :1024] = h_att(t) and XS[t + 2][:, 1536:] = h_dec(t) are zero exactly where the replica drops
    (o * tanh(c) of a kept unit is not 0).  The c masks cannot be seen in the arena (CA / CD hold the cells before dropout):
    test_decoder_state_dropout_matches_oracle ties them down."""
    p_att, p_dec = 0.5, 0.25
    B, T_in, T, _ = DEC_SHAPES[0]
    XS = _device(0, p_att, p_dec, engine, monkeypatch, keep_last=True)[5]
    dec = _setup(0)[2]
    keeps = R.decoder_state_keeps(_call_seed(dec), 0, B, T, p_att, p_dec)
    att_h = torch.stack([k['att_h'] for k in keeps])
    dec_h = torch.stack([k['dec_h'] for k in keeps])
    assert XS.shape == (T + 2, B, 2560)
    assert torch.equal(XS[1:T + 1, :, :1024] == 0, ~att_h)
    assert torch.equal(XS[2:T + 2, :, 1536:] == 0, ~dec_h)


# --------------------------------------------------------------------------------------------- (b) decoder core
@pytest.mark.parametrize("shape,p_att,p_dec,engine", DEC_CASES,
                         ids=['B%d-Tin%d-T%d-p%g-%g-%s' % (DEC_SHAPES[s][:3] + (pa, pd, e)) for s, pa, pd, e in DEC_CASES])
def test_decoder_state_dropout_matches_oracle(shape, p_att, p_dec, engine, monkeypatch):
    """mel / gate within 2e-4 / (1 - p), alignments within 2e-5 / (1 - p), every parameter gradient and d memory within 2e-3 of
    the tensor's largest reference entry.  One wrong mask bit moves a state element by |h| / (1 - p) ~ 0.1."""
    o_mel, o_gate, o_align, o_grads, o_dmem = _oracle(shape, p_att, p_dec)
    mel, gate, align, grads, dmem, _ = _device(shape, p_att, p_dec, engine, monkeypatch)
    scale = 1.0 / (1.0 - max(p_att, p_dec))
    fwd = {'mel': (mel, o_mel, 2e-4 * scale), 'gate': (gate, o_gate, 2e-4 * scale), 'align': (align, o_align, 2e-5 * scale)}
    report, failed = [], []
    for name, (d, r, bound) in fwd.items():
        err, where = _worst(d, r)
        report.append('%s %.2e / %.1e at %s' % (name, err, bound, where))       # mel (b, channel, t), gate (b, t), align (b, t, j)
        if not err < bound:
            failed.append(report[-1])
    worst = (-1.0, None, None)
    for name, d in list(grads.items()) + [('d_memory', dmem)]:
        rel, where = _grad_rel(d, o_dmem if name == 'd_memory' else o_grads[name])
        if rel > worst[0]:
            worst = (rel, name, where)
        if not rel < 2e-3:
            failed.append('grad %s %.2e / 2e-3 at %s' % (name, rel, where))
    report.append('worst gradient %.2e / 2e-3 (%s at %s)' % worst)
    print('dropout parity B=%d T_in=%d T=%d p=(%g, %g) %s: ' % (DEC_SHAPES[shape][:3] + (p_att, p_dec, engine)) + '; '.join(report))
    assert not failed, failed


# --------------------------------------------------------------------------------------------- (c) the test sees the slips
@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("mutation", ['c-shifted', 'item-shifted'])
def test_wrong_masks_in_the_oracle_are_seen(mutation, engine, monkeypatch):
    """CPU-side mutations of the REFERENCE (nothing in the kernels is altered): against an oracle whose c masks come from the next
    step, or whose masks are indexed with the next item, the device's d memory and attention_rnn.weight_hh gradient are off by
    more than 10 times the bound of test_decoder_state_dropout_matches_oracle."""
    p = 0.1
    o_grads, o_dmem = _oracle(0, p, p, mutation)[3:]
    grads, dmem = _device(0, p, p, engine, monkeypatch)[3:5]
    rel_mem = _grad_rel(dmem, o_dmem)[0]
    rel_whh = _grad_rel(grads['attention_rnn.weight_hh'], o_grads['attention_rnn.weight_hh'])[0]
    print('mutation %s, %s: d_memory off by %.2e, attention_rnn.weight_hh by %.2e (bound of the parity test 2e-3)' % (
        mutation, engine, rel_mem, rel_whh))
    assert rel_mem > 10 * 2e-3, rel_mem
    assert rel_whh > 10 * 2e-3, rel_whh


# --------------------------------------------------------------------------------------------- (d) ConvBNAct1d
@functools.lru_cache(maxsize=None)
def _conv_reference(B, Cin, Cout, T, KS, act):
    """fp64: act(BatchNorm_train(conv1d(x))) * keep / (1 - p) and the gradients of sum(y * wo)"""
    x, w, b, gamma, beta, wo = _conv_inputs(B, Cin, Cout, T, KS)
    cx, cw, cb, cg, cbt = (t.double().requires_grad_(True) for t in (x, w, b, gamma, beta))
    y = F.batch_norm(F.conv1d(cx, cw, cb, padding=KS // 2), None, None, cg, cbt, True, 0.0, 1e-5)
    y = torch.tanh(y) if act == 1 else F.relu(y) if act == 2 else y
    keep = R.conv_keep(CONV_SEED, CONV_STREAM, CONV_T, B, Cout, T, 0.5)
    y = y * keep.double() / (1.0 - 0.5)
    (y * wo.double()).sum().backward()
    return y.detach(), {'dx': cx.grad, 'dw': cw.grad, 'dgamma': cg.grad, 'dbeta': cbt.grad}


@pytest.mark.parametrize("x3_mode", [None, 1], ids=['conv-default', 'conv-x3'])
@pytest.mark.parametrize("act", [0, 1, 2], ids=['none', 'tanh', 'relu'])
@pytest.mark.parametrize("B,Cin,Cout,T,KS", [(2, 33, 70, 129, 3), (1, 64, 64, 2, 5), (3, 512, 80, 37, 5)])
def test_conv_bn_act_dropout_matches_fp64(B, Cin, Cout, T, KS, act, x3_mode):
    """output within 2e-4 * 2 (the 1 / (1 - p) scale), dx / dw / dgamma / dbeta within 2e-3 of the largest reference entry — the
    backward regenerates the mask (bn_act.hip: k_bn_act_bwd); once with the default convolution form and once with the x3 form
    wherever the shape allows it (its epilogue emits the BatchNorm partial sums)"""
    import t2v_hip
    lib = t2v_hip.load_library()
    ref, ref_grads = _conv_reference(B, Cin, Cout, T, KS, act)
    x, w, b, gamma, beta, wo = _conv_inputs(B, Cin, Cout, T, KS)
    dev = 'cuda'
    gx, gw, gb, gg, gbt = (t.clone().to(dev).requires_grad_(True) for t in (x, w, b, gamma, beta))
    prev = lib.t2v_conv1d_x3_set_mode(-1 if x3_mode is None else x3_mode)
    try:
        out = t2v_hip.ConvBNAct1d.apply(gx, gw, gb, gg, gbt, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev),
                                        True, act, 0.5, CONV_SEED, CONV_STREAM, CONV_T)
        (out * wo.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)
    err, where = _worst(out.detach().cpu(), ref)
    report = ['out %.2e / 4e-4' % err]
    failed = [] if err < 2e-4 * 2 else ['out %.2e at %s' % (err, where)]
    for name, a in (('dx', gx.grad), ('dw', gw.grad), ('dgamma', gg.grad), ('dbeta', gbt.grad)):
        r = ref_grads[name]
        d, where = _worst(a.cpu(), r)
        scale = r.abs().max().item() + 1e-6
        report.append('%s %.2e / 2e-3' % (name, d / scale))
        if not d < 2e-3 * scale:
            failed.append('%s %.2e of %.2e at %s' % (name, d, scale, where))
    print('conv dropout parity B=%d %d->%d T=%d k=%d act=%d x3=%s: ' % (B, Cin, Cout, T, KS, act, x3_mode) + '; '.join(report))
    assert not failed, failed
