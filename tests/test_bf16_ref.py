"""tests/bf16_ref.py on the reference alone: no GPU.  What makes tests/test_decoder_bf16_stepwise_gpu.py mean something:

derivation   with Q = identity in float64, each step fed by the reference's own previous step, forward() reproduces
             oracle/t2v_oracle.py::decoder_forward and reverse() the autograd gradients of the same loss — DGA and DGD (the gradients
             of the gate pre-activations), DCTX, the sum of dpre over the steps (d pm), dq through d W_q, d memory and the LSTM
             weight gradients that are products of DGA — at 1e-10 class, state dropout on.  This proves the hand-derived reverse pass.
fake arena   a stand-in for a correct kernel: the reference chained in float32 with Q on, the arithmetic a correct bf16 engine
             performs.  The local check passes on it at the bound of the GPU test, K * max(floor, 4 * 2^-24 * scale) with K = 16 ...
mutations    ... and under every mutation of bf16_ref.MUTATIONS each quantity the mutation must move stands at least 4 x over that
             bound, on every case of the GPU test (T_in = 1 excepted where said: a one-position softmax is constant, so the
             alignment is 1 and nothing flows through the attention's backward).  The factors are printed (pytest -s).
"""
import functools

import pytest
import torch

import bf16_ref as R

F32, F64 = torch.float32, torch.float64
SEED = 0x5DEECE66D1234567 & 0x7FFFFFFFFFFFFFFF
SHARP = 4.0


@functools.lru_cache(maxsize=None)
def _decoder():
    import hparams as HP
    import model as M
    old = M.drop_rate
    try:
        torch.manual_seed(0)
        return M.Decoder(HP.create_hparams("bf16_run=True"))
    finally:
        M.drop_rate = old


def _sd(dec, dtype):
    return {'decoder.' + k: v.detach().to(dtype) for k, v in dec.state_dict().items()}


def _loss_weights(case):
    B, _, T, _ = case
    g = torch.Generator().manual_seed(7)
    return torch.randn(B, 80, T, generator=g, dtype=F64), torch.randn(B, T, generator=g, dtype=F64)


def _filled_arena(case, dtype):
    """inputs of the loop, computed in float64 from the decoder's parameters: gpre (no Prenet dropout), pm, and dHC of the loss
    sum(mel * wm) + sum(gate * wg), which is linear in [h_dec | ctx]: dHC[t] = wm[:, :, t] W_proj + wg[:, t] W_gate"""
    import t2v_oracle as O
    B, T_in, T, _ = case
    dec = _decoder()
    sd = _sd(dec, F64)
    memory, mels, lengths = R.case_inputs(case)
    a = R.empty_arena(B, T_in, T, dtype)
    inp = torch.cat((torch.zeros(1, B, 80, dtype=F64), mels.double().permute(2, 0, 1)), 0)[:T]
    pre = O.prenet_forward(sd, inp, None, 0.0)
    w_ih = sd['decoder.attention_rnn.weight_ih']
    a['gpre'].copy_(pre @ w_ih[:, :R.PRE].t() + sd['decoder.attention_rnn.bias_ih'] + sd['decoder.attention_rnn.bias_hh'])
    a['memory'].copy_(memory)
    a['pm'].copy_(a['memory'].double() @ sd['decoder.attention_layer.memory_layer.linear_layer.weight'].t())
    a['lengths'] = lengths
    wm, wg = _loss_weights(case)
    a['dHC'].copy_(wm.permute(2, 0, 1) @ sd['decoder.linear_projection.linear_layer.weight'] +
                   wg.t()[:, :, None] * sd['decoder.gate_layer.linear_layer.weight'][0])
    return a, pre


# ------------------------------------------------------------------------------------------------ derivation
@pytest.mark.parametrize("case", [(3, 20, 5, True), (2, 1, 3, False)], ids=R.case_id)
def test_identity_reference_is_the_oracle_and_its_autograd(case):
    import t2v_oracle as O
    B, T_in, T, _ = case
    dec = _decoder()
    w = {k: v.double() for k, v in R.weights(dec).items()}
    w['bias_dec'] = (dec.decoder_rnn.bias_ih.detach().double() + dec.decoder_rnn.bias_hh.detach().double())
    a, pre = _filled_arena(case, F64)
    keeps = R.drop_ref.decoder_state_keeps(SEED, 0, B, T, R.P_DROP, R.P_DROP)
    fac = R.factors(SEED, B, T, R.P_DROP, R.P_DROP, exact=True)
    R.forward(w, a, fac, F64, R.identity, chain=True)
    R.reverse(w, a, fac, F64, R.identity, chain=True)

    # the oracle, step by step, with the gate pre-activations' biases as per-step leaves: their gradients are DGA / DGD
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd(dec, F64).items()}
    mem = a['memory'].clone().requires_grad_(True)
    st = O.decoder_init(sd, mem, R._mask(a['lengths'], T_in))
    st.pm.retain_grad()
    wm, wg = _loss_weights(case)
    ba, bd, ctxs, loss, aligns = [], [], [], 0.0, []
    for t in range(T):
        sd_t = dict(sd)
        ba.append(sd['decoder.attention_rnn.bias_ih'].detach().expand(B, -1).clone().requires_grad_(True))
        bd.append(sd['decoder.decoder_rnn.bias_ih'].detach().expand(B, -1).clone().requires_grad_(True))
        sd_t['decoder.attention_rnn.bias_ih'], sd_t['decoder.decoder_rnn.bias_ih'] = ba[-1], bd[-1]
        mel, gate, al = O.decoder_step(sd_t, st, pre[t], R.P_DROP, R.P_DROP, keeps[t])
        st.ctx.retain_grad()
        ctxs.append(st.ctx)
        aligns.append(al)
        loss = loss + (mel * wm[:, :, t]).sum() + (gate[:, 0] * wg[:, t]).sum()
        # forward: the chained reference wrote the oracle's state
        for name, mine, ref in (('h_att', a['XS'][t + 1][:, :R.H], st.h_att), ('ctx', a['XS'][t + 1][:, R.H:R.KATT], st.ctx),
                                ('h_dec', a['XS'][t + 2][:, R.KATT:], st.h_dec), ('AL', a['AL'][t + 1], st.alpha),
                                ('ACUM', a['ACUM'][t + 1], st.alpha_cum)):
            assert (mine - ref.detach()).abs().max().item() < 1e-12, (name, t)
    # ... which is decoder_forward's
    o_mel, o_gate, o_align = O.decoder_forward(_sd(dec, F64), a['memory'], R.case_inputs(case)[1].double(), a['lengths'],
                                               R.P_DROP, R.P_DROP, drop={'lstm': keeps}, p_prenet=0.0)
    assert (torch.stack(aligns, 1) - o_align).abs().max().item() < 1e-12
    loss.backward()
    worst = {}

    def close(name, mine, ref):
        scale = max(ref.abs().max().item(), 1e-30)
        worst[name] = max(worst.get(name, 0.0), (mine - ref).abs().max().item() / scale)
        assert worst[name] < 1e-10, (name, worst[name])

    for t in range(T):
        close('DGA', a['DGA'][t], ba[t].grad)
        close('DGD', a['DGD'][t], bd[t].grad)
        close('DCTX', a['DCTX'][t], ctxs[t].grad)
    xs_prev = a['XS'][:T].reshape(T * B, R.XW)
    if T_in > 1:        # (one position: the softmax is constant and these are identically zero on both sides)
        close('d_pm = sum of dpre', a['DPRE'].sum(0), st.pm.grad)
        close('d_wq = dq^T h_att', a['DQ'].reshape(T * B, R.A).t() @ a['XS'][1:T + 1, :, :R.H].reshape(T * B, R.H),
              sd['decoder.attention_layer.query_layer.linear_layer.weight'].grad)
    else:
        assert a['DPRE'].abs().max().item() == 0 and st.pm.grad.abs().max().item() < 1e-18
    close('d_memory', torch.einsum('tbj,tbe->bje', a['AL'][1:], a['DCTX']) +
          a['DPRE'].sum(0) @ sd['decoder.attention_layer.memory_layer.linear_layer.weight'].detach(), mem.grad)
    close('d_w_hh_att', a['DGA'].reshape(T * B, R.G4).t() @ xs_prev[:, :R.H], sd['decoder.attention_rnn.weight_hh'].grad)
    close('d_w_ih_att[ctx]', a['DGA'].reshape(T * B, R.G4).t() @ xs_prev[:, R.H:R.KATT], sd['decoder.attention_rnn.weight_ih'].grad[:, R.PRE:])
    close('d_w_ih_dec', a['DGD'].reshape(T * B, R.G4).t() @ a['XS'][1:T + 1].reshape(T * B, R.XW)[:, :R.KATT], sd['decoder.decoder_rnn.weight_ih'].grad)
    close('d_w_hh_dec', a['DGD'].reshape(T * B, R.G4).t() @ a['XS'][1:T + 1].reshape(T * B, R.XW)[:, R.KATT:], sd['decoder.decoder_rnn.weight_hh'].grad)
    print('derivation %s: largest relative differences %s' % (R.case_id(case), ', '.join('%s %.1e' % kv for kv in worst.items())))


def test_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -7 - 2.0 ** -20), 0.0])
    # ties go to the even bf16 neighbour; anything past the tie rounds up; truncation drops towards zero
    assert R.rne(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 0.0]
    assert R.truncate(x).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -1.0, 0.0]
    assert R.rne(x.double()).dtype == F64 and torch.equal(R.rne(x.double()), R.rne(x).double())
    f = R.factors(SEED, 3, 2, 0.1, 0.0)
    assert set(f['att_h'].unique().tolist()) == {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1)))}
    assert torch.equal(f['dec_c'], torch.ones(2, 3, 1024))


# ------------------------------------------------------------------------------------------------ fake arena, mutations
@functools.lru_cache(maxsize=1)
def _fake(case):
    """the arena a correct bf16 engine would leave: the reference chained in float32 with Q = rne.  + weights, factors"""
    B, _, T, _ = case
    w = R.weights(_decoder())
    a, _ = _filled_arena(case, F32)
    fac = R.factors(SEED, B, T, R.P_DROP, R.P_DROP)
    R.forward(w, a, fac, F32, R.rne, chain=True)
    R.reverse(w, a, fac, F32, R.rne, chain=True)
    return w, a, fac


@functools.lru_cache(maxsize=2)
def _judged(case, which):
    """(saved quantities, floors) of the fake arena for one pass"""
    w, a, fac = _fake(case)
    saved = R.saved_forward(a) if which == 'fwd' else R.saved_reverse(a)
    ref64 = R.run(which, w, a, fac, F64, R.rne)
    floors = R.floor(R.run(which, w, a, fac, F32, R.rne), ref64)
    return saved, ref64, floors


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_local_check_passes_on_a_float32_chained_reference(case):
    for which in ('fwd', 'bwd'):
        saved, ref64, floors = _judged(case, which)
        res = R.worst(R.compare(saved, ref64, floors))
        print('\n'.join(R.table('fake arena %s %s' % (R.case_id(case), which), res)))
        over = {q: v for q, v in res.items() if not v[0] < 1}
        assert not over, over


def moved_quantities(case, mutation):
    """the quantities a mutation must move at this case's shape (R.MUTATIONS, minus what a one-position softmax keeps constant)"""
    which, moved = R.MUTATIONS[mutation]
    if case[1] == 1:
        moved = tuple(q for q in moved if q not in ('AL', 'dpre', 'dq'))
    return which, moved


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_mutation_stands_over_the_bound(case):
    w, a, fac = _fake(case)
    weak = []
    for mutation in R.MUTATIONS:
        which, moved = moved_quantities(case, mutation)
        if not moved:
            continue
        saved, _, floors = _judged(case, which)
        res = R.worst(R.compare(saved, R.run(which, w, a, fac, F64, R.rne, mutation), floors))
        print('mutation %-24s %s: %s' % (mutation, R.case_id(case), ', '.join('%s %.3g x bound' % (q, res[q][0]) for q in moved)))
        weak += [(mutation, q, res[q][0]) for q in moved if not res[q][0] > SHARP]
    assert not weak, weak
