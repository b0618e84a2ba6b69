"""The bf16_run decoder engines, step by step, against a rounding oracle at fp32 round-off.

The four bf16 engines (k_lstm_fwd256<true> + k_attn_fwd, k_dec_train_persist16, k_lstm_bwd256<true> + k_attn_cell_bwd, k_bwd_persist16)
were only compared with each other (test_decoder_persist16_gpu.py: 1e-2 of scale, because a last-bit difference that crosses a bf16
rounding boundary is carried on by the recurrence) or with fp32 builds through statistics of a whole step.  Here every time step
is checked LOCALLY (tests/bf16_ref.py): the reference reads the kernel's own saved fp32 state of step t - 1 (t + 1 in the reverse
pass) from the kept arena, rounds it to bf16 where the contract of include/t2vae.h says the kernel rounds, computes step t in
float64 and is compared with what the kernel saved for step t.  Nothing is carried from step to step and no rounding boundary can
be crossed differently; what remains is fp32 accumulation order and the ~1e-7 absolute error of sigmoidf_ / tanhf_.

(a) parity, per engine pair a case qualifies for — bf16 with Q = RNE rounding: launch-per-step + launch-per-step, k_dec_train_persist16
    + launch-per-step, k_dec_train_persist16 + k_bwd_persist16; fp32 with Q = identity, the control on engines the suite already
    holds to the fp64 oracle: launch-per-step + launch-per-step, and persistent + one-launch reverse pass for B <= 6.  Every saved
    quantity of every step — GA, CA, h_att, S, AL, ACUM, ctx, GD, CD, h_dec; DGD, DCTX, dpre, dq, DGA — lies below
    K * max(floor, 4 * 2^-24 * scale): floor = the reference in float32 minus the reference in float64 on the same saved inputs, per
    quantity and step; scale = the largest reference entry of that quantity at that step; K = 16 as in test_decoder_steered_gpu.py,
    for its two reasons (the fast sigmoid / tanh, the summation order).  No bound is a number taken from the kernels.
    What the header leaves unwritten or fixed is checked for what it says: row 0 of XS / CA / CD / AL / ACUM and h_dec(-1) in row 1 of XS
    are zero, the attention weights and dpre of padded positions are exactly zero (S there is tanh of the energy argument like
    anywhere else and is compared); XS[T + 1][:, :1536] is never written and not looked at.
(b) the comparison of (a) against a MUTATED reference (bf16_ref.MUTATIONS: an operand not rounded, weights truncated, a k-block
    or a row quarter lost, a state row read late, the query from the rounded h, the cumulative channel's return path lost) must
    FAIL on the quantities the mutation moves — the device results of (a) are reused, nothing runs again.  tests/test_bf16_ref.py
    shows on the reference alone that each stands >= 4 x over the bound.

Every test prints worst value, floor and bound per quantity before it asserts (pytest -s); profiles/bf16_stepwise_parity.txt is that
table from an MI355X: every quantity of every engine pair below 0.52 of its bound, every mutation at least 16 bounds away.

One position (B9-Tin1-T4): the softmax is constant, the reference's dpre / dq are exactly zero, so floor = scale = 0 and the bound is
0.  The attention backward takes sum_j alpha_j dalpha_j as dctx . ctx_t + sum_j alpha_j G_j, another summation order than dalpha_0
itself, and used to leave the cancellation's round-off there (1.0e-07 .. 2.0e-07 in every engine, fp32 included); softmax_de
(csrc/t2v_common.h) now returns the exact 0 for a weight that is exactly 1, and these rows hold the kernels to it.
"""
import pytest
import torch

import bf16_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
STEPS_FWD, STEPS_BWD = 'k_lstm_fwd256 + k_attn_fwd', 'k_lstm_bwd256 + k_attn_cell_bwd'
# engine pair -> (bf16_run, DecoderCore.persistent16, .persistent, .persistent_bwd, last_kernel, last_bwd_kernel)
ENGINES = {'bf16-steps+steps': (True, False, False, False, STEPS_FWD, STEPS_BWD),
           'bf16-persist16+steps': (True, 'force', None, False, 'k_dec_train_persist16', STEPS_BWD),
           'bf16-persist16+persist16': (True, 'force', None, None, 'k_dec_train_persist16', 'k_bwd_persist16'),
           'fp32-steps+steps': (False, False, False, False, STEPS_FWD, STEPS_BWD),
           'fp32-persist+achain': (False, False, True, True, 'k_dec_train_persist', 'k_achain_bwd')}


def _engines(case):
    return [e for e in ENGINES if e != 'fp32-persist+achain' or case[0] <= 6]


QUANTITIES = R.FWD_QUANTITIES + R.BWD_QUANTITIES
RUNS = [(c, e) for c in R.CASES for e in _engines(c)]
# one test per quantity, in the order of the runs: the device result of a run is computed by its first test and kept for the rest
PARITY = [(c, e, q) for c, e in RUNS for q in QUANTITIES]
# (b): a short-form and a long-form case (16-position tiles with idle lanes; 96-position reverse slices), the bf16 engine pairs
MUTATED_CASES = (R.CASES[1], R.CASES[4])
MUTATIONS = [(m, c, e) for c in MUTATED_CASES for e in ENGINES if e.startswith('bf16') for m in R.MUTATIONS]

_DEVICE, _LAST = {}, {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    _LAST.clear()


def _dq(H, lib, kept, B, T_in, T):
    """dq(t) summed over the position slices, (T, B, 128), from what the reverse pass of the first chunk kept"""
    if H.DecoderCore.last_bwd is not None:
        return kept['DQ'][..., 0].sum(2)
    eng = H._BWD_ENGINES[H.DecoderCore.last_bwd_persist_engine]
    off, rows = getattr(lib, eng.dq_offset)(B, T_in, T), eng.dq_rows or B
    return kept['scratch'][off:off + T * rows * R.A].view(T, rows, R.A)[:, :B]


def _device(case, engine):
    """the HIP decoder on the case's inputs, state dropout on at 0.1: (weights, arena in the form of bf16_ref on the host, dropout
    factors, Q).  Kept for the cases (b) looks at again, together with what (a) judged."""
    if (case, engine) in _DEVICE:
        return _DEVICE[case, engine]
    if _LAST.get('key') == (case, engine):
        return _LAST['res']
    import hparams as HP
    import model as M
    import t2v_hip as H
    bf16, p16, persistent, persistent_bwd, kernel, bwd_kernel = ENGINES[engine]
    B, T_in, T, _ = case
    D = H.DecoderCore
    old = (M.drop_rate, D.keep_last, D.persistent, D.persistent16, D.persistent_bwd, H.bf16_enabled())
    M.drop_rate = 0.0               # Prenet dropout off (its mask is keyed by a per-call counter); the LSTM state dropout stays ON
    D.keep_last, D.persistent, D.persistent16, D.persistent_bwd = True, persistent, p16, persistent_bwd
    D.last_call = D.last_bwd = D.last_bwd_persist = None
    H.set_bf16(bf16)
    try:
        torch.manual_seed(0)
        dec = M.Decoder(HP.create_hparams("bf16_run=True") if bf16 else HP.create_hparams()).cuda().train()
        dec.p_attention_dropout = dec.p_decoder_dropout = R.P_DROP
        dec._calls = 0
        memory, mels, lengths = R.case_inputs(case)
        mem = memory.cuda().requires_grad_(True)
        mel, gate, _ = dec(mem, mels.cuda(), lengths.cuda())
        assert D.last_kernel == kernel, (D.last_kernel, kernel)
        keep, dims = D.last_call[3], D.last_call[2]
        assert dims[:5] == (B, T_in, T, R.P_DROP, R.P_DROP), dims
        names = H._ARENA
        # cloned before the backward: it overwrites S with dpre
        arena = {n: (keep[i].detach().cpu().clone() if torch.is_tensor(keep[i]) else None) for i, n in enumerate(names) if n != 'QP'}
        (mel.sum() + 0.3 * gate.sum() + 0.01 * (mel * mel).sum()).backward()
        torch.cuda.synchronize()
        H.check_async_errors()
        assert D.last_bwd_kernel == bwd_kernel, (D.last_bwd_kernel, bwd_kernel)
        if D.last_bwd is not None:          # launch-per-step: the fields of t2v_dec_bwd_bufs behind the arena
            kept = dict(zip(('dHC', 'DGA', 'DGD', 'DQ', 'DCTX'), D.last_bwd[4][len(names):]))
        else:                               # one launch: (dHC, DGA, DGD, DCTX, DV, DQP, scratch, error word)
            kept = dict(zip(('dHC', 'DGA', 'DGD', 'DCTX', 'DV', 'DQP', 'scratch'), D.last_bwd_persist[2]))
        for n in ('dHC', 'DGA', 'DGD', 'DCTX'):
            arena[n] = kept[n].detach().cpu().clone()
        arena['DQ'] = _dq(H, H.load_library(), kept, B, T_in, T).detach().cpu().clone()
        arena['DPRE'] = keep[names.index('S')].detach().cpu().clone()
        arena['lengths'] = arena['lengths'].long()
        res = {'w': R.weights(dec), 'arena': arena, 'fac': R.factors(dims[5], B, T, R.P_DROP, R.P_DROP),
               'Q': R.rne if bf16 else R.identity}
    finally:
        M.drop_rate, D.keep_last, D.persistent, D.persistent16, D.persistent_bwd = old[:5]
        H.set_bf16(old[5])
        D.last_call = D.last_bwd = D.last_persist = D.last_bwd_persist = None
    _LAST.update(key=(case, engine), res=res)
    if case in MUTATED_CASES and engine.startswith('bf16'):
        _DEVICE[case, engine] = res
    return res


def _judged(res, which):
    """(what the device saved, floors, {quantity: worst step against the float64 reference}) of one pass, once per device result"""
    if which not in res:
        w, a, fac, Q = res['w'], res['arena'], res['fac'], res['Q']
        ref64 = R.run(which, w, a, fac, F64, Q)
        saved = R.saved_forward(a) if which == 'fwd' else R.saved_reverse(a)
        floors = R.floor(R.run(which, w, a, fac, F32, Q), ref64)
        res[which] = (saved, floors, R.worst(R.compare(saved, ref64, floors)))
    return res[which]


def _fixed_rows(case, arena):
    """what the header says about rows and positions no step computes"""
    B, T_in, T, _ = case
    bad = []
    for name, x in (('XS[0]', arena['XS'][0]), ('XS[1] h_dec(-1)', arena['XS'][1][:, R.KATT:]), ('CA[0]', arena['CA'][0]),
                    ('CD[0]', arena['CD'][0]), ('AL[0]', arena['AL'][0]), ('ACUM[0]', arena['ACUM'][0])):
        if not (x == 0).all():
            bad.append(name + ' is not zero')
    pad = R._mask(arena['lengths'], T_in)                        # (B, T_in) True at padding
    for name, x in (('AL', arena['AL'][1:]), ('ACUM', arena['ACUM'][1:]), ('dpre', arena['DPRE'].abs().amax(-1))):
        if not (x[:, pad] == 0).all():
            bad.append(name + ' is not exactly zero at padded positions')
    assert arena['XS'].shape == (T + 2, B, R.XW) and arena['S'].shape == (T, B, T_in, R.A)
    return bad


# ------------------------------------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("case,engine,quantity", PARITY, ids=['%s-%s-%s' % (R.case_id(c), e, q) for c, e, q in PARITY])
def test_every_step_matches_the_rounding_oracle(case, engine, quantity):
    worst = _judged(_device(case, engine), 'fwd' if quantity in R.FWD_QUANTITIES else 'bwd')[2]
    row = R.table('stepwise %s %s' % (R.case_id(case), engine), {quantity: worst[quantity]})[0]
    print(row)
    assert worst[quantity][0] < 1, row


@pytest.mark.parametrize("case,engine", RUNS, ids=['%s-%s' % (R.case_id(c), e) for c, e in RUNS])
def test_rows_no_step_computes_are_what_the_header_says(case, engine):
    bad = _fixed_rows(case, _device(case, engine)['arena'])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (b) mutations must fail
@pytest.mark.parametrize("mutation,case,engine", MUTATIONS, ids=['%s-%s-%s' % (m, R.case_id(c), e) for m, c, e in MUTATIONS])
def test_a_mutated_reference_is_seen(mutation, case, engine):
    """CPU-side mutation of the REFERENCE; the unmutated kernels' saved values are over the bound of (a) on every quantity the
    mutation moves"""
    res = _device(case, engine)
    which, moved = R.MUTATIONS[mutation]
    saved, floors, _ = _judged(res, which)
    w, a, fac, Q = res['w'], res['arena'], res['fac'], res['Q']
    worst = R.worst(R.compare(saved, R.run(which, w, a, fac, F64, Q, mutation), floors))
    print('mutation %-24s %s %s: %s' % (mutation, R.case_id(case), engine, ', '.join('%s %.3g x bound' % (q, worst[q][0]) for q in moved)))
    assert all(worst[q][0] > 1 for q in moved), {q: worst[q] for q in moved}
