"""One decoder time step at a time, with the bf16 engines' rounding points — TEST INFRASTRUCTURE, NOT PRODUCT.

The teacher-forced decoder saves everything a step reads and writes (include/t2vae.h: t2v_dec_train_bufs XS, CA, CD, GA, GD, AL,
ACUM, S; the reverse pass DGA, DGD, DCTX and dpre in S), so a step can be checked LOCALLY: the reference below is fed the saved
fp32 state of step t - 1 (t + 1 in the reverse pass), rounds it to bf16 exactly where the contract says a bf16_run kernel rounds,
computes step t in the dtype it is asked for and is compared with what was saved for step t.  The inputs are bit-identical and
round-to-nearest-even of an fp32 value is deterministic: no rounding boundary is crossed differently, nothing is carried from
step to step, and what remains is fp32 accumulation order and the ~1e-7 absolute error of sigmoidf_ / tanhf_.

The contract (include/t2vae.h, the headers of csrc/decoder_train_persist16.hip and csrc/decoder_train_bwd_persist16.hip):
  * LSTM weights are rounded to bf16 (RNE);
  * the recurrent-state operands [h_att | ctx | h_dec] are rounded to bf16 in front of every LSTM product — the SAVED rows of XS,
    i.e. h after its dropout factor (k_lstm_fwd256<true> reads XS, k_dec_train_persist16 packs `hd`), ctx as the attention wrote it;
  * gate gradients and the transposed LSTM weights are rounded to bf16 in front of every reverse-pass product;
  * fp32: accumulation, the cell state (saved BEFORE its dropout factor; the factor of step t - 1 is applied when step t reads it),
    all of the attention (the query reads h_att in fp32) and its backward, W_q^T dq, every saved activation and gradient;
  * gpre and dHC are inputs of the loop: taken from the kept buffers.

Q is that rounding (rne) or the identity (the fp32 engines).  forward() / reverse() walk the steps; with chain=False (the check)
every stage of every step reads the arena, with chain=True a stage reads what the reference itself produced and the results are
written back into the arena — the derivation test (float64, identity) and the stand-in for a correct kernel (float32, rne) of
tests/test_bf16_ref.py.  Three linear chains that no buffer saves per step are carried by reverse() itself in its own dtype: the
two cell-state gradients and the cumulative-weights gradient; they are contractions or plain sums and cross no bf16 rounding.

floor(): the reference in float32 minus the reference in float64 on the same saved inputs, per case and quantity (the largest
difference over the steps) — the round-off of the arithmetic itself, measured on the reference and never on the kernels (the
idea of steer_ref.floor).  A bound is K * max(floor, 4 * 2^-24 * scale) with the scale of the step that is judged.
MUTATIONS: one way each in which a kernel can break the contract, applied to the reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

import drop_ref

H, E, A, PRE, G4, XW, KATT = 1024, 512, 128, 256, 4096, 2560, 1536
F32, F64 = torch.float32, torch.float64
ULP4 = 4.0 * 2.0 ** -24
K = 16.0

FWD_QUANTITIES = ('GA', 'CA', 'h_att', 'S', 'AL', 'ACUM', 'ctx', 'GD', 'CD', 'h_dec')
BWD_QUANTITIES = ('DGD', 'DCTX', 'dpre', 'dq', 'DGA')

# name -> (pass, the quantities it must move).  See _Weights / forward / reverse for what each one does.
MUTATIONS = {
    'state_not_rounded': ('fwd', ('GD',)),          # h_dec goes into W_hh_dec · h_dec unrounded
    'weights_truncated': ('fwd', ('GA', 'GD')),     # bf16 weights by truncation, not RNE
    'k_block_dropped': ('fwd', ('GA',)),            # W_hh_att · h_att without columns 64..95 for the units 8..15
    'h_dec_one_row_late': ('fwd', ('GD',)),         # decoder_rnn reads h_dec of step t - 2
    'query_from_rounded_h': ('fwd', ('S', 'AL')),   # q = W_q · Q(h_att)
    'gate_grads_not_rounded': ('bwd', ('DGD', 'DCTX', 'DGA')),
    'row_quarter_dropped': ('bwd', ('DGA',)),       # W_hh_att^T dga(t+1): units 256..511 missing in the columns 0..127
    'no_cumulative_return': ('bwd', ('dpre', 'dq')),    # the location filter sends nothing back through the cumulative channel
}


def rne(x):
    """fp32 -> bf16 (round to nearest even) -> back, in x's dtype"""
    return x.float().bfloat16().to(x.dtype)


def truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def identity(x):
    return x


def weights(dec):
    """the decoder's parameters as the fp32 tensors the kernels read ({name: CPU tensor}), from a model.Decoder"""
    sd = {k: v.detach().float().cpu() for k, v in dec.state_dict().items()}
    return {'w_ih_att': sd['attention_rnn.weight_ih'], 'w_hh_att': sd['attention_rnn.weight_hh'],
            'w_ih_dec': sd['decoder_rnn.weight_ih'], 'w_hh_dec': sd['decoder_rnn.weight_hh'],
            'bias_dec': sd['decoder_rnn.bias_ih'] + sd['decoder_rnn.bias_hh'],          # summed in fp32, as Decoder._param_operands
            'wq': sd['attention_layer.query_layer.linear_layer.weight'],
            'loc_conv': sd['attention_layer.location_layer.location_conv.conv.weight'],
            'loc_dense': sd['attention_layer.location_layer.location_dense.linear_layer.weight'],
            'v': sd['attention_layer.v.linear_layer.weight'][0]}


class _Weights(object):
    """the operands of one reference run: LSTM weights through Q (or truncated), everything in `dtype`"""

    def __init__(self, w, dtype, Q, mutation):
        q = truncate if mutation == 'weights_truncated' else Q
        d = lambda x: x.to(dtype)
        self.a_ctx = d(q(w['w_ih_att'][:, PRE:]))       # (4096, 512)
        self.a_hh = d(q(w['w_hh_att']))                 # (4096, 1024)
        self.d_ih = d(q(w['w_ih_dec']))                 # (4096, 1536) [h_att | ctx]
        self.d_hh = d(q(w['w_hh_dec']))
        self.bias_dec, self.wq, self.v = d(w['bias_dec']), d(w['wq']), d(w['v'])
        self.loc_conv, self.loc_dense = d(w['loc_conv']), d(w['loc_dense'])


def factors(seed, B, T, p_att, p_dec, exact=False):
    """the fp32 dropout factors the kernels draw (t2v_drop_scale: 0 or 1 / (1 - p) in fp32): {name: (T, B, 1024) float32}.
    exact: 1 / (1 - p) in float64, the factor of the oracle's _apply_keep (the derivation test)."""
    keeps = drop_ref.decoder_state_keeps(seed, 0, B, T, p_att, p_dec)
    out = {}
    for name, p in (('att_h', p_att), ('att_c', p_att), ('dec_h', p_dec), ('dec_c', p_dec)):
        keep = torch.stack([k[name] for k in keeps])
        if exact:
            out[name] = keep.to(F64) / (1.0 - p)
        else:
            f = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if np.float32(p) > 0 else 1.0
            out[name] = keep.to(F32) * f
    return out


# (B, T_in, T, ragged): B <= 16 (the first chunk is what DecoderCore keeps), T small (every step is checked alike).
# 7 / 3 / 9 items: lanes without an item; T_in = 1: a one-position softmax; 200: 96-position reverse slices from 193 symbols; 225 and
# 555: the long attention form; T = 40: a step index well past any ring or parity period of the persistent kernels.
CASES = ((16, 84, 12, False), (7, 40, 9, True), (3, 16, 6, True), (9, 1, 4, False), (16, 200, 6, True), (16, 225, 5, True),
         (16, 555, 4, True), (16, 84, 40, False))
P_DROP = 0.1
MEMORY_GAIN = 0.5           # memory = 0.5 * randn, the inputs of tests/test_decoder_persist16_gpu.py


def case_id(case):
    return 'B%d-Tin%d-T%d' % case[:3]


def case_lengths(case):
    B, T_in, _, ragged = case
    return [max(1, T_in - (7 * i) % max(T_in, 1)) for i in range(B)] if ragged else [T_in] * B


def case_inputs(case):
    """(memory (B, T_in, 512), mels (B, 80, T), lengths int64 (B)) on the CPU, seeded as tests/test_decoder_persist16_gpu.py"""
    B, T_in, T, _ = case
    g = torch.Generator().manual_seed(1)
    memory = torch.randn(B, T_in, 512, generator=g) * MEMORY_GAIN
    mels = torch.randn(B, 80, T, generator=g)
    return memory, mels, torch.tensor(case_lengths(case))


def empty_arena(B, T_in, T, dtype=F32):
    """a zeroed arena with the rows of t2v_dec_train_bufs and of the reverse pass (the inputs gpre, memory, pm, lengths, dHC are the
    caller's to fill)"""
    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    return {'gpre': z(T, B, G4), 'memory': z(B, T_in, E), 'pm': z(B, T_in, A), 'lengths': None, 'XS': z(T + 2, B, XW),
            'CA': z(T + 1, B, H), 'CD': z(T + 1, B, H), 'GA': z(T, B, G4), 'GD': z(T, B, G4), 'AL': z(T + 1, B, T_in),
            'ACUM': z(T + 1, B, T_in), 'S': z(T, B, T_in, A), 'dHC': z(T, B, H + E), 'DGA': z(T, B, G4), 'DGD': z(T, B, G4),
            'DPRE': z(T, B, T_in, A), 'DCTX': z(T, B, E), 'DQ': z(T, B, A)}


def _cell(pre, c_prev, f_h):
    """gate activations (B, 4096), the cell before its dropout factor, h behind its factor"""
    i, f, g, o = pre[:, :H], pre[:, H:2 * H], pre[:, 2 * H:3 * H], pre[:, 3 * H:]
    i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
    c = f * c_prev + i * g
    return torch.cat((i, f, g, o), 1), c, o * torch.tanh(c) * f_h


def _mask(lengths, T_in):
    return torch.arange(T_in)[None, :] >= lengths.long()[:, None] if lengths is not None else None


def forward(w, arena, fac, dtype, Q, chain=False, mutation=None, steps=None):
    """Steps 0 .. T - 1 of the forward pass.  arena: {'gpre', 'memory', 'pm', 'lengths', 'XS', 'CA', 'CD', 'GA', 'GD', 'AL', 'ACUM',
    'S'} of CPU fp32 tensors laid out as t2v_dec_train_bufs.  Returns {quantity: [tensor per step]} in `dtype`:
    GA, GD (B, 4096); CA = CA[t+1], CD = CD[t+1], h_att = XS[t+1][:, :1024], h_dec = XS[t+2][:, 1536:] (B, 1024);
    ctx = XS[t+1][:, 1024:1536]; S (B, T_in, 128); AL = AL[t+1], ACUM = ACUM[t+1] (B, T_in).  chain: written back."""
    W = _Weights(w, dtype, Q, mutation)
    d = lambda x: x.to(dtype)
    T, B = arena['gpre'].shape[:2]
    T_in = arena['memory'].shape[1]
    memory, pm, mask = d(arena['memory']), d(arena['pm']), _mask(arena['lengths'], T_in)
    XS, CA, CD, AL, ACUM = (arena[n] for n in ('XS', 'CA', 'CD', 'AL', 'ACUM'))
    one = torch.ones(B, H, dtype=dtype)
    out = {q: [] for q in FWD_QUANTITIES}
    for t in (range(T) if steps is None else steps):
        # ---- attention_rnn(t): reads row t = [h_att(t-1) | ctx(t-1) | .]
        h_prev, ctx_prev = d(XS[t][:, :H]), d(XS[t][:, H:KATT])
        hh = Q(h_prev) @ W.a_hh.t()
        if mutation == 'k_block_dropped':
            lost = Q(h_prev)[:, 64:96] @ W.a_hh[:, 64:96].t()
            unit = torch.zeros(H, dtype=dtype)
            unit[8:16] = 1
            hh = hh - lost * unit.repeat(4)
        pre = d(arena['gpre'][t]) + Q(ctx_prev) @ W.a_ctx.t() + hh
        ga, ca, h_att = _cell(pre, d(CA[t]) * (d(fac['att_c'][t - 1]) if t > 0 else one), d(fac['att_h'][t]))
        if chain:
            XS[t + 1][:, :H], CA[t + 1] = h_att.to(XS.dtype), ca.to(XS.dtype)
        # ---- attention(t): h_att(t) in fp32, the alignment rows t
        h_in = d(XS[t + 1][:, :H])
        q = (Q(h_in) if mutation == 'query_from_rounded_h' else h_in) @ W.wq.t()
        loc = F.conv1d(torch.stack((d(AL[t]), d(ACUM[t])), 1), W.loc_conv, None, padding=15).transpose(1, 2) @ W.loc_dense.t()
        s = torch.tanh(q[:, None, :] + loc + pm)
        e = s @ W.v
        if mask is not None:
            e = e.masked_fill(mask, -float('inf'))
        al = F.softmax(e, dim=1)
        acum = d(ACUM[t]) + al
        ctx = torch.bmm(al[:, None, :], memory).squeeze(1)
        if chain:
            AL[t + 1], ACUM[t + 1], XS[t + 1][:, H:KATT] = al.to(XS.dtype), acum.to(XS.dtype), ctx.to(XS.dtype)
            arena['S'][t] = s.to(XS.dtype)
        # ---- decoder_rnn(t): reads row t + 1 = [h_att(t) | ctx(t) | h_dec(t-1)]
        x = d(XS[t + 1][:, :KATT])
        hd_prev = d(XS[t][:, KATT:]) if mutation == 'h_dec_one_row_late' else d(XS[t + 1][:, KATT:])
        hd_op = hd_prev if mutation == 'state_not_rounded' else Q(hd_prev)
        pre = W.bias_dec + Q(x) @ W.d_ih.t() + hd_op @ W.d_hh.t()
        gd, cd, h_dec = _cell(pre, d(CD[t]) * (d(fac['dec_c'][t - 1]) if t > 0 else one), d(fac['dec_h'][t]))
        if chain:
            XS[t + 2][:, KATT:], CD[t + 1] = h_dec.to(XS.dtype), cd.to(XS.dtype)
            arena['GA'][t], arena['GD'][t] = ga.to(XS.dtype), gd.to(XS.dtype)
        for n, v in (('GA', ga), ('CA', ca), ('h_att', h_att), ('S', s), ('AL', al), ('ACUM', acum), ('ctx', ctx), ('GD', gd),
                     ('CD', cd), ('h_dec', h_dec)):
            out[n].append(v)
    return out


def saved_forward(arena, steps=None):
    """what the arena holds for the quantities of forward(), in the same form"""
    T = arena['gpre'].shape[0]
    XS = arena['XS']
    rows = {'GA': lambda t: arena['GA'][t], 'CA': lambda t: arena['CA'][t + 1], 'h_att': lambda t: XS[t + 1][:, :H],
            'S': lambda t: arena['S'][t], 'AL': lambda t: arena['AL'][t + 1], 'ACUM': lambda t: arena['ACUM'][t + 1],
            'ctx': lambda t: XS[t + 1][:, H:KATT], 'GD': lambda t: arena['GD'][t], 'CD': lambda t: arena['CD'][t + 1],
            'h_dec': lambda t: XS[t + 2][:, KATT:]}
    return {q: [rows[q](t) for t in (range(T) if steps is None else steps)] for q in FWD_QUANTITIES}


def _cell_bwd(dh, dcs, gates, c_cur, c_prev, f_h, f_c):
    """k_attn_cell_bwd / q16_cell_role: dh = gradient of h behind its dropout factor, dcs = gradient of the cell step t + 1
    read (behind the factor f_c of step t).  Returns the gate-pre-activation gradients (B, 4096) and the next dcs."""
    gi, gf, gg, go = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    dht = dh * f_h
    tc = torch.tanh(c_cur)
    dct = dcs * f_c + dht * go * (1 - tc * tc)
    dg = torch.cat((dct * gg * gi * (1 - gi), dct * c_prev * gf * (1 - gf), dct * gi * (1 - gg * gg), dht * tc * go * (1 - go)), 1)
    return dg, dct * gf


def reverse(w, arena, fac, dtype, Q, chain=False, mutation=None):
    """Steps T - 1 .. 0 of the reverse pass.  arena: the forward arena (S = the tanh outputs, i.e. cloned BEFORE the backward) +
    'dHC' (T, B, 1536), 'DGA', 'DGD' (T, B, 4096), 'DPRE' (T, B, T_in, 128) = S after the backward.  Returns {quantity: [tensor
    per step, index = t]}: DGD, DGA (B, 4096); DCTX (B, 512); dpre (B, T_in, 128); dq (B, 128).  chain: DGA, DGD, DPRE (and
    'DCTX', 'DQ') are written back."""
    W = _Weights(w, dtype, Q, mutation)
    Qg = identity if mutation == 'gate_grads_not_rounded' else Q
    d = lambda x: x.to(dtype)
    T, B = arena['gpre'].shape[:2]
    T_in = arena['memory'].shape[1]
    memory = d(arena['memory'])
    XS, CA, CD, GA, GD, AL, S = (arena[n] for n in ('XS', 'CA', 'CD', 'GA', 'GD', 'AL', 'S'))
    dHC, DGA, DGD, DPRE = (arena[n] for n in ('dHC', 'DGA', 'DGD', 'DPRE'))
    one = torch.ones(B, H, dtype=dtype)
    dcs_att = dcs_dec = torch.zeros(B, H, dtype=dtype)
    gcum = torch.zeros(B, T_in, dtype=dtype)
    out = {q: [None] * T for q in BWD_QUANTITIES}
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        f = {n: d(fac[n][t]) for n in fac}
        fc_prev = {n: (d(fac[n][t - 1]) if t > 0 else one) for n in ('att_c', 'dec_c')}
        dga_n = None if last else Qg(d(DGA[t + 1]))
        # ---- 1. decoder_rnn(t)
        dh = d(dHC[t][:, :H])
        if not last:
            dh = dh + Qg(d(DGD[t + 1])) @ W.d_hh
        dgd, dcs_dec = _cell_bwd(dh, dcs_dec, d(GD[t]), d(CD[t + 1]), d(CD[t]) * fc_prev['dec_c'], f['dec_h'], f['dec_c'])
        if chain:
            DGD[t] = dgd.to(DGD.dtype)
        # ---- 2. context
        dgd_t = Qg(d(DGD[t]))
        dctx = d(dHC[t][:, H:]) + dgd_t @ W.d_ih[:, H:]
        if not last:
            dctx = dctx + dga_n @ W.a_ctx
        # ---- 3. attention(t): what the location filter of step t + 1 sends back, softmax, tanh
        g_prev = torch.zeros(B, T_in, dtype=dtype)
        if not last:
            back = F.conv_transpose1d((d(DPRE[t + 1]) @ W.loc_dense).transpose(1, 2), W.loc_conv, None, padding=15)     # (B, 2, T_in)
            g_prev = back[:, 0]
            if mutation != 'no_cumulative_return':
                gcum = gcum + back[:, 1]
        dalpha = torch.bmm(memory, dctx[:, :, None]).squeeze(2) + g_prev + gcum
        al = d(AL[t + 1])
        de = al * (dalpha - (al * dalpha).sum(1, keepdim=True))
        s = d(S[t])
        dpre = de[:, :, None] * W.v * (1 - s * s)
        dq = dpre.sum(1)
        if chain:
            DPRE[t] = dpre.to(DGD.dtype)
            arena['DCTX'][t], arena['DQ'][t] = dctx.to(DGD.dtype), dq.to(DGD.dtype)
        # ---- 4. attention_rnn(t)
        dh = dq @ W.wq + dgd_t @ W.d_ih[:, :H]
        if not last:
            rec = dga_n @ W.a_hh
            if mutation == 'row_quarter_dropped':
                rows = torch.zeros(H, dtype=dtype)
                rows[256:512] = 1
                lost = (dga_n * rows.repeat(4)) @ W.a_hh[:, :128]
                rec = torch.cat((rec[:, :128] - lost, rec[:, 128:]), 1)
            dh = dh + rec
        dga, dcs_att = _cell_bwd(dh, dcs_att, d(GA[t]), d(CA[t + 1]), d(CA[t]) * fc_prev['att_c'], f['att_h'], f['att_c'])
        if chain:
            DGA[t] = dga.to(DGD.dtype)
        for n, v in (('DGD', dgd), ('DCTX', dctx), ('dpre', dpre), ('dq', dq), ('DGA', dga)):
            out[n][t] = v
    return out


def saved_reverse(arena):
    """what the reverse pass saved for the quantities of reverse(): needs 'DCTX' (T, B, 512) and 'DQ' (T, B, 128) as well"""
    T = arena['gpre'].shape[0]
    names = {'DGD': 'DGD', 'DCTX': 'DCTX', 'dpre': 'DPRE', 'dq': 'DQ', 'DGA': 'DGA'}
    return {q: [arena[names[q]][t] for t in range(T)] for q in BWD_QUANTITIES}


def run(which, w, arena, fac, dtype, Q, mutation=None):
    """the check: every stage of every step fed from the arena"""
    return (forward if which == 'fwd' else reverse)(w, arena, fac, dtype, Q, False, mutation)


def floor(f32_run, f64_run):
    """{quantity: largest |reference in float32 - reference in float64| over all steps}"""
    return {q: max((a.double() - b.double()).abs().max().item() for a, b in zip(f32_run[q], f64_run[q])) for q in f64_run}


def compare(saved, ref, floors):
    """[(quantity, step, error, floor, scale, bound)] with bound = K * max(floor, 4 * 2^-24 * scale), scale = the largest reference
    entry of that quantity at that step"""
    rows = []
    for q in ref:
        for t, (x, r) in enumerate(zip(saved[q], ref[q])):
            err = (x.double() - r.double()).abs().max().item()
            err = err if err == err else float('inf')           # a NaN anywhere is the worst error there is
            scale = r.abs().max().item()
            rows.append((q, t, err, floors[q], scale, K * max(floors[q], ULP4 * scale)))
    return rows


def worst(rows):
    """{quantity: (error / bound, error, floor, bound, step)} of the step with the largest error / bound (a zero bound — a
    reference that is identically zero, e.g. every gradient through a one-position softmax — passes on an exact zero only)"""
    out = {}
    for q, t, err, fl, _scale, bound in rows:
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
        if q not in out or ratio > out[q][0]:
            out[q] = (ratio, err, fl, bound, t)
    return out


def table(title, w_rows):
    return ['%s %-5s worst %.2e floor %.2e bound %.2e (%.3g of the bound) at step %d' % (title, q, e, fl, b, r, t)
            for q, (r, e, fl, b, t) in w_rows.items()]
