"""Step references for the cooperative recurrences outside the decoder — TEST INFRASTRUCTURE, NOT PRODUCT.

  bilstm()   nn.LSTM(512, 256, bidirectional) on a packed batch: each item over its own length, the reverse direction from
             len_b - 1, zero outputs past len_b, length 0 allowed (csrc/bilstm.hip: k_bilstm_fwd / k_bilstm_bwd)
  gru()      nn.GRU(256, 256): gates r, z, n with hn = W_hn h + b_hn kept apart, every state, and the last state or the state
             after steps[b] steps (csrc/refenc.hip, csrc/refenc_fwd.inc: k_gru_fwd / k_gru_bwd / k_gru_fwd_len)

Both are written step by step as the kernels are (the step counter runs 0 .. T - 1 in both directions; an item that has ended
keeps its state), in the dtype asked for, with the kernels' saved tensors in the kernels' layouts; gradients come from autograd.
oracle() runs one on the seeded inputs of a case and returns every quantity the device tests compare; floor() is the fp32 run
minus the fp64 run, the round-off of the arithmetic itself, which every bound of tests/test_recurrent_edges_gpu.py is a multiple
of.  A `mutation` is a one-line wrong variant that models a kernel slip; tests/test_rnn_ref.py shows on the reference alone that
each stands at least 100 bounds above the reference.

Quantities and how they are measured (compare()):
  abs     y, gates, h_last, hs, gsave (r, z, n)   largest |difference|; these are bounded by 1, scale 1
  scaled  cells, hn                               largest |difference|, scale = max |reference| (not bounded by 1: a cell state
                                                  grows with the steps, hn = W_hn h + b_hn with the weights)
  rel     dg, dgi, dgh, dx, grad                  largest |difference| / largest |reference| entry, per tensor; 'grad' is the
                                                  worst parameter gradient
"""
import collections
import functools

import torch

H = 256
ULP4 = 4.0 * 2.0 ** -24

LstmCase = collections.namedtuple('LstmCase', 'name B T lens x_scale whh_scale bias')
GruCase = collections.namedtuple('GruCase', 'name B T steps x_scale whh_scale bias')

LSTM_NAMES = tuple(n + s for s in ('', '_reverse') for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'))
GRU_NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')

LSTM_MUTATIONS = ('reverse_from_T', 'neighbour_row', 'drop_cell', 'one_unit')
GRU_MUTATIONS = ('steps_T', 'neighbour_row', 'one_unit')

KIND = {'y': 'abs', 'gates': 'abs', 'cells': 'scaled', 'dg': 'rel', 'dx': 'rel', 'grad': 'rel',
        'h_last': 'abs', 'hs': 'abs', 'gsave': 'abs', 'hn': 'scaled', 'dgi': 'rel', 'dgh': 'rel'}
ORDER = ('y', 'gates', 'cells', 'h_last', 'hs', 'gsave', 'hn', 'dg', 'dgi', 'dgh', 'dx', 'grad')


# ------------------------------------------------------------------------------------------------ cases
def _lstm(name, T, lens, x_scale=1.0, whh_scale=1.0, bias=None):
    return LstmCase(name, len(lens), T, tuple(lens), x_scale, whh_scale, bias)


def _gru(name, B, T, steps=None, x_scale=1.0, whh_scale=1.0, bias=None):
    return GruCase(name, B, T, None if steps is None else tuple(steps), x_scale, whh_scale, bias)


# unsorted, every prefix of two or more holds both 1 and T; the items a mutation acts on at step 1 (B = 5, 9, 12, 13: the last
# one) are longer than 1
_SWEEP_LENS = (1, 6, 3, 5, 2, 4, 6, 1, 4, 2, 5, 3, 4, 6, 2, 5)
_SWEEP_STEPS = (1, 5, 3, 4, 2, 5, 1, 3, 2, 4, 5, 1, 4, 2, 3, 5)
_EDGE_LENS = (4, 6, 1, 5, 2, 6, 3, 1, 5, 2, 3)             # longest 6; item 0 and the last item of B = 5 and 11 longer than 1
_ZERO_LENS = (4, 6, 0, 1, 3, 6, 2, 5, 1, 4, 2)             # one zero-length item in the middle (item 2)
_LONG_LENS = (37, 84, 1, 66, 50, 80, 2, 71, 84, 13, 60)
_SAT_LENS = (4, 9, 1, 7, 9, 2, 5, 8, 3, 6, 9, 1, 7, 2, 5, 8)

# a bias of +40 on the first 128 units of one gate block and -40 on the other 128: a whole gate at 1 or at 0.
# (parameter, gate block, magnitude): the forward direction's forget gate and the reverse direction's input gate
_LSTM_BIAS40 = (('bias_ih_l0', 1, 40.0), ('bias_ih_l0_reverse', 0, 40.0))
# past +-88.7 the kernels' exp overflows: sigmoid = rcp(1 + inf) = 0 and tanh = 1 - 2 rcp(1 + inf) = 1 must come out exact
_LSTM_BIAS100 = (('bias_ih_l0', 1, 100.0), ('bias_ih_l0', 2, 100.0), ('bias_ih_l0_reverse', 0, 100.0), ('bias_hh_l0_reverse', 3, 100.0))
_GRU_BIAS40 = (('bias_ih_l0', 1, 40.0),)                    # the update gate
# (r at 1 where z is at 0, and n left alone: otherwise no gradient would be left to compare)
_GRU_BIAS100 = (('bias_ih_l0', 0, 100.0), ('bias_hh_l0', 1, -100.0))

LSTM_SWEEP = tuple(_lstm('sweep-B%d' % B, 6, (6,) if B == 1 else _SWEEP_LENS[:B]) for B in range(1, 17))
LSTM_EDGES = tuple(c for B in (5, 11) for c in (
    _lstm('T1-B%d' % B, 1, (1,) * B),
    _lstm('T2-B%d' % B, 2, ((1, 2, 2, 1, 2) * 3)[:B]),
    _lstm('T7-all1-B%d' % B, 7, (1,) * B),
    _lstm('T9-longest6-B%d' % B, 9, _EDGE_LENS[:B]),
    _lstm('ascending-B%d' % B, 6, sorted(_SWEEP_LENS[:B])),
    _lstm('zero-length-B%d' % B, 6, _ZERO_LENS[:B]))) + (_lstm('long-T84-B11', 84, _LONG_LENS),)
LSTM_SATURATED = (_lstm('saturated-B7', 9, _SAT_LENS[:7], 6.0, 4.0), _lstm('saturated-B16', 9, _SAT_LENS, 6.0, 4.0),
                  _lstm('bias40-B7', 9, _SAT_LENS[:7], 1.0, 1.0, _LSTM_BIAS40),
                  _lstm('bias100-B7', 9, _SAT_LENS[:7], 1.0, 1.0, _LSTM_BIAS100))
LSTM_CASES = LSTM_SWEEP + LSTM_EDGES + LSTM_SATURATED

GRU_SWEEP = tuple(_gru('sweep-B%d' % B, B, 3) for B in range(1, 17))
GRU_LEN_SWEEP = tuple(_gru('len-sweep-B%d' % B, B, 5, (5,) if B == 1 else _SWEEP_STEPS[:B]) for B in range(1, 17))
GRU_EDGES = tuple(_gru('T%d-B%d' % (T, B), B, T) for B in (9, 13) for T in (1, 2, 19))
GRU_SATURATED = (_gru('saturated-B7', 7, 9, None, 6.0, 4.0), _gru('saturated-B16', 16, 9, None, 6.0, 4.0),
                 _gru('bias40-B7', 7, 9, None, 1.0, 1.0, _GRU_BIAS40), _gru('bias100-B7', 7, 9, None, 1.0, 1.0, _GRU_BIAS100))
GRU_CASES = GRU_SWEEP + GRU_LEN_SWEEP + GRU_EDGES + GRU_SATURATED


def case(name, table=None):
    for c in (table or LSTM_CASES + GRU_CASES):
        if c.name == name:
            return c
    raise KeyError(name)


# (mutation, case) pairs the device test asserts on; tests/test_rnn_ref.py shows the margin of each on the reference alone
LSTM_MUTATED = ((('reverse_from_T', case('sweep-B9', LSTM_SWEEP)), ('reverse_from_T', case('T9-longest6-B5', LSTM_EDGES)))
                + tuple(('neighbour_row', case('sweep-B%d' % B, LSTM_SWEEP)) for B in (5, 9, 12, 13))
                + (('drop_cell', case('T9-longest6-B11', LSTM_EDGES)), ('one_unit', case('T9-longest6-B11', LSTM_EDGES))))
GRU_MUTATED = (tuple(('neighbour_row', case('sweep-B%d' % B, GRU_SWEEP)) for B in (5, 9, 12, 13))
               + (('one_unit', case('sweep-B11', GRU_SWEEP)),)
               + tuple(('steps_T', c) for c in GRU_LEN_SWEEP[1:]))         # B = 1 has steps = (T,): nothing to get wrong


# ------------------------------------------------------------------------------------------------ inputs
def _split_bias(params, spec):
    for name, block, mag in spec or ():
        params[name][block * H:block * H + H // 2] = mag
        params[name][block * H + H // 2:(block + 1) * H] = -mag


def lstm_inputs(c):
    """(x (B, T, 512), wo (B, T, 512), {parameter: fp32 tensor}) of a case, seeded by its shape; nn.LSTM's initial
    distribution U(-1/16, 1/16).  x is random past each length too: nothing may read it there."""
    g = torch.Generator().manual_seed(7000 + 131 * c.B + c.T)
    k = H ** -0.5
    params = {}
    for n in LSTM_NAMES:
        shape = (4 * H, 512) if 'weight_ih' in n else (4 * H, H) if 'weight_hh' in n else (4 * H,)
        params[n] = (torch.rand(*shape, generator=g) * 2 - 1) * k
    x = torch.randn(c.B, c.T, 512, generator=g) * c.x_scale
    wo = torch.randn(c.B, c.T, 512, generator=g)
    for n in LSTM_NAMES:
        if 'weight_hh' in n:
            params[n] *= c.whh_scale
    _split_bias(params, c.bias)
    return x, wo, params


def gru_inputs(c):
    """(x (B, T, 256), wo (B, 256), {parameter: fp32 tensor}) of a case"""
    g = torch.Generator().manual_seed(9000 + 131 * c.B + c.T)
    k = H ** -0.5
    params = {}
    for n in GRU_NAMES:
        shape = (3 * H, H) if 'weight' in n else (3 * H,)
        params[n] = (torch.rand(*shape, generator=g) * 2 - 1) * k
    x = torch.randn(c.B, c.T, H, generator=g) * c.x_scale
    wo = torch.randn(c.B, H, generator=g)
    params['weight_hh_l0'] *= c.whh_scale
    _split_bias(params, c.bias)
    return x, wo, params


# ------------------------------------------------------------------------------------------------ the references
def bilstm(x, lens, params, dtype, mutation=None):
    """Returns y (B, T, 512), gates (2, B, T, 1024: i, f, g, o after their nonlinearity), cells (2, B, T, 256) and the input
    projections gx (2 x (B, T, 1024), x W_ih^T + b_ih + b_hh, in the graph: its gradient is the kernels' dg).  gates / cells
    are zero where the kernels write nothing (past each length)."""
    assert mutation is None or mutation in LSTM_MUTATIONS, mutation
    x = x.to(dtype)
    B, T, _ = x.shape
    lens = torch.as_tensor(lens, dtype=torch.long)
    rows = torch.arange(B)
    valid = (torch.arange(T)[None, :] < lens[:, None]).to(dtype)[:, :, None]            # (B, T, 1)
    ys, gates, cells, gxs = [], [], [], []
    for d, sfx in enumerate(('', '_reverse')):
        w_ih, w_hh, b_ih, b_hh = (params[n + sfx].to(dtype) for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'))
        gx = x @ w_ih.t() + b_ih + b_hh
        if gx.requires_grad:
            gx.retain_grad()
        run = torch.full_like(lens, T) if (d == 1 and mutation == 'reverse_from_T') else lens
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        ib, it, hv, gv, cv = [], [], [], [], []
        for step in range(T):
            act = step < run
            if not bool(act.any()):
                break                                               # the trailing steps change nothing
            t = (torch.full_like(run, step) if d == 0 else run - 1 - step).clamp(min=0)
            h_in, c_prev = h, c
            if mutation == 'neighbour_row' and step >= 1 and B >= 2:
                h_in = torch.cat((h[:B - 1], h[B - 2:B - 1]))       # the last item reads its neighbour's row
            if mutation == 'drop_cell' and step == 1:
                c_prev = torch.cat((torch.zeros(1, H, dtype=dtype), c[1:]))
            if mutation == 'one_unit' and step == 1 and d == 1:
                keep = torch.ones(B, H, dtype=dtype)
                keep[B - 1, H - 1] = 0
                c_prev = c * keep
            a = gx[rows, t] + h_in @ w_hh.t()
            i, f = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H])
            g, o = torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c_new = f * c_prev + i * g
            h_new = o * torch.tanh(c_new)
            m = act[:, None]
            h, c = torch.where(m, h_new, h), torch.where(m, c_new, c)       # an item that has ended keeps its state
            ib.append(rows[act])
            it.append(t[act])
            hv.append(h_new[act])
            gv.append(torch.cat((i, f, g, o), 1)[act].detach())
            cv.append(c_new[act].detach())
        at = (torch.cat(ib), torch.cat(it)) if ib else (rows[:0], rows[:0])
        put = lambda n, vals: torch.zeros(B, T, n, dtype=dtype).index_put(at, torch.cat(vals) if vals else torch.zeros(0, n, dtype=dtype))
        ys.append(put(H, hv) * valid)
        gates.append(put(4 * H, gv) * valid)
        cells.append(put(H, cv) * valid)
        gxs.append(gx)
    return torch.cat(ys, 2), torch.stack(gates), torch.stack(cells), gxs


def gru(x, params, dtype, steps=None, mutation=None):
    """Returns hs (B, T + 1, 256), h_last (B, 256: hs[:, T], or hs[b, steps[b]]), gsave (B, T, 4, 256: r, z, n, hn), the
    input projections gi (B, T, 768) and the recurrent ones gh (T x (B, 768)), both in the graph."""
    assert mutation is None or mutation in GRU_MUTATIONS, mutation
    x = x.to(dtype)
    B, T, _ = x.shape
    w_ih, w_hh, b_ih, b_hh = (params[n].to(dtype) for n in GRU_NAMES)
    gi = x @ w_ih.t() + b_ih
    if gi.requires_grad:
        gi.retain_grad()
    h = torch.zeros(B, H, dtype=dtype)
    hs, ghs, saves = [h], [], []
    for t in range(T):
        h_in = h
        if mutation == 'neighbour_row' and t >= 1 and B >= 2:
            h_in = torch.cat((h[:B - 1], h[B - 2:B - 1]))
        if mutation == 'one_unit' and t == 1:
            keep = torch.ones(B, H, dtype=dtype)
            keep[B - 1, H - 1] = 0
            h_in = h * keep
        gh = h_in @ w_hh.t() + b_hh
        if gh.requires_grad:
            gh.retain_grad()
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = torch.tanh(gi[:, t, 2 * H:] + r * hn)
        h = (1 - z) * n + z * h_in
        hs.append(h)
        ghs.append(gh)
        saves.append(torch.stack((r, z, n, hn), 1).detach())
    hs = torch.stack(hs, 1)
    if steps is None or mutation == 'steps_T':
        h_last = hs[:, T]
    else:
        h_last = hs[torch.arange(B), torch.as_tensor(steps, dtype=torch.long)]
    return hs, h_last, torch.stack(saves, 1), gi, ghs


def lstm_quantities(x, wo, lens, params, dtype, mutation=None):
    """every compared quantity of the BiLSTM on these inputs, loss sum(y * wo)"""
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().to(dtype).requires_grad_(True)
    y, gates, cells, gxs = bilstm(xx, lens, P, dtype, mutation)
    (y * wo.to(dtype)).sum().backward()
    return {'y': y.detach(), 'gates': gates, 'cells': cells, 'dg': torch.stack([g.grad for g in gxs]), 'dx': xx.grad,
            'grad': {k: v.grad for k, v in P.items()}}


def gru_quantities(x, wo, steps, params, dtype, mutation=None):
    """every compared quantity of the GRU on these inputs: with steps (the ragged inference instance) the forward ones alone,
    otherwise loss sum(h_last * wo) and the gradients too"""
    P = {k: v.detach().to(dtype).requires_grad_(steps is None) for k, v in params.items()}
    xx = x.detach().to(dtype).requires_grad_(steps is None)
    hs, h_last, gsave, gi, ghs = gru(xx, P, dtype, steps, mutation)
    out = {'h_last': h_last.detach(), 'hs': hs.detach(), 'gsave': gsave[:, :, :3], 'hn': gsave[:, :, 3]}
    if steps is None:
        (h_last * wo.to(dtype)).sum().backward()
        out.update(dgi=gi.grad, dgh=torch.stack([g.grad for g in ghs], 1), dx=xx.grad, grad={k: v.grad for k, v in P.items()})
    return out


@functools.lru_cache(maxsize=None)
def oracle(c, dtype, mutation=None):
    """{quantity: tensor} of a case ('grad': {parameter: gradient}).  Cached; never modify the result."""
    if isinstance(c, LstmCase):
        x, wo, params = lstm_inputs(c)
        return lstm_quantities(x, wo, c.lens, params, dtype, mutation)
    x, wo, params = gru_inputs(c)
    return gru_quantities(x, wo, c.steps, params, dtype, mutation)


# ------------------------------------------------------------------------------------------------ comparison
def worst(a, ref):
    """largest |a - ref| and where"""
    d = (a.double() - ref.double()).abs()
    if d.numel() == 0:
        return 0.0, ()
    i = int(d.argmax())
    e = d.flatten()[i].item()
    where = []
    for n in reversed(d.shape):
        where.append(i % n)
        i //= n
    return e, tuple(reversed(where))


def rel(a, ref):
    """largest difference relative to the largest reference entry; a reference that is identically zero (the recurrent weight
    gradient at T = 1) is compared absolutely, as steer_ref.grad_rel does (d / 1e-3)"""
    d, where = worst(a, ref)
    s = ref.abs().max().item() if ref.numel() else 0.0
    return (d / s if s > 0 else d / 1e-3), where


def compare(res, ref):
    """{quantity: (error, where)} over the quantities both hold, measured as the module docstring says"""
    out = {}
    for q in ORDER:
        if q not in ref or q not in res:
            continue
        if q == 'grad':
            g = (-1.0, None)
            for name in sorted(ref[q]):
                e, where = rel(res[q][name], ref[q][name])
                if e > g[0]:
                    g = (e, (name, where))
            out[q] = g
        elif KIND[q] == 'rel':
            out[q] = rel(res[q], ref[q])
        else:
            out[q] = worst(res[q], ref[q])
    return out


@functools.lru_cache(maxsize=None)
def floor(c):
    """{quantity: fp32 reference minus fp64 reference}, measured as compare() measures"""
    return {k: v[0] for k, v in compare(oracle(c, torch.float32), oracle(c, torch.float64)).items()}


def bounds(floors, ref, K=16.0):
    """{quantity: K * max(floor, 4 * 2^-24 * scale)}: scale = max |reference| for the 'scaled' quantities, 1 for the others
    (bounded by 1, or relative already).  K: a number, or {quantity: number} (default 16)."""
    out = {}
    for q, f in floors.items():
        scale = ref[q].abs().max().item() if KIND[q] == 'scaled' and ref[q].numel() else 1.0
        out[q] = (K.get(q, 16.0) if isinstance(K, dict) else K) * max(f, ULP4 * scale)
    return out


def without(c, b):
    """the quantities (fp64) of an LSTM case's batch without item b, on the same rows of x and wo"""
    x, wo, params = lstm_inputs(c)
    rest = [i for i in range(c.B) if i != b]
    return lstm_quantities(x[rest], wo[rest], [c.lens[i] for i in rest], params, torch.float64)
