"""Steered alignments for the decoder's attention — TEST INFRASTRUCTURE, NOT PRODUCT.

With its initial weights and randn memory the decoder's alignment is flat (alpha ~ 1 / T_in) and the 31-tap location filter adds
a few 1e-3 to a tanh argument of O(0.6): a halo tap lost where a kernel cuts T_in (16-position tiles, 128-position strides,
32- / 96-position reverse slices, the second softmax position from 512) moves nothing a test could see.  The recipe below puts
probability mass on both sides of every cut and gives the location term weight, on the same fp32 decoder:

  targets(n)   {0, n - 1} and {b - 1, b} for every cut b < n
  memory       + 0.4 u at an item's targets, u = pinv(W_mem) sign(v) in fp64: the processed memory moves by 0.4 sign(v), the
               direction in which the energy v . tanh(...) grows fastest
  location     location_dense.weight * 60

oracle() runs oracle/t2v_oracle.py on the harness of tests/test_decoder_gpu.py::_setup, steered, in fp32 or fp64, and can lose
one halo tap at a cut on purpose — in the forward values, or in the input gradient alone — by substituting the convolution the
oracle calls for the duration of the call (t2v_oracle.py itself is untouched).  floor() is the fp32 oracle minus the fp64 one: the
round-off of the arithmetic itself, the scale every bound of tests/test_decoder_steered_gpu.py is a multiple of.
"""
import functools

import torch
import torch.nn.functional as F

CUTS = (16, 32, 96, 128, 192, 288, 384, 480, 512)
GAIN, LOCATION_SCALE = 0.4, 60.0
HALO = 15                                           # location_conv: 31 taps, padding 15

# (B, T_in, T_out, lengths)
CASES = ((2, 20, 5, (20, 7)), (6, 84, 6, (84, 80, 71, 66, 50, 37)), (3, 97, 5, (97, 96, 17)), (16, 40, 3, tuple(range(40, 24, -1))),
         (2, 224, 4, (224, 129)), (2, 225, 4, (225, 130)), (2, 555, 3, (555, 290)), (2, 570, 3, (570, 300)))
# free-running decode: (T_in, B), every item at full length
DECODE_CASES = ((97, 3), (224, 1), (225, 1))
DECODE_FRAMES = 6

# one cut per family of cuts, (cut, case), for the mutation checks on the device: 16-position tiles, 32-position reverse slices,
# 96-position reverse slices (short and long form), 128-position strides, a 96-multiple of the long form, the second softmax
# position of a thread
MUTATION_CUTS = ((16, CASES[0]), (32, CASES[1]), (96, CASES[2]), (96, CASES[5]), (128, CASES[4]), (288, CASES[6]), (512, CASES[6]))

QUANTITIES = ('mel', 'gate', 'align', 'grad', 'd_memory')


def targets(n):
    """positions of an item of length n that are made to hold mass: both ends and both sides of every cut inside it"""
    t = {0, n - 1}
    for b in CUTS:
        if b < n:
            t.update((b - 1, b))
    return sorted(t)


def boundary_case(b):
    """the case with the shortest T_in whose longest item contains the cut b"""
    return min((c for c in CASES if b < c[1]), key=lambda c: c[1])


def steer(dec, memory, lengths):
    """Returns the steered memory (fp32, a new tensor) and scales location_dense of the CPU module `dec` in place."""
    al = dec.attention_layer
    with torch.no_grad():
        w_mem = al.memory_layer.linear_layer.weight.detach().double()                   # (128, 512)
        v = al.v.linear_layer.weight.detach().double()[0]                               # (128,)
        u = torch.linalg.pinv(w_mem) @ torch.sign(v)                                    # (512,): W_mem u = sign(v)
        mem = memory.detach().double().clone()
        for i, n in enumerate(int(x) for x in lengths):
            mem[i, targets(n)] += GAIN * u
        al.location_layer.location_dense.linear_layer.weight.mul_(LOCATION_SCALE)
    return mem.to(memory.dtype)


# ------------------------------------------------------------------------------------------------ the mutated convolution
def _lost_tap(x, w, b):
    """what input position b - 1 contributes to the outputs b .. b + 14 of conv1d(x, w, padding = 15), zero elsewhere"""
    T = x.shape[2]
    only = torch.zeros(T, dtype=x.dtype)
    only[b - 1] = 1
    out = torch.zeros(T, dtype=x.dtype)
    out[b:b + HALO] = 1
    return F.conv1d(x * only, w, None, padding=HALO) * out


class _ConvLosingTapInBackward(torch.autograd.Function):
    """conv1d(x, w, padding = 15) with its forward values untouched; the gradient with respect to x lacks what the outputs
    b .. b + 14 send to position b - 1.  The weight gradient is the true one."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.b = b
        return F.conv1d(x, w, None, padding=HALO)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            x_ = x.detach().requires_grad_(True)
            w_ = w.detach().requires_grad_(True)
            gx, gw = torch.autograd.grad(F.conv1d(x_, w_, None, padding=HALO), (x_, w_), g)
            lost, = torch.autograd.grad(_lost_tap(x_, w.detach(), ctx.b), x_, g)
        return gx - lost, gw, None


class _Functional(object):
    """torch.nn.functional with another conv1d for the location filter (the only conv1d of the decoder: padding 15, no bias)"""

    def __init__(self, mutation):
        self.kind, self.b = mutation

    def __getattr__(self, name):
        return getattr(F, name)

    def conv1d(self, x, w, bias=None, padding=0):
        assert bias is None and padding == HALO and w.shape[2] == 2 * HALO + 1 and self.b < x.shape[2]
        if self.kind == 'fwd':
            return F.conv1d(x, w, None, padding=HALO) - _lost_tap(x, w, self.b)
        assert self.kind == 'bwd', self.kind
        return _ConvLosingTapInBackward.apply(x, w, self.b)


class _substituted(object):
    def __init__(self, mutation):
        self.mutation = mutation

    def __enter__(self):
        import t2v_oracle as O
        self.O, self.old = O, O.F
        if self.mutation is not None:
            O.F = _Functional(self.mutation)

    def __exit__(self, *exc):
        self.O.F = self.old


# ------------------------------------------------------------------------------------------------ inputs and oracles
def inputs(case):
    """the harness of test_decoder_core_matches_oracle (seed 0), steered: (dec on the CPU, memory, mels, lengths, wm, wg).
    (_setup switches the Prenet dropout off for good: put back here.)"""
    import model as M
    import test_decoder_gpu as TD
    B, T_in, T, lens = case
    old = M.drop_rate
    try:
        hp, M, dec, memory, mels, lengths, wm, wg = TD._setup(B, T_in, T, list(lens))
    finally:
        M.drop_rate = old
    return dec, steer(dec, memory, lens), mels, lengths, wm, wg


def decode_inputs(T_in, B):
    """free-running decode: (dec on the CPU, steered memory), every item of length T_in"""
    dec, memory = inputs((B, T_in, 1, (T_in,) * B))[:2]
    return dec, memory


@functools.lru_cache(maxsize=3)
def oracle(case, dtype, mutation=None):
    """(mel, gate, align, {parameter: gradient}, d memory) of the steered case, teacher-forced, no dropout, loss
    sum(mel * wm) + sum(gate * wg).  mutation: None | ('fwd', b) | ('bwd', b).  Cached; never modify the result."""
    import t2v_oracle as O
    dec, memory, mels, lengths, wm, wg = inputs(case)
    sd = {'decoder.' + k: v.detach().to(dtype).requires_grad_(True) for k, v in dec.state_dict().items()}
    mem = memory.to(dtype).requires_grad_(True)
    with _substituted(mutation):
        mel, gate, align = O.decoder_forward(sd, mem, mels.to(dtype), lengths, p_att=0.0, p_dec=0.0)
        ((mel * wm.to(dtype)).sum() + (gate * wg.to(dtype)).sum()).backward()
    grads = {k[len('decoder.'):]: v.grad for k, v in sd.items()}
    return mel.detach(), gate.detach(), align.detach(), grads, mem.grad


@functools.lru_cache(maxsize=None)
def decode_oracle(T_in, B, dtype):
    """(mel (B, 80, 6), gate (B, 6), align (B, 6, T_in)) of 6 free-running frames, the gate ignored"""
    import t2v_oracle as O
    dec, memory = decode_inputs(T_in, B)
    sd = {'decoder.' + k: v.detach().to(dtype) for k, v in dec.state_dict().items()}
    with torch.no_grad():
        mel, gate, align = O.decoder_inference(sd, memory.to(dtype), max_steps=DECODE_FRAMES, stop_on_gate=False)
    return mel, gate.squeeze(-1), align


# ------------------------------------------------------------------------------------------------ comparison
def worst(a, ref):
    """largest |a - ref| and where"""
    d = (a.double() - ref.double()).abs()
    i = int(d.argmax())
    where = []
    for n in reversed(d.shape):
        where.append(i % n)
        i //= n
    return d.flatten()[int(d.argmax())].item(), tuple(reversed(where))


def grad_rel(a, ref):
    """largest difference relative to the largest reference entry; a reference gradient that is identically zero is compared
    absolutely, with the rule of test_decoder_core_matches_oracle (d / 1e-3)"""
    d, where = worst(a, ref)
    s = ref.abs().max().item()
    return (d / s if s > 0 else d / 1e-3), where


def compare(res, ref):
    """{quantity: (error, where)} of a result (mel, gate, align[, grads, d memory]) against a reference of the same form:
    mel / gate / align absolute; 'grad' the worst parameter gradient, each relative to its tensor's largest reference entry
    (where = (name, index)); 'd_memory' the worst item, each relative to that item's largest reference entry"""
    out = {name: worst(res[i], ref[i]) for i, name in enumerate(('mel', 'gate', 'align'))}
    if len(ref) > 3:
        g = (-1.0, None)
        for name in sorted(ref[3]):
            rel, where = grad_rel(res[3][name], ref[3][name])
            if rel > g[0]:
                g = (rel, (name, where))
        out['grad'] = g
        m = (-1.0, None)
        for i in range(ref[4].shape[0]):
            rel, where = grad_rel(res[4][i], ref[4][i])
            if rel > m[0]:
                m = (rel, (i,) + where)
        out['d_memory'] = m
    return out


def scales(ref):
    """max |reference| of the forward quantities: the scale their round-off goes with"""
    return {name: ref[i].abs().max().item() for i, name in enumerate(('mel', 'gate', 'align'))}


@functools.lru_cache(maxsize=None)
def floor(case):
    """{quantity: fp32 oracle minus fp64 oracle}, measured as compare() measures"""
    return {k: v[0] for k, v in compare(oracle(case, torch.float32), oracle(case, torch.float64)).items()}


@functools.lru_cache(maxsize=None)
def decode_floor(T_in, B):
    return {k: v[0] for k, v in compare(decode_oracle(T_in, B, torch.float32), decode_oracle(T_in, B, torch.float64)).items()}


ULP4 = 4.0 * 2.0 ** -24


def bounds(floors, ref, K=16.0):
    """{quantity: K * max(floor, 4 * 2^-24 * scale)}: scale = max |reference| for the forward quantities, 1 for the relative
    ones.  K: a number, or {quantity: number} (default 16)."""
    sc = scales(ref)
    return {q: (K.get(q, 16.0) if isinstance(K, dict) else K) * max(f, ULP4 * sc.get(q, 1.0)) for q, f in floors.items()}
