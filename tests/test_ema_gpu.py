"""The weight average inside the fused clip + Adam step: t2v_clip_adam_ema_step_guarded (csrc/optim.hip) through the C ABI
and optim.FlatAdam(ema_decay=) on adam_ref's toy module.

Parameters, both moments and the norm must be the very bits of t2v_clip_adam_step_guarded on the same inputs; the shadow is
held to the bound of tests/ema_ref.py,

    |s32 - s64| <= K_EMA * t * 2^-24 * scale,      scale = running maximum of |s| + 2 rate_t |p - s|,     K_EMA = 3.1

(K_EMA: twice the worst ratio of ema_ref's numpy fp32 emulation, re-measured by tests/test_ema_ref.py, never taken from the
kernel).  A single step is compared with the fp64 update from the kernel's own stored parameters; the trajectories with an
fp64 Adam + average, which adds adam_ref.K_TRAJ['p'] * t half-ulps of p: the shadow is a convex combination of the p's.
Measured on an MI355X: a single step needs at most 1.24 of the allowed 3.1, the 20-step trajectories 0.30 of their bound.
"""
import ctypes as C
import math
import sys

import pytest
import torch

import adam_ref as A
import ema_ref as R

pytestmark = pytest.mark.gpu

TAIL = 64          # sentinel floats behind every arena
SIZES = (1, 3, 4, 7, A.CLIP_SWEEP + 4, 2 * A.CLIP_SWEEP + 3075)       # tail only, first float4, sweep boundary, third sweep + odd tail
REGIMES = ('active_late_wd', 'active_first')
RATE = R.rate32(R.DECAY)


@pytest.fixture(autouse=True)
def _no_grad_slots_leak():
    """a FlatAdam replaces the process-wide gradient-slot registration: later tests must not see slots of freed arenas"""
    yield
    mod = sys.modules.get('t2v_hip')
    if mod is not None:
        mod.register_grad_slots({})


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------ kernel level
class _Arenas(object):
    """p, g, m, v and the shadow s on the GPU, each with TAIL sentinel floats behind n; the partials and the norm word"""

    def __init__(self, p, g, m, v, s):
        self.n = p.numel()
        self.host = {}
        for i, (k, t) in enumerate(zip('pgmvs', (p, g, m, v, s))):
            sentinel = -(1.0 + i) * 1e6 - 3.25 * torch.arange(TAIL, dtype=torch.float32)
            self.host[k] = torch.cat([t.reshape(-1).float(), sentinel])
        self.buf = {k: t.cuda() for k, t in self.host.items()}
        self.part = torch.full((1024,), -5.0, device='cuda')
        self.norm = torch.full((1,), -1.0, device='cuda')

    def _args(self, h):
        ptr = lambda k: C.c_void_p(self.buf[k].data_ptr())
        return [ptr('p'), ptr('g'), ptr('m'), ptr('v'), self.n, h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], h['max_norm'],
                h['inv_world'], 1.0 - h['b1'] ** h['step'], 1.0 - h['b2'] ** h['step'], C.c_void_p(self.part.data_ptr()),
                C.c_void_p(self.norm.data_ptr())]

    def plain(self, h):
        """t2v_clip_adam_step_guarded without guard words -> rc (the shadow is not an argument)"""
        import t2v_hip
        rc = t2v_hip.load_library().t2v_clip_adam_step_guarded(*(self._args(h) + [None, 0, self._stream()]))
        torch.cuda.synchronize()
        return rc

    def ema(self, h, warmup, t, rate=RATE, guard=None, shadow='ok'):
        """t2v_clip_adam_ema_step_guarded -> rc.  shadow: 'ok', 'null', or '+4' (the pointer moved by 4 bytes)"""
        import t2v_hip
        sp = {'ok': self.buf['s'].data_ptr(), '+4': self.buf['s'].data_ptr() + 4, 'null': None}[shadow]
        gp, gn = (None, 0) if guard is None else (C.c_void_p(guard.data_ptr()), guard.numel())
        rc = t2v_hip.load_library().t2v_clip_adam_ema_step_guarded(
            *(self._args(h) + [gp, gn, None if sp is None else C.c_void_p(sp), rate, int(warmup), int(t), self._stream()]))
        torch.cuda.synchronize()
        return rc

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def result(self):
        return tuple(self.buf[k][:self.n] for k in 'pmvs')

    def untouched(self, arenas=''):
        """names of what changed among the five sentinel tails and the whole of `arenas`"""
        bad = [k + '_tail' for k in 'pgmvs' if not _same_bits(self.buf[k][self.n:].cpu(), self.host[k][self.n:])]
        return bad + [k for k in arenas if not _same_bits(self.buf[k].cpu(), self.host[k])]

    def norm_bits(self):
        return int(_bits(self.norm).cpu()) & 0xffffffff


def _case(n, regime):
    p, g, m, v, h = A.kernel_case(n, regime)
    return p, g, m, v, R.shadow_for(p), h


@pytest.mark.parametrize('regime', REGIMES)             # (the upper parameter varies fastest: kernel_inputs caches by n)
@pytest.mark.parametrize('n', SIZES)
def test_step_keeps_adams_bits_and_moves_the_shadow_like_fp64(n, regime):
    """warm-up at t = 0, 5 and 10^6 (rates 0.9, 0.6, 1e-4) and no warm-up: p, m, v and the norm are the bits of the plain guarded
    step; the shadow is within the bound of the fp64 update taken from the kernel's own p_new; nothing is written behind n, the
    gradients are read only, and fresh copies give the same bits again"""
    p, g, m, v, s, h = _case(n, regime)
    base = _Arenas(p, g, m, v, s)
    assert base.plain(h) == 0 and base.untouched('gs') == []
    assert not _same_bits(base.result()[0].cpu(), p)
    s0 = s.cuda()
    for warmup, t in R.STEP_CASES:
        a = _Arenas(p, g, m, v, s)
        assert a.ema(h, warmup, t) == 0
        assert all(_same_bits(x, y) for x, y in zip(a.result()[:3], base.result()[:3])), (warmup, t)
        assert a.norm_bits() == base.norm_bits()
        ref, scale = R.ema_ref(s0, a.result()[0], RATE, warmup, t)
        ratio = R.worst_ratio(a.result()[3], ref, scale)
        print('n=%d %s warmup=%s t=%d: shadow ratio %.3f of K_EMA %.2f' % (n, regime, warmup, t, ratio, R.K_EMA))
        assert ratio <= R.K_EMA, (warmup, t, ratio)
        assert not _same_bits(a.result()[3], s0)
        assert a.untouched('g') == []
        b = _Arenas(p, g, m, v, s)
        assert b.ema(h, warmup, t) == 0
        assert all(_same_bits(x, y) for x, y in zip(a.result(), b.result())) and a.norm_bits() == b.norm_bits()


RECORD_CASE = (A.SUMSQ_SWEEP + 4, 'active_late_wd')


def test_device_record_overrides_the_by_value_ema_t():
    """with a record installed, t of the warm-up is the record's epoch (what a replayed graph sees): epoch 3 against a by-value
    ema_t of 10^6 moves the shadow at 9 / 13, and lr / bc1 / bc2s come from the record as they always did"""
    import t2v_hip
    p, g, m, v, s, h = _case(*RECORD_CASE)
    sp = t2v_hip.step_params(create=True)
    sp.set(epoch=3, lr=h['lr'], bc1=1.0 - h['b1'] ** h['step'], bc2s=math.sqrt(1.0 - h['b2'] ** h['step']))
    sp.upload()
    other = dict(h, lr=7.0 * h['lr'], step=2)               # what the calls pass by value: another lr, another step's corrections
    base, a = _Arenas(p, g, m, v, s), _Arenas(p, g, m, v, s)
    assert base.plain(other) == 0 and a.ema(other, True, 10 ** 6) == 0
    assert all(_same_bits(x, y) for x, y in zip(a.result()[:3], base.result()[:3]))
    adam, sc = A.clip_adam_ref_and_scales(p, g, m, v, **h)
    assert not A.beyond(A.step_ratios(a.result()[:3] + (float(a.norm),), adam, sc, device='cuda'), A.K_STEP)
    s0 = s.cuda()
    assert R.rate_t(RATE, True, 3) == 9.0 / 13.0
    ref, scale = R.ema_ref(s0, a.result()[0], RATE, True, 3)
    assert R.worst_ratio(a.result()[3], ref, scale) <= R.K_EMA
    by_value, _ = R.ema_ref(s0, a.result()[0], RATE, True, 10 ** 6)          # (the by-value t alone would have landed far outside)
    assert R.worst_ratio(a.result()[3], by_value, scale) > 1e3 * R.K_EMA
    assert a.untouched('g') == []


def test_guard_leaves_all_five_arenas_alone():
    import optim
    p, g, m, v, s, h = _case(*RECORD_CASE)
    for w in range(5):
        guard = torch.zeros(5, dtype=torch.int32, device='cuda')
        guard[w] = 1 << (7 * w)
        a = _Arenas(p, g, m, v, s)
        assert a.ema(h, True, 5, guard=guard) == 0
        assert a.untouched('pgmvs') == [], w
        assert a.norm_bits() == optim.FlatAdam.SKIPPED_NORM_BITS


def test_zero_guard_is_the_plain_ema_step():
    p, g, m, v, s, h = _case(*RECORD_CASE)
    a, b = _Arenas(p, g, m, v, s), _Arenas(p, g, m, v, s)
    assert a.ema(h, True, 5) == 0 and b.ema(h, True, 5, guard=torch.zeros(5, dtype=torch.int32, device='cuda')) == 0
    assert all(_same_bits(x, y) for x, y in zip(a.result(), b.result())) and a.norm_bits() == b.norm_bits()
    assert not _same_bits(b.result()[3].cpu(), s) and b.untouched('g') == []


@pytest.mark.parametrize('what', ['null_ema', 'ema+4', 'rate=0', 'rate=1.5'])
def test_bad_ema_arguments_are_refused_and_write_nothing(what):
    import t2v_abi
    p, g, m, v, s, h = _case(7, 'active_late_wd')
    a = _Arenas(p, g, m, v, s)
    part, norm = a.part.clone(), a.norm.clone()
    kw = {'null_ema': dict(shadow='null'), 'ema+4': dict(shadow='+4'), 'rate=0': dict(rate=0.0), 'rate=1.5': dict(rate=1.5)}[what]
    assert a.ema(h, True, 0, **kw) == t2v_abi.load().define('T2V_ERR_ARG')
    assert a.untouched('pgmvs') == [] and _same_bits(a.part, part) and _same_bits(a.norm, norm)
    assert a.ema(h, True, 0, rate=1.0) == 0                 # (the closed end of (0, 1] is a rate)


# ------------------------------------------------------------------ FlatAdam on the toy module
class _Toy(torch.nn.Module):
    def __init__(self, params):
        super(_Toy, self).__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in params])
        self.register_buffer('stat', torch.arange(5, dtype=torch.float32))     # a buffer: ema_state_dict takes it from the model


def _toy_adam(params=None, **kw):
    import optim
    model = _Toy(A.toy_params() if params is None else params).cuda()
    opt = optim.FlatAdam(model, lr=A.TOY_LR[0], betas=(A.B1, A.B2), eps=1e-8, weight_decay=A.TOY_WD, grad_clip_thresh=1.0, **kw)
    return model, opt


def _arena(ts, dtype=torch.float64, device='cuda'):
    """a list of per-tensor values laid out like FlatAdam's arena: every slot padded with zeros to a multiple of 4"""
    flat = []
    for t in ts:
        flat += [t.detach().reshape(-1).to(device=device, dtype=dtype), torch.zeros((-t.numel()) & 3, dtype=dtype, device=device)]
    return torch.cat(flat)


def _set_grads(model, grads):
    for p, g in zip(model.w, grads):
        p.grad = None if g is None else g.cuda()


_ADAM64 = {}


def _adam64(no_grad):
    """the fp64 Adam trajectory of the toy module as arenas on the GPU, one per step; computed once per variant"""
    if no_grad not in _ADAM64:
        ref = A.flat_adam_ref(A.toy_params(), A.toy_grads(no_grad=no_grad), lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0)
        _ADAM64[no_grad] = [_arena(r[0]) for r in ref]
    return _ADAM64[no_grad]


@pytest.mark.parametrize('decay,warmup', [(0.99, True), (0.9999, False)], ids=['0.99_warmup', '0.9999_plain'])
@pytest.mark.parametrize('no_grad', [False, True], ids=['all_grads', 'no_grad_steps'])
def test_flat_adam_shadow_follows_fp64_adam_and_average_for_20_steps(no_grad, decay, warmup):
    """20 steps on prescribed gradients (lr changed half-way, clipped and unclipped steps, in the no_grad variant one tensor
    without a gradient on two steps, whose slot is put back): the shadow stays within the bound of the fp64 Adam + average at
    every step, and a FlatAdam without the average walks the very same bits in p, m and v"""
    params, grads = A.toy_params(), A.toy_grads(no_grad=no_grad)
    model, opt = _toy_adam(params, ema_decay=decay, ema_warmup=warmup)
    plain_model, plain = _toy_adam(params)
    assert plain.ema is None and opt.ema is not None and opt.ema.data_ptr() != opt.params.data_ptr()
    assert _same_bits(opt.ema, opt.params) and opt.ema.numel() == opt.numel
    rate = R.rate32(decay)
    s64 = _arena(params)
    scale = torch.zeros_like(s64)
    idx, none_steps = A.TOY_NO_GRAD
    o, k = opt._offsets[idx], params[idx].numel()
    worst = 0.0
    for t, (gs, p64) in enumerate(zip(grads, _adam64(no_grad)), 1):
        opt.param_groups[0]['lr'] = plain.param_groups[0]['lr'] = A.TOY_LR[t - 1]
        before = (opt.params[o:o + k].clone(), opt.ema[o:o + k].clone())
        _set_grads(model, gs)
        _set_grads(plain_model, gs)
        opt.step()
        plain.step()
        assert all(_same_bits(a, b) for a, b in zip((opt.params, opt.exp_avg, opt.exp_avg_sq, opt.grad_norm),
                                                    (plain.params, plain.exp_avg, plain.exp_avg_sq, plain.grad_norm))), t
        s64, sc = R.ema_ref(s64, p64, rate, warmup, t - 1)
        scale = torch.maximum(scale, sc)
        tol = R.bound(scale, t) + A.K_TRAJ['p'] * t * A.half_ulp32(p64)
        err = (opt.ema.double() - s64).abs()
        assert bool(torch.isfinite(opt.ema).all()) and bool((err <= tol).all()), (t, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
        if gs[idx] is None:
            # the slot that was put back: its weights keep their bits and its shadow moved towards THEM
            assert t in none_steps and _same_bits(opt.params[o:o + k], before[0])
            want, sc0 = R.ema_ref(before[1], before[0], rate, warmup, t - 1)
            assert R.worst_ratio(opt.ema[o:o + k], want, sc0) <= R.K_EMA
    assert not _same_bits(opt.ema, opt.params)
    print('toy no_grad=%s decay=%s warmup=%s: worst error / bound %.3f' % (no_grad, decay, warmup, worst))


def test_ema_state_round_trip_and_swap():
    """ema_state_dict() + state_dict() into a fresh FlatAdam continue with the same bits; swapped_ema() puts the average into
    the model in place and takes it out again bit-exactly"""
    params, grads = A.toy_params(), A.toy_grads(8)
    model, opt = _toy_adam(params, ema_decay=0.99)
    for t in range(5):
        _set_grads(model, grads[t])
        opt.step()
    esd, osd, msd = opt.ema_state_dict(model), opt.state_dict(), {k: v.clone() for k, v in model.state_dict().items()}
    assert list(esd) == list(model.state_dict()) and len(esd) == len(params) + 1
    for (name, p), off in zip(model.named_parameters(), opt._offsets):
        assert _same_bits(esd[name].reshape(-1), opt.ema[off:off + p.numel()]) and esd[name].shape == p.shape
        assert esd[name].data_ptr() != opt.ema[off:].data_ptr()                       # a clone
    assert torch.equal(esd['stat'], model.stat) and esd['stat'].data_ptr() != model.stat.data_ptr()
    # -- swap
    ptrs = [p.data_ptr() for p in model.w]
    p0, s0 = opt.params.clone(), opt.ema.clone()
    with opt.swapped_ema() as inside:
        assert inside is opt and [p.data_ptr() for p in model.w] == ptrs
        got = model.state_dict()
        assert list(got) == list(esd) and all(_same_bits(got[k_], esd[k_]) for k_ in esd)
        assert _same_bits(opt.ema, p0)
    assert _same_bits(opt.params, p0) and _same_bits(opt.ema, s0)
    with pytest.raises(RuntimeError, match='boom'):         # ... and on the way out of an exception as well
        with opt.swapped_ema():
            raise RuntimeError('boom')
    assert _same_bits(opt.params, p0) and _same_bits(opt.ema, s0)
    # -- continue in a fresh optimiser
    twin_model = _Toy([msd['w.%d' % i] for i in range(len(params))]).cuda()
    import optim
    twin = optim.FlatAdam(twin_model, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5, grad_clip_thresh=1.0, ema_decay=0.99)
    twin.ema.fill_(7.0)
    twin.load_state_dict(osd)
    assert twin.step_count == 5 and _same_bits(twin.ema, twin.params)       # no average in Adam's format: the shadow starts over
    twin.load_ema_state_dict(esd)
    assert _same_bits(twin.ema, opt.ema) and _same_bits(twin.params, opt.params)
    for t in range(5, 8):
        for mdl, op in ((model, opt), (twin_model, twin)):
            _set_grads(mdl, grads[t])
            op.step()
        assert _same_bits(twin.ema, opt.ema) and _same_bits(twin.params, opt.params), t
    # -- without an average there is nothing to ask for
    _, bare = _toy_adam(params)
    for call in (lambda: bare.ema_state_dict(model), lambda: bare.load_ema_state_dict(esd), lambda: bare.swapped_ema().__enter__()):
        with pytest.raises(ValueError, match='ema_decay'):
            call()
    with pytest.raises(ValueError):
        _toy_adam(params, ema_decay=1.0)
