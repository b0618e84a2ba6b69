"""csrc/optim.hip (k_sumsq, k_clip_adam) through the C ABI, and optim.FlatAdam on a toy module, against the fp64 Adam of
tests/adam_ref.py on prescribed gradients.  No model in the loop: the error grows by a few ulp per step, so every element is
held to fp32 round-off,

    |got - ref64| <= K * 2^-24 * scale + ulp32(ref) / 2
    scale_p = |p| + |update|,  scale_m = |b1 m| + |(1-b1) gg|,  scale_v = b2 v + (1-b2) gg^2,  scale_norm = total.

K is twice the worst ratio that the same step reaches in torch fp32 on the CPU, in the kernel's operation order, on the very
inputs of these tests (tests/test_adam_ref.py measures it; profiles/adam_parity.txt holds the figures per case):

    single step (103 cases)      K_p = 30.88   K_m = 4.94   K_v = 11.22   K_norm = 1.00
    trajectory, at step t        K_p = 1.44 t  K_m = 4.54 t K_v = 10.40 t K_norm = 0.64

(p's single-step K is the largest because scale_p is |update| alone where a weight is tiny, and the update carries the errors
of m, v, a square root and two divisions.)  No element is masked out: the inputs avoid the one thing these scales cannot
express, a sum that cancels (adam_ref.kernel_inputs, adam_ref.toy_grads).
Every side (kernels, FlatAdam, references, torch) runs at adam_ref.B1 / B2, the fp32 neighbours of 0.9 / 0.999: the betas
cross the C ABI as floats, and against an Adam at the double 0.999 exp_avg_sq would sit 216 ulp off (documented, DESIGN a-20).
"""
import copy
import ctypes as C
import math
import os
import sys

import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu

TAIL = 64          # sentinel floats behind every arena


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


def _emul_wanted():
    return bool(os.environ.get('T2V_ADAM_PARITY'))


# ------------------------------------------------------------------ kernel level
class _Arenas(object):
    """p, g, m, v on the GPU, each with TAIL sentinel floats behind n; the partials and the norm word"""

    def __init__(self, p, g, m, v):
        self.n = p.numel()
        self.host = {}
        for i, (k, t) in enumerate(zip('pgmv', (p, g, m, v))):
            sentinel = -(1.0 + i) * 1e6 - 3.25 * torch.arange(TAIL, dtype=torch.float32)
            self.host[k] = torch.cat([t.reshape(-1).float(), sentinel])
        self.buf = {k: t.cuda() for k, t in self.host.items()}
        self.part = torch.full((1024,), -5.0, device='cuda')
        self.norm = torch.full((1,), -1.0, device='cuda')

    def call(self, h, lr=None, bc1=None, bc2=None, guard=None, guard_n=None, shift=None):
        """-> rc.  guard: None = t2v_clip_adam_step, else an int32 device tensor (or 'null') for the guarded entry;
        shift: the arena whose pointer is moved by 4 bytes"""
        import t2v_hip
        lib = t2v_hip.load_library()
        ptr = lambda k: C.c_void_p(self.buf[k].data_ptr() + (4 if shift == k else 0))
        args = [ptr('p'), ptr('g'), ptr('m'), ptr('v'), self.n, h['lr'] if lr is None else lr, h['b1'], h['b2'], h['eps'],
                h['wd'], h['max_norm'], h['inv_world'], 1.0 - h['b1'] ** h['step'] if bc1 is None else bc1,
                1.0 - h['b2'] ** h['step'] if bc2 is None else bc2, C.c_void_p(self.part.data_ptr()),
                C.c_void_p(self.norm.data_ptr())]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if guard is None:
            rc = lib.t2v_clip_adam_step(*(args + [stream]))
        else:
            gp = None if isinstance(guard, str) else C.c_void_p(guard.data_ptr())
            rc = lib.t2v_clip_adam_step_guarded(*(args + [gp, guard.numel() if guard_n is None else guard_n, stream]))
        torch.cuda.synchronize()
        return rc

    def result(self):
        return self.buf['p'][:self.n], self.buf['m'][:self.n], self.buf['v'][:self.n], float(self.norm)

    def untouched(self, arenas=''):
        """names of what changed among the four sentinel tails and the whole of `arenas`"""
        bad = [k + '_tail' for k in 'pgmv' if not _same_bits(self.buf[k][self.n:].cpu(), self.host[k][self.n:])]
        return bad + [k for k in arenas if not _same_bits(self.buf[k].cpu(), self.host[k])]

    def norm_bits(self):
        return int(_bits(self.norm).cpu()) & 0xffffffff


def _check_case(name, case):
    p, g, m, v, h = case
    ref, sc = A.clip_adam_ref_and_scales(p, g, m, v, **h)
    a = _Arenas(p, g, m, v)
    assert a.call(h) == 0
    r = A.step_ratios(a.result(), ref, sc, device='cuda')
    emul = A.step_ratios(A.clip_adam_emul32(p, g, m, v, **h), ref, sc) if _emul_wanted() else None
    A.parity_log(name, emul=emul, got=r)
    print(name, r)
    assert not A.beyond(r, A.K_STEP), r
    assert a.untouched('g') == []                  # the gradient arena is read only; nothing is written behind n
    b = _Arenas(p, g, m, v)                        # fresh copies: the same bits again
    assert b.call(h) == 0
    assert all(_same_bits(x, y) for x, y in zip(a.result()[:3], b.result()[:3])) and a.norm_bits() == b.norm_bits()
    return a, ref


@pytest.mark.parametrize('regime', list(A.REGIMES))          # (the upper parameter varies fastest: kernel_inputs caches by n)
@pytest.mark.parametrize('n', A.KERNEL_NS)
def test_step_matches_fp64_adam(n, regime):
    """t2v_clip_adam_step at the tail-only sizes, the exact sweep boundaries of both kernels, their second and third sweeps
    and an odd tail behind them; clip active / inactive / off, the 4-rank sum, wd 0 / 1e-2, step 1 from m = v = 0 and
    step 7 from random moments, all-zero gradients"""
    _check_case('step n=%d %s' % (n, regime), A.kernel_case(n, regime))


@pytest.mark.parametrize('where', list(A.OUTLIER_AT))
def test_norm_sees_an_outlier_wherever_it_sits(where):
    """one gradient of 1e3 among N(0, 1e-2) noise: the norm (~1000.2) and with it the coefficient (~1e-3, read back from
    exp_avg of the outlier, which is (1 - b1) * 1e3 * coef) follow the fp64 value; a region that k_sumsq dropped would leave a
    norm of ~20 and a coefficient 50 times too large"""
    case = A.outlier_case(where)
    a, ref = _check_case('outlier %s' % where, case)
    at, g = A.OUTLIER_AT[where], case[1]
    assert float(g[at]) == 1e3 and abs(ref[3] - 1000.2) < 0.1
    coef = float(a.result()[1][at].double()) / ((1.0 - A.B1) * 1e3)
    assert abs(coef - ref[4]) <= (A.K_STEP['m'] + 1.0) * A.EPS32 * ref[4]


GUARD_CASE = (A.SUMSQ_SWEEP + 4, 'active_late_wd')


def test_guard_skips_the_step_on_any_nonzero_word():
    import optim
    p, g, m, v, h = A.kernel_case(*GUARD_CASE)
    for w in range(5):
        guard = torch.zeros(5, dtype=torch.int32, device='cuda')
        guard[w] = 1 << (7 * w)
        a = _Arenas(p, g, m, v)
        assert a.call(h, guard=guard) == 0
        assert a.untouched('pgmv') == [], w
        assert a.norm_bits() == optim.FlatAdam.SKIPPED_NORM_BITS


def test_zero_guard_is_the_plain_step():
    p, g, m, v, h = A.kernel_case(*GUARD_CASE)
    a, b = _Arenas(p, g, m, v), _Arenas(p, g, m, v)
    assert a.call(h) == 0 and b.call(h, guard=torch.zeros(5, dtype=torch.int32, device='cuda')) == 0
    assert all(_same_bits(x, y) for x, y in zip(a.result()[:3], b.result()[:3])) and a.norm_bits() == b.norm_bits()
    assert not _same_bits(a.result()[0].cpu(), p) and b.untouched('g') == []


def test_device_record_overrides_the_by_value_scalars():
    """with a record installed, lr, bc1 and sqrt(bc2) of the step come from device memory (what a captured graph replays):
    the call passes another lr and the bias corrections of another step, and the result follows the record"""
    import t2v_hip
    p, g, m, v, h = A.kernel_case(A.SUMSQ_SWEEP + 4, 'active_late_wd')
    ref, sc = A.clip_adam_ref_and_scales(p, g, m, v, **h)
    sp = t2v_hip.step_params(create=True)
    sp.set(lr=h['lr'], bc1=1.0 - h['b1'] ** h['step'], bc2s=math.sqrt(1.0 - h['b2'] ** h['step']))
    sp.upload()
    a = _Arenas(p, g, m, v)
    assert a.call(h, lr=7.0 * h['lr'], bc1=1.0 - h['b1'] ** 2, bc2=1.0 - h['b2'] ** 2) == 0
    r = A.step_ratios(a.result(), ref, sc, device='cuda')
    A.parity_log('device record n=%d active_late_wd' % p.numel(), got=r)
    assert not A.beyond(r, A.K_STEP), r
    assert a.untouched('g') == []
    # (and the by-value scalars alone would have landed far outside the bound)
    by_value = A.clip_adam_ref(p, g, m, v, **dict(h, lr=7.0 * h['lr'], step=2))
    assert A.worst_ratio(a.result()[0], by_value[0], sc['p'], 'cuda') > 1e3 * A.K_STEP['p']


@pytest.mark.parametrize('what', ['p+4', 'g+4', 'm+4', 'v+4', 'bc1=0', 'null_guard'])
def test_bad_arguments_are_refused_and_write_nothing(what):
    p, g, m, v, h = A.kernel_case(7, 'active_late_wd')
    a = _Arenas(p, g, m, v)
    part, norm = a.part.clone(), a.norm.clone()
    if what == 'bc1=0':
        rc = a.call(h, bc1=0.0)
    elif what == 'null_guard':
        rc = a.call(h, guard='null', guard_n=2)
    else:
        rc = a.call(h, shift=what[0])
    assert rc != 0
    assert a.untouched('pgmv') == [] and _same_bits(a.part, part) and _same_bits(a.norm, norm)


# ------------------------------------------------------------------ FlatAdam on a toy module
class _Toy(torch.nn.Module):
    def __init__(self, params):
        super(_Toy, self).__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in params])


def _toy_adam(params=None, world=1):
    import optim
    model = _Toy(A.toy_params() if params is None else params).cuda()
    opt = optim.FlatAdam(model, lr=A.TOY_LR[0], betas=(A.B1, A.B2), eps=1e-8, weight_decay=A.TOY_WD, grad_clip_thresh=1.0,
                         world_size=world)
    return model, opt


def _arena(ts, dtype=torch.float64, device='cuda'):
    """a list of per-tensor values laid out like FlatAdam's arena: every slot padded with zeros to a multiple of 4"""
    flat = []
    for t in ts:
        flat += [t.detach().reshape(-1).to(device=device, dtype=dtype), torch.zeros((-t.numel()) & 3, dtype=dtype, device=device)]
    return torch.cat(flat)


def _pad_mask(opt):
    mask = torch.ones(opt.numel, dtype=torch.bool, device='cuda')
    for (_, _, p), o in zip(opt._live, opt._offsets):
        mask[o:o + p.numel()] = False
    return mask


def _padding_is_zero(opt, mask):
    return all(not bool(_bits(a[mask]).any()) for a in (opt.params, opt.grads, opt.exp_avg, opt.exp_avg_sq)) \
        and not bool(_bits(opt.poison_slot()).any())


def _ratios(state, r):
    """state: (p, m, v arenas or per-tensor lists, norm); r: one step of flat_adam_ref(with_scales=True)"""
    to = lambda x: x if torch.is_tensor(x) else _arena(x)
    sc = r[5]
    return A.step_ratios(tuple(to(x) for x in state[:3]) + (state[3],), (_arena(r[0]), _arena(r[1]), _arena(r[2]), r[3]),
                         dict(p=_arena(sc['p']), m=_arena(sc['m']), v=_arena(sc['v']), norm=sc['norm']), device='cuda')


def _set_grads(model, grads, scale=1.0):
    for p, g in zip(model.w, grads):
        p.grad = None if g is None else (scale * g).cuda()


def _torch_step(params, opt, grads, lr, dtype):
    """clip_grad_norm_ + Adam.step() of the reference loop on `params`; -> the norm"""
    opt.param_groups[0]['lr'] = lr
    for p, g in zip(params, grads):
        p.grad = g.to(device=p.device, dtype=dtype)
    total = torch.nn.utils.clip_grad_norm_(params, 1.0)
    opt.step()
    return float(total)


def _torch_state(params, opt, total):
    return ([p.detach() for p in params], [opt.state[p]['exp_avg'] for p in params],
            [opt.state[p]['exp_avg_sq'] for p in params], total)


@pytest.mark.parametrize('world', [1, 4])
def test_flat_adam_follows_fp64_adam_for_20_steps(world):
    """20 steps on prescribed gradients (written as the 4-rank SUM when world_size = 4; the references get the mean), lr
    changed through param_groups half-way, clipped and unclipped steps, one tensor with zero gradient, wd = 1e-2: weights,
    both moments and grad_norm within the bound of flat_adam_ref at every step, and of clip_grad_norm_ + torch.optim.Adam in
    float64, which walks the same trajectory; the padding of every slot and the poison slot stay exactly zero"""
    params, grads = A.toy_params(), A.toy_grads()
    model, opt = _toy_adam(params, world)
    assert opt.numel == sum((p.numel() + 3) & ~3 for p in params) > A.CLIP_SWEEP
    assert opt._offsets == [sum((q.numel() + 3) & ~3 for q in params[:i]) for i in range(len(params))]
    mask = _pad_mask(opt)
    assert int(mask.sum()) == sum((-p.numel()) & 3 for p in params) == 13
    tp = [torch.nn.Parameter(p.double()) for p in params]
    topt = torch.optim.Adam(tp, lr=A.TOY_LR[0], betas=(A.B1, A.B2), eps=1e-8, weight_decay=A.TOY_WD)
    ref = A.flat_adam_ref(params, grads, lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0, with_scales=True)
    worst, coefs = {}, set()
    for t, (gs, r) in enumerate(zip(grads, ref), 1):
        opt.param_groups[0]['lr'] = A.TOY_LR[t - 1]
        _set_grads(model, gs, float(world))
        norm = opt.step()
        assert norm is opt.grad_norm and opt.step_count == t
        got = (opt.params, opt.exp_avg, opt.exp_avg_sq, float(norm))
        ratios = _ratios(got, r)
        A.worst_per_step(worst, ratios, t)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
        t64 = _torch_state(tp, topt, _torch_step(tp, topt, gs, A.TOY_LR[t - 1], torch.float64))
        assert abs(t64[3] - r[3]) <= 1e-12 * r[3]
        for i in range(3):              # torch in float64 and flat_adam_ref are one trajectory ...
            assert all(float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) for a, b in zip(t64[i], r[i])), (t, i)
        ratios64 = A.step_ratios(got, tuple(_arena(x) for x in t64[:3]) + (t64[3],),
                                 dict(p=_arena(r[5]['p']), m=_arena(r[5]['m']), v=_arena(r[5]['v']), norm=r[3]), device='cuda')
        assert not A.beyond(ratios64, A.K_TRAJ, t), (t, ratios64)          # ... and the arena is within the bound of both
        assert _padding_is_zero(opt, mask), t
        assert not bool(_bits(opt.exp_avg_sq[opt._offsets[A.TOY_ZERO_GRAD]:][:8]).eq(0).any())   # wd moves the zero-gradient tensor
        coefs.add(r[4] < 1.0)
    assert coefs == {True, False}
    print('toy world=%d' % world, worst)
    A.parity_log('toy 20 steps world=%d (p, m, v: ratio / step)' % world, got=worst)
    for p, o in zip(model.w, opt._offsets):                 # the module's parameters ARE the arena
        assert p.data_ptr() == opt.params[o:].data_ptr()


def test_poison_slot_is_outside_the_norm_and_the_update():
    """the 4 floats behind the gradient arena travel with the all-reduce (a rank's "my step is void" flag) and must never
    reach the norm or a weight"""
    grads = A.toy_grads(1)[0]
    res = []
    for poison in (0.0, 1e6):
        model, opt = _toy_adam()
        _set_grads(model, grads)
        opt.poison_slot().fill_(poison)
        opt.step()
        torch.cuda.synchronize()
        res.append([t.clone() for t in (opt.params, opt.exp_avg, opt.exp_avg_sq, opt.grad_norm)])
        assert float(opt.poison_slot().min()) == poison
    assert all(_same_bits(a, b) for a, b in zip(*res))
    assert not _same_bits(res[0][0], _arena(A.toy_params(), torch.float32))


def test_parameter_without_gradient_keeps_its_slot():
    """`.grad = None` on two steps: that tensor's p, exp_avg and exp_avg_sq slices keep their bits, every other tensor
    follows flat_adam_ref, and afterwards the tensor goes on under the GLOBAL step count (torch.optim.Adam keeps one count
    per parameter and would lag by one: a documented deviation, see optim.FlatAdam.step)"""
    params, grads = A.toy_params(), A.toy_grads(no_grad=True)
    idx, steps = A.TOY_NO_GRAD
    model, opt = _toy_adam(params)
    o, k = opt._offsets[idx], params[idx].numel()
    ref = A.flat_adam_ref(params, grads, lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0, with_scales=True)
    worst, skipped = {}, 0
    for t, (gs, r) in enumerate(zip(grads, ref), 1):
        opt.param_groups[0]['lr'] = A.TOY_LR[t - 1]
        before = [a[o:o + k].clone() for a in (opt.params, opt.exp_avg, opt.exp_avg_sq)]
        _set_grads(model, gs)
        opt.step()
        after = [a[o:o + k] for a in (opt.params, opt.exp_avg, opt.exp_avg_sq)]
        if gs[idx] is None:
            assert t in steps and all(_same_bits(a, b) for a, b in zip(before, after)), t
            assert not bool(_bits(opt.grads[o:o + k]).any())
            skipped += 1
        else:
            assert not any(_same_bits(a, b) for a, b in zip(before, after)), t
        ratios = _ratios((opt.params, opt.exp_avg, opt.exp_avg_sq, float(opt.grad_norm)), r)
        A.worst_per_step(worst, ratios, t)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
    assert skipped == len(steps) == 2 and opt.step_count == A.TOY_STEPS
    print('toy no_grad', worst)
    A.parity_log('toy 20 steps world=1 no_grad (p, m, v: ratio / step)', got=worst)


def test_state_dict_continues_in_torch_adam():
    """after 7 steps FlatAdam.state_dict() goes into a stock fp32 torch.optim.Adam over a copy of the module; both go on
    for 7 more steps (across the lr change) on the same gradients, weights and moments of each within the bound of the fp64
    trajectory at steps 8..14"""
    params, grads = A.toy_params(), A.toy_grads(14)
    model, opt = _toy_adam(params)
    ref = A.flat_adam_ref(params, grads, lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0, with_scales=True)
    worst_f, worst_t = {}, {}
    for t, (gs, r) in enumerate(zip(grads, ref), 1):
        if t == 8:
            sd = opt.state_dict()
            assert all(float(st['step']) == 7.0 for st in sd['state'].values()) and len(sd['state']) == len(params)
            twin = _Toy([p.detach() for p in model.w]).cuda()
            tw = list(twin.w)
            topt = torch.optim.Adam(tw, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5)
            topt.load_state_dict(copy.deepcopy(sd))
            g0 = topt.param_groups[0]
            assert (g0['lr'], tuple(g0['betas']), g0['eps'], g0['weight_decay']) == (A.TOY_LR[6], (A.B1, A.B2), 1e-8, A.TOY_WD)
            assert all(_same_bits(topt.state[p]['exp_avg'].reshape(-1), opt.exp_avg[o:o + p.numel()])
                       for p, o in zip(tw, opt._offsets))
        opt.param_groups[0]['lr'] = A.TOY_LR[t - 1]
        _set_grads(model, gs)
        opt.step()
        ratios = _ratios((opt.params, opt.exp_avg, opt.exp_avg_sq, float(opt.grad_norm)), r)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
        if t >= 8:
            A.worst_per_step(worst_f, ratios, t)
            total = _torch_step(tw, topt, gs, A.TOY_LR[t - 1], torch.float32)
            ratios = _ratios(_torch_state(tw, topt, total), r)
            del ratios['norm']          # (clip_grad_norm_'s return value is no optimiser state: torch's own summation)
            A.worst_per_step(worst_t, ratios, t)
            assert not A.beyond(ratios, A.K_TRAJ, t), ('torch', t, ratios)
    print('interchange', worst_f, worst_t)
    A.parity_log('toy steps 8-14 FlatAdam beside torch fp32 Adam', got=worst_f)
    A.parity_log('toy steps 8-14 torch fp32 Adam from FlatAdam.state_dict()', got=worst_t)


def test_torch_adam_state_continues_in_flat_adam():
    """the reverse: 7 steps of a stock fp32 torch.optim.Adam, its state_dict() through FlatAdam.load_state_dict(): the step
    count follows, and 7 more steps stay within the bound of an fp64 trajectory restarted from that very fp32 state (what
    torch's own seven steps lost is not FlatAdam's to answer for); differing per-parameter counts are refused"""
    import optim
    params, grads = A.toy_params(), A.toy_grads(14)
    twin = _Toy(params).cuda()
    tw = list(twin.w)
    topt = torch.optim.Adam(tw, lr=A.TOY_LR[0], betas=(A.B1, A.B2), eps=1e-8, weight_decay=A.TOY_WD)
    for t in range(1, 8):
        _torch_step(tw, topt, grads[t - 1], A.TOY_LR[t - 1], torch.float32)
    sd = topt.state_dict()
    bad = copy.deepcopy(sd)
    bad['state'][3]['step'] = torch.tensor(6.0)
    with pytest.raises(ValueError):
        optim.FlatAdam(_Toy(params).cuda(), grad_clip_thresh=1.0).load_state_dict(bad)
    model = _Toy([p.detach() for p in tw]).cuda()
    opt = optim.FlatAdam(model, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5, grad_clip_thresh=1.0)
    opt.load_state_dict(sd)
    g0 = opt.param_groups[0]
    assert opt.step_count == 7
    assert (g0['lr'], tuple(g0['betas']), g0['eps'], g0['weight_decay']) == (A.TOY_LR[6], (A.B1, A.B2), 1e-8, A.TOY_WD)
    state = _torch_state(tw, topt, 0.0)
    assert all(_same_bits(q, _arena(x, torch.float32)) for q, x in zip((opt.params, opt.exp_avg, opt.exp_avg_sq), state))
    ref = A.flat_adam_ref(state[0], grads[7:], lr=list(A.TOY_LR[7:14]), wd=A.TOY_WD, max_norm=1.0, m=state[1], v=state[2],
                          step0=7, with_scales=True)
    worst = {}
    for t, (gs, r) in enumerate(zip(grads[7:], ref), 1):
        opt.param_groups[0]['lr'] = A.TOY_LR[7 + t - 1]
        _set_grads(model, gs)
        opt.step()
        assert opt.step_count == 7 + t
        ratios = _ratios((opt.params, opt.exp_avg, opt.exp_avg_sq, float(opt.grad_norm)), r)
        A.worst_per_step(worst, ratios, t)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
    print('reverse interchange', worst)
    A.parity_log('toy steps 8-14 FlatAdam from torch fp32 Adam.state_dict() (p, m, v: ratio / step)', got=worst)
