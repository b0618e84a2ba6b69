"""tests/adam_ref.py on the CPU: the fp64 reference of the fused clip + Adam step against torch in float64, and the fp32
emulation that sets the K of the bound against the reference on every case of tests/test_optim_gpu.py."""
import math

import pytest
import torch

import adam_ref as A

SHAPES = ((1,), (3,), (5,), (8, 8), (1023,), (70001,))


def _small(steps=12):
    gen = torch.Generator().manual_seed(5)
    params = [0.3 * torch.randn(*s, generator=gen) for s in SHAPES]
    numel = sum(p.numel() for p in params)
    grads = []
    for k in range(steps):
        norm = 3.0 if k % 3 else 0.3                  # clip_grad_norm_(…, 1.0) bites on two steps of three
        gs = [torch.randn(*s, generator=gen) * (norm / math.sqrt(numel)) for s in SHAPES]
        gs[2] = torch.zeros(*SHAPES[2])
        grads.append(gs)
    return params, grads


@pytest.mark.parametrize('wd', [0.0, 1e-6, 1e-2])
@pytest.mark.parametrize('max_norm', [1.0, 0.0], ids=['clip', 'noclip'])
def test_reference_is_torch_adam_in_float64(max_norm, wd):
    """a dozen steps of clip_grad_norm_ + torch.optim.Adam(weight_decay=wd) in float64, lr changed half-way: p, exp_avg,
    exp_avg_sq (per tensor, relative to its largest element), the norm and the coefficient agree with flat_adam_ref to 1e-12;
    clip_adam_ref on the concatenation walks the same trajectory bit for bit"""
    params, grads = _small()
    lrs = [1e-3] * 6 + [4e-4] * 6
    tp = [torch.nn.Parameter(p.double()) for p in params]
    opt = torch.optim.Adam(tp, lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref = A.flat_adam_ref(params, grads, lr=lrs, b1=0.9, b2=0.999, wd=wd, max_norm=max_norm, with_scales=True)
    cat = lambda ts: torch.cat([t.detach().double().reshape(-1) for t in ts])
    P, M, V = cat(params), torch.zeros(sum(p.numel() for p in params), dtype=torch.float64), None
    V = M.clone()
    seen = set()
    for k, (gs, (rp, rm, rv, total, coef, sc)) in enumerate(zip(grads, ref)):
        opt.param_groups[0]['lr'] = lrs[k]
        for p, g in zip(tp, gs):
            p.grad = g.double()
        if max_norm > 0:
            t_total = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
            assert abs(t_total - total) <= 1e-12 * total
            t_coef = float(tp[-1].grad[0] / gs[-1].double()[0])
            assert abs(t_coef - coef) <= 1e-12
            seen.add(coef < 1.0)
        else:
            assert coef == 1.0
        opt.step()
        for i, p in enumerate(tp):
            st = opt.state[p]
            for got, want in ((p.detach(), rp[i]), (st['exp_avg'], rm[i]), (st['exp_avg_sq'], rv[i])):
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (k, i)
        # the single-call reference on the concatenated arena walks the same trajectory
        P, M, V, total1, coef1 = A.clip_adam_ref(P, cat(gs), M, V, step=k + 1, lr=lrs[k], b1=0.9, b2=0.999, eps=1e-8, wd=wd,
                                                 max_norm=max_norm, inv_world=1.0)
        assert total1 == total and coef1 == coef
        assert torch.equal(P, cat(rp)) and torch.equal(M, cat(rm)) and torch.equal(V, cat(rv))
    if max_norm > 0:
        assert seen == {True, False}          # the trajectory has clipped and unclipped steps


def test_reference_averages_the_rank_sum():
    """inv_world: the norm and the coefficient are those of the MEAN gradient, like a single process fed the mean"""
    params, grads = _small(3)
    one = list(A.flat_adam_ref(params, grads, lr=1e-3, wd=1e-2))
    four = list(A.flat_adam_ref(params, [[4.0 * g for g in gs] for gs in grads], lr=1e-3, wd=1e-2, inv_world=0.25))
    for a, b in zip(one, four):
        assert a[3] == b[3] and a[4] == b[4]
        assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]))


def test_reference_skips_a_tensor_without_gradient_under_one_global_step_count():
    """FlatAdam's semantics, not torch's: the skipped tensor keeps p, m, v, adds nothing to the norm, and afterwards its
    bias corrections follow the GLOBAL step count (torch.optim.Adam would lag by one for that tensor)."""
    params, grads = _small(4)
    grads[1][4] = None
    traj = list(A.flat_adam_ref(params, grads, lr=1e-3, b1=0.9, b2=0.999, wd=1e-2))
    for q in range(3):
        assert torch.equal(traj[1][q][4], traj[0][q][4])
        assert not torch.equal(traj[2][q][4], traj[1][q][4])
    others = [g for i, g in enumerate(grads[1]) if i != 4]
    assert abs(traj[1][3] - math.sqrt(sum(float((g.double() ** 2).sum()) for g in others))) <= 1e-14 * traj[1][3]
    # step 3 of the skipped tensor uses bias corrections of t = 3 although it has taken two steps
    coef = traj[2][4]
    p, m, v = traj[1][0][4], traj[1][1][4], traj[1][2][4]
    gg = 1e-2 * p + grads[2][4].double() * coef
    m1, v1 = 0.9 * m + (1.0 - 0.9) * gg, 0.999 * v + (1.0 - 0.999) * gg * gg
    want = p - 1e-3 / (1 - 0.9 ** 3) * m1 / (v1.sqrt() / math.sqrt(1 - 0.999 ** 3) + 1e-8)
    assert bool(((traj[2][0][4] - want).abs() <= 1e-15 * p.abs()).all())
    lag = p - 1e-3 / (1 - 0.9 ** 2) * m1 / (v1.sqrt() / math.sqrt(1 - 0.999 ** 2) + 1e-8)
    assert float((traj[2][0][4] - lag).abs().max()) > 1e-5


def test_half_ulp32():
    x = torch.tensor([1.0, 1.5, 2.0 - 2.0 ** -24, 2.0, 3.7, 1e-3, 1000.2, 2.0 ** -126, 1e-40, 0.0], dtype=torch.float64)
    f = x.float()
    up = torch.nextafter(f, torch.full_like(f, float('inf'))).double() - f.double()
    up[2] = 2.0 ** -23                # 2 - 2^-24 is no fp32 number: it lies in [1, 2)
    assert torch.equal(A.half_ulp32(x), up / 2)
    assert torch.equal(A.half_ulp32(-x), up / 2)


def test_worst_ratio_counts_every_element():
    ref = torch.tensor([1.0, -2.0, 0.0, 4.0], dtype=torch.float64)
    scale = torch.tensor([1.0, 2.0, 0.0, 4.0], dtype=torch.float64)
    assert A.worst_ratio(ref.float(), ref, scale) == 0.0
    got = ref.clone()
    got[1] += 2.0 ** -23 + 3 * 2.0 ** -24 * 2.0            # half an ulp of 2.0 is free, the rest is 3 eps * scale
    assert A.worst_ratio(got, ref, scale) == 3.0
    got = ref.clone()
    got[2] = 1e-30                                         # scale 0: anything beyond half a (subnormal) ulp is infinite
    assert A.worst_ratio(got, ref, scale) == float('inf')
    got[2] = float('nan')
    assert A.worst_ratio(got, ref, scale) == float('inf')
    assert A.worst_ratio(ref[:3], ref, scale) == float('inf')


def test_norm_emulation_sums_every_element_once():
    """the kernel-shaped summation tree of norm_emul32 against a float64 sum, at sizes around its sweep boundaries"""
    for n in (1, 5, A.SUMSQ_SWEEP - 1, A.SUMSQ_SWEEP + 5, 2 * A.SUMSQ_SWEEP + 7):
        g = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
        want = float((g.double() * 0.25).norm())
        assert abs(float(A.norm_emul32(g, 0.25)) - want) <= 4 * A.EPS32 * want


def _emul_ratios(case):
    p, g, m, v, h = case
    return A.step_ratios(A.clip_adam_emul32(p, g, m, v, **h), A.clip_adam_ref(p, g, m, v, **h), A.clip_adam_scales(p, g, m, v, **h))


@pytest.mark.parametrize('regime', list(A.REGIMES))          # (the upper parameter varies fastest: kernel_inputs caches by n)
@pytest.mark.parametrize('n', A.KERNEL_NS)
def test_fp32_emulation_is_inside_the_single_step_bound(n, regime):
    """Where K_STEP comes from: the step in CPU fp32, in the kernel's operation order, against the fp64 reference on the
    very inputs of test_optim_gpu's kernel cases, every element counted.  It sits at half of K or below (K is twice the
    worst of these ratios); the assertion allows K itself, for a libm or generator that differs in the last bit."""
    r = _emul_ratios(A.kernel_case(n, regime))
    A.parity_log('step n=%d %s' % (n, regime), emul=r)
    assert not A.beyond(r, A.K_STEP), r


@pytest.mark.parametrize('where', list(A.OUTLIER_AT))
def test_fp32_emulation_is_inside_the_bound_with_an_outlier(where):
    case = A.outlier_case(where)
    r = _emul_ratios(case)
    A.parity_log('outlier %s' % where, emul=r)
    assert not A.beyond(r, A.K_STEP), r
    # and the bound tells a dropped outlier from round-off by orders of magnitude
    p, g, m, v, h = case
    g2 = g.clone()
    g2[A.OUTLIER_AT[where]] = 0.0
    total, dropped = A.clip_adam_ref(p, g, m, v, **h)[3], A.clip_adam_ref(p, g2, m, v, **h)[3]
    assert abs(dropped - total) > 1e5 * A.K_STEP['norm'] * A.EPS32 * total


@pytest.mark.parametrize('world,no_grad', [(1, False), (4, False), (1, True)], ids=['world1', 'world4', 'no_grad'])
def test_fp32_emulation_is_inside_the_trajectory_bound(world, no_grad):
    """Where K_TRAJ comes from: FlatAdam's arena stepped in CPU fp32 over the toy trajectories of test_optim_gpu (20 steps,
    lr change, clipped and unclipped steps, a tensor with zero gradient, wd = 1e-2; the 4-rank sum; a tensor without a
    gradient on two steps), against flat_adam_ref"""
    params, grads = A.toy_params(), A.toy_grads(no_grad=no_grad)
    kw = dict(lr=list(A.TOY_LR), wd=A.TOY_WD, max_norm=1.0)
    ref = A.flat_adam_ref(params, grads, with_scales=True, **kw)
    arena = [[None if g is None else float(world) * g for g in gs] for gs in grads]
    coefs, worst = set(), {}
    for t, (e, r) in enumerate(zip(A.flat_adam_emul32(params, arena, inv_world=1.0 / world, **kw), ref), 1):
        ratios = A.step_ratios(e, r, r[5])
        A.worst_per_step(worst, ratios, t)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
        coefs.add(r[4] < 1.0)
        assert all(bool((a * b > 0).all()) for a, b in zip(r[0], params))      # no weight changed sign (see toy_grads)
    A.parity_log('toy 20 steps world=%d%s (p, m, v: ratio / step)' % (world, ' no_grad' if no_grad else ''), emul=worst)
    assert coefs == {True, False}


def test_fp32_emulation_is_inside_the_trajectory_bound_after_a_restart():
    """the interchange case of test_optim_gpu: 7 more steps from an fp32 state (here: 7 emulated steps), against a
    reference restarted from that very state with step count 7"""
    params, grads = A.toy_params(), A.toy_grads(14)
    kw = dict(wd=A.TOY_WD, max_norm=1.0)
    for p, m, v, _, _ in A.flat_adam_emul32(params, grads[:7], lr=list(A.TOY_LR[:7]), **kw):
        pass
    kw.update(lr=list(A.TOY_LR[7:14]), m=m, v=v, step0=7)
    worst = {}
    for t, (e, r) in enumerate(zip(A.flat_adam_emul32(p, grads[7:], **kw), A.flat_adam_ref(p, grads[7:], with_scales=True, **kw)), 1):
        ratios = A.step_ratios(e, r, r[5])
        A.worst_per_step(worst, ratios, t)
        assert not A.beyond(ratios, A.K_TRAJ, t), (t, ratios)
    A.parity_log('toy steps 8-14 restarted from an fp32 state (p, m, v: ratio / step)', emul=worst)


def test_betas_are_the_fp32_neighbours_of_the_requested_ones():
    """Why the tests run at adam_ref.B1 / B2: the betas reach the kernel as floats.  With them 1.0f - beta is exact; against
    an Adam at the double 0.999, 1 - beta2 is 1.3e-5 off and exp_avg_sq far outside the round-off bound: a property of the
    fp32 interface that is documented (optimiser row), not an error of a step."""
    one = torch.tensor(1.0, dtype=torch.float32)
    for b, want in ((A.B1, 0.9), (A.B2, 0.999)):
        assert b != want and abs(b - want) <= A.EPS32 * want
        assert float(one - torch.tensor(b, dtype=torch.float32)) == 1.0 - b
    assert abs((1.0 - A.B2) / (1.0 - 0.999) - 1.0) > 200 * A.EPS32
    p, g, m, v, h = A.kernel_case(7, 'active_first')
    at_double = dict(h, b1=0.9, b2=0.999)
    r = A.step_ratios(A.clip_adam_emul32(p, g, m, v, **h), A.clip_adam_ref(p, g, m, v, **at_double),
                      A.clip_adam_scales(p, g, m, v, **at_double))
    assert r['v'] > 10 * A.K_STEP['v'] and not A.beyond({k: r[k] for k in ('p', 'norm')}, A.K_STEP)
