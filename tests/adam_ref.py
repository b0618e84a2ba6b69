"""fp64 reference of the fused clip + Adam step (csrc/optim.hip, optim.FlatAdam), its fp32 emulation and the error bound
that tests/test_optim_gpu.py holds the kernels to.  Plain torch on the CPU.

The step, as optim.hip documents it:
    gs    = g * inv_world                          (the all-reduce left the SUM over ranks in g)
    total = ||gs||_2
    coef  = min(1, max_norm / (total + 1e-6))      (1 when max_norm <= 0)
    gg    = wd * p + gs * coef                     (L2-in-gradient weight decay, torch.optim.Adam's)
    m     = b1 * m + (1 - b1) * gg
    v     = b2 * v + (1 - b2) * gg^2
    p     = p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
"""
import math

import torch

EPS32 = 2.0 ** -24                  # unit round-off of fp32
SUMSQ_BLOCKS, CLIP_BLOCKS = 1024, 2048       # grids of k_sumsq / k_clip_adam (256 threads, one float4 per thread and sweep)
SUMSQ_SWEEP = SUMSQ_BLOCKS * 256 * 4         # elements per grid sweep
CLIP_SWEEP = CLIP_BLOCKS * 256 * 4
# The betas cross the C ABI as floats, so the optimiser runs at the fp32 neighbours of the betas it is asked for:
# 0.89999998 and 0.99900001.  That is round-off of the hyper-parameter (1.3e-8 of beta2), but 1 - beta2 then is
# 0.00099998713, 1.3e-5 (216 fp32 ulp) off 1e-3, so against an Adam at the double 0.999 every exp_avg_sq increment is
# 1.3e-5 small.  The tests give these fp32 values, as doubles, to the kernels, to FlatAdam, to the references and to torch:
# every side then works with the very same betas, and 1.0f - beta in the kernel is exact.
B1 = float(torch.tensor(0.9, dtype=torch.float32))
B2 = float(torch.tensor(0.999, dtype=torch.float32))


def _f64(t):
    return t.detach().to(device='cpu', dtype=torch.float64).clone()


def _step64(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, inv_world):
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    gs = g * inv_world
    total = math.sqrt(float((gs * gs).sum()))
    coef = min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0
    gg = wd * p + gs * coef
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    denom = v1.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    upd = (lr / (1.0 - b1 ** step)) * (m1 / denom)
    scales = dict(p=p.abs() + upd.abs(), m=(b1 * m).abs() + ((1.0 - b1) * gg).abs(),
                  v=b2 * v + (1.0 - b2) * gg * gg, norm=total)
    return (p - upd, m1, v1, total, coef), scales


def clip_adam_ref(p, g, m, v, *, step, lr, b1, b2, eps, wd, max_norm, inv_world):
    """one step on float64 copies of the inputs -> (p, m, v, total_norm, coef); the inputs are left alone"""
    return _step64(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, inv_world)[0]


def clip_adam_ref_and_scales(p, g, m, v, *, step, lr, b1, b2, eps, wd, max_norm, inv_world):
    """(clip_adam_ref(...), clip_adam_scales(...)) from one evaluation"""
    return _step64(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, inv_world)


def clip_adam_scales(p, g, m, v, *, step, lr, b1, b2, eps, wd, max_norm, inv_world):
    """the magnitudes the error bound is relative to: dict(p=|p| + |update|, m=|b1 m| + |(1-b1) gg|,
    v=b2 v + (1-b2) gg^2, norm=total), from the values BEFORE the step"""
    return _step64(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, inv_world)[1]


def flat_adam_ref(params, grads_per_step, *, lr, b1=B1, b2=B2, eps=1e-8, wd=0.0, max_norm=1.0, inv_world=1.0,
                  m=None, v=None, step0=0, with_scales=False):
    """A multi-tensor trajectory with FlatAdam's semantics.  params: list of tensors; grads_per_step: one list per step
    with a tensor or None per parameter; lr: a float or one float per step.  ONE global step count (step0 + 1, ...); a
    tensor without a gradient adds zeros to the norm and keeps its p, m and v.  Yields, per step,
    (params, m, v, total_norm, coef) as float64 lists (fresh copies), plus the per-tensor scales when asked."""
    ps = [_f64(t) for t in params]
    ms = [torch.zeros_like(t) for t in ps] if m is None else [_f64(t) for t in m]
    vs = [torch.zeros_like(t) for t in ps] if v is None else [_f64(t) for t in v]
    sizes = [t.numel() for t in ps]
    for k, grads in enumerate(grads_per_step):
        lr_k = lr[k] if isinstance(lr, (list, tuple)) else lr
        gs = [torch.zeros_like(t) if g is None else _f64(g) for t, g in zip(ps, grads)]
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        (p1, m1, v1, total, coef), sc = _step64(cat(ps), cat(gs), cat(ms), cat(vs), step0 + k + 1, lr_k, b1, b2, eps, wd,
                                                max_norm, inv_world)
        split = lambda flat: [c.view_as(t) for c, t in zip(flat.split(sizes), ps)]
        keep = [g is None for g in grads]
        ps = [old if kp else new.clone() for kp, old, new in zip(keep, ps, split(p1))]
        ms = [old if kp else new.clone() for kp, old, new in zip(keep, ms, split(m1))]
        vs = [old if kp else new.clone() for kp, old, new in zip(keep, vs, split(v1))]
        out = ([t.clone() for t in ps], [t.clone() for t in ms], [t.clone() for t in vs], total, coef)
        if with_scales:
            out = out + (dict(p=split(sc['p']), m=split(sc['m']), v=split(sc['v']), norm=total),)
        yield out


# ---- the same step in fp32, in the kernels' operation order (without fma contraction)
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _wave_sum32(a):
    """a: (..., 64) -> (...): butterfly sum of one wavefront (xor 1, 2, 4, ... 32)"""
    for _ in range(6):
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def norm_emul32(g, inv_world):
    """||g * inv_world||_2 in fp32 with the summation tree of k_sumsq + the head of k_clip_adam: per-thread running sums over
    the grid sweeps, wavefront butterflies, (r0 + r1) + (r2 + r3) per block, 1024 partials re-reduced by 256 threads"""
    g = g.detach().to(device='cpu', dtype=torch.float32).reshape(-1)
    n = g.numel()
    n4 = n >> 2
    threads = SUMSQ_BLOCKS * 256
    sweeps = max(1, -(-n4 // threads))
    x = torch.zeros(sweeps * threads * 4, dtype=torch.float32)
    x[:n4 * 4] = g[:n4 * 4] * _f32(inv_world)
    x = x.view(sweeps, threads, 4)
    acc = torch.zeros(threads, dtype=torch.float32)
    for s in range(sweeps):
        for c in range(4):
            acc = acc + x[s, :, c] * x[s, :, c]
    if n & 3:
        t = g[n4 * 4:] * _f32(inv_world)
        acc[:n & 3] = acc[:n & 3] + t * t
    red = _wave_sum32(acc.view(SUMSQ_BLOCKS, 4, 64))
    partials = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])
    acc = ((partials[0:256] + partials[256:512]) + partials[512:768]) + partials[768:1024]
    red = _wave_sum32(acc.view(4, 64))
    return ((red[0] + red[1]) + (red[2] + red[3])).sqrt()


def clip_adam_emul32(p, g, m, v, *, step, lr, b1, b2, eps, wd, max_norm, inv_world, bc1=None, bc2=None):
    """-> (p, m, v, total_norm, coef) in fp32: every operation of optim.hip rounded to fp32 in the kernel's order.  The
    scalars arrive like at the C ABI, as floats; 1 - b1 and 1 - b2 are formed in fp32 like in the kernel."""
    p, g, m, v = (t.detach().to(device='cpu', dtype=torch.float32).reshape(-1).clone() for t in (p, g, m, v))
    bc1 = 1.0 - b1 ** step if bc1 is None else bc1
    bc2 = 1.0 - b2 ** step if bc2 is None else bc2
    total = norm_emul32(g, inv_world)
    coef = _f32(max_norm) / (total + _f32(1e-6))
    coef = coef if (coef < 1.0 and max_norm > 0) else _f32(1.0)
    gs = coef * _f32(inv_world)
    step_size = _f32(lr) / _f32(bc1)
    bc2s = _f32(bc2).sqrt()
    gg = _f32(wd) * p + g * gs
    m1 = _f32(b1) * m + (_f32(1.0) - _f32(b1)) * gg
    v1 = _f32(b2) * v + ((_f32(1.0) - _f32(b2)) * gg) * gg
    p1 = p - step_size * (m1 / (v1.sqrt() / bc2s + _f32(eps)))
    return p1, m1, v1, float(total), float(coef)


# ---- the bound: |got - ref64| <= K * 2^-24 * scale + ulp32(ref) / 2, elementwise
def half_ulp32(ref):
    """half the spacing of fp32 at |ref| (float64 tensor in, float64 out; the subnormal spacing below 2^-126)"""
    e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1] - 1          # |ref| in [2^e, 2^(e+1))
    return torch.ldexp(torch.full_like(ref, 2.0 ** -24), e)


def worst_ratio(got, ref, scale, device='cpu'):
    """max over all elements of (|got - ref| - ulp32(ref)/2) / (2^-24 * scale): the K this result needs.  An element
    with scale 0 must be within ulp32(ref)/2 (else inf); NaN anywhere gives inf.  device: where the comparison itself is
    evaluated (in float64 either way)."""
    got = torch.as_tensor(got).detach().to(device=device, dtype=torch.float64).reshape(-1)
    ref = torch.as_tensor(ref).to(device=device, dtype=torch.float64).reshape(-1)
    scale = torch.as_tensor(scale).to(device=device, dtype=torch.float64).reshape(-1).expand_as(ref)
    if got.numel() != ref.numel() or not bool(torch.isfinite(got).all()):
        return float('inf')
    if got.numel() == 0:
        return 0.0
    excess = ((got - ref).abs() - half_ulp32(ref)).clamp_min(0.0)
    r = torch.where(excess > 0, excess / (EPS32 * scale), torch.zeros_like(excess))
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
    return float(r.max())


def step_ratios(got, ref, scales, device='cpu'):
    """got / ref: (p, m, v, total_norm, ...) of one step, tensors or lists of tensors -> dict(p=, m=, v=, norm=) of worst
    ratios"""
    flat = lambda x: torch.cat([t.reshape(-1) for t in x]) if isinstance(x, (list, tuple)) else x
    r = {k: worst_ratio(flat(got[i]), flat(ref[i]), flat(scales[k]), device) for i, k in enumerate(('p', 'm', 'v'))}
    one = lambda x: torch.tensor([float(x)], dtype=torch.float64)
    r['norm'] = worst_ratio(one(got[3]), one(ref[3]), one(scales['norm']))
    return r


# ---- K of the bound, per quantity: twice the worst ratio the fp32 emulation above reaches against the fp64 reference on
# the very inputs of the tests (the factor 2 allows for fma contraction and for another summation tree of the norm).
# tests/test_adam_ref.py re-measures the emulation on every case; profiles/adam_parity.txt holds the figures per case.
EMUL_STEP = dict(p=15.44, m=2.47, v=5.61, norm=0.50)      # worst over the 103 single-step cases (KERNEL_NS x REGIMES, 7 outliers)
K_STEP = {k: 2.0 * x for k, x in EMUL_STEP.items()}
# multi-step (the toy trajectories): the errors of p, m and v accumulate from step to step, so their bound at step t is
# K * t (t counted from where the trajectory starts); the figures are the worst ratio / t over the steps of the four
# trajectories.  The norm of a step does not depend on earlier ones.
EMUL_TRAJ = dict(p=0.72, m=2.27, v=5.20, norm=0.32)
K_TRAJ = {k: 2.0 * x for k, x in EMUL_TRAJ.items()}


def beyond(ratios, K, t=1):
    """the names of the quantities whose ratio exceeds the bound at step t (empty = pass)"""
    return [k for k, x in ratios.items() if not x <= K[k] * (t if k != 'norm' else 1)]


def flat_adam_emul32(params, grads_per_step, *, lr, b1=B1, b2=B2, eps=1e-8, wd=0.0, max_norm=1.0, inv_world=1.0,
                     m=None, v=None, step0=0):
    """flat_adam_ref in fp32 over FlatAdam's arena (every slot padded to a multiple of 4 floats); grads_per_step holds
    the gradients as the arena sees them (the SUM over ranks).  Yields (params, m, v, total_norm, coef) per step."""
    sizes = [t.numel() for t in params]
    pads = [(-k) & 3 for k in sizes]
    flat = lambda ts: torch.cat([torch.cat([t.detach().to(device='cpu', dtype=torch.float32).reshape(-1),
                                            torch.zeros(pd, dtype=torch.float32)]) for t, pd in zip(ts, pads)])
    split = lambda a: [c[:k].view_as(t) for c, k, t in zip(a.split([k + pd for k, pd in zip(sizes, pads)]), sizes, params)]
    P = flat(params)
    M = torch.zeros_like(P) if m is None else flat(m)
    V = torch.zeros_like(P) if v is None else flat(v)
    for k, grads in enumerate(grads_per_step):
        lr_k = lr[k] if isinstance(lr, (list, tuple)) else lr
        G = flat([torch.zeros_like(t) if g is None else g for t, g in zip(params, grads)])
        p1, m1, v1, total, coef = clip_adam_emul32(P, G, M, V, step=step0 + k + 1, lr=lr_k, b1=b1, b2=b2, eps=eps, wd=wd,
                                                   max_norm=max_norm, inv_world=inv_world)
        olds, news = (split(P), split(M), split(V)), (split(p1), split(m1), split(v1))
        P, M, V = (flat([o if g is None else w for o, w, g in zip(old, new, grads)]) for old, new in zip(olds, news))
        yield split(P), split(M), split(V), total, coef


# ---- the cases of tests/test_optim_gpu.py (here, so that tests/test_adam_ref.py can run their fp32 emulation on the CPU)
KERNEL_NS = (1, 3, 4, 7, SUMSQ_SWEEP, SUMSQ_SWEEP + 4, CLIP_SWEEP + 4, 2 * CLIP_SWEEP + 3075)     # ..., 4 197 379
HYPER = dict(lr=1e-3, b1=B1, b2=B2, eps=1e-8)
# norm: ||g|| as it sits in the arena (before inv_world); first: step 1 with m = v = 0, else step 7 with random m, v > 0
REGIMES = {
    'active_late':        dict(norm=3.7, max_norm=1.0, inv_world=1.0, wd=0.0, first=False),
    'active_late_wd':     dict(norm=3.7, max_norm=1.0, inv_world=1.0, wd=1e-2, first=False),
    'active_first':       dict(norm=3.7, max_norm=1.0, inv_world=1.0, wd=0.0, first=True),
    'inactive_late':      dict(norm=0.4, max_norm=1.0, inv_world=1.0, wd=0.0, first=False),
    'inactive_first_wd':  dict(norm=0.4, max_norm=1.0, inv_world=1.0, wd=1e-2, first=True),
    'noclip_late_wd':     dict(norm=3.7, max_norm=0.0, inv_world=1.0, wd=1e-2, first=False),
    'world4_active':      dict(norm=14.0, max_norm=1.0, inv_world=0.25, wd=0.0, first=False),
    'world4_inactive_wd': dict(norm=2.0, max_norm=1.0, inv_world=0.25, wd=1e-2, first=True),
    'zero_late':          dict(norm=0.0, max_norm=1.0, inv_world=1.0, wd=0.0, first=False),
    'zero_first':         dict(norm=0.0, max_norm=1.0, inv_world=1.0, wd=0.0, first=True),
    'zero_first_wd':      dict(norm=0.0, max_norm=1.0, inv_world=1.0, wd=1e-2, first=True),
    'zero_late_wd':       dict(norm=0.0, max_norm=1.0, inv_world=1.0, wd=1e-2, first=False),
}
_INPUTS = {}


def kernel_inputs(n):
    """(p, g of unit norm in float64, m, v) for an arena of n floats, seeded by n.  p carries the sign of g, so that
    wd * p + g * coef never cancels: the scales of the bound are relative to |gg|, and an fp32 sum that cancels to 1e-6 of
    its terms (some element among four million does) has no relative accuracy left to test."""
    if n not in _INPUTS:
        if len(_INPUTS) >= 2:
            _INPUTS.clear()
        gen = torch.Generator().manual_seed(1000 + n % 9973)
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        g = g / g.norm()
        p = (0.3 * torch.randn(n, generator=gen)).abs() * torch.sign(g).float()
        m = 1e-3 * torch.randn(n, generator=gen)
        v = 1e-6 * (torch.rand(n, generator=gen) + 0.01)
        _INPUTS[n] = (p, g, m, v)
    return _INPUTS[n]


def kernel_case(n, regime):
    """-> (p, g, m, v, hyper): fp32 CPU tensors and the keyword arguments of clip_adam_ref"""
    r = REGIMES[regime]
    p, g, m, v = kernel_inputs(n)
    g = (g * r['norm']).float()
    if r['first']:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    return p, g, m, v, dict(HYPER, step=1 if r['first'] else 7, wd=r['wd'], max_norm=r['max_norm'], inv_world=r['inv_world'])


OUTLIER_N = KERNEL_NS[-1]
OUTLIER_AT = dict(first=0, end_of_norm_sweep=SUMSQ_SWEEP - 1, start_of_norm_sweep_2=SUMSQ_SWEEP,
                  end_of_update_sweep=CLIP_SWEEP - 1, start_of_update_sweep_2=CLIP_SWEEP,
                  last_float4=(OUTLIER_N & ~3) - 1, tail=OUTLIER_N - 1)


def outlier_case(where):
    """one gradient of 1e3 among N(0, 1e-2) noise: step 1, m = v = 0, clip active (coef ~ 1e-3)"""
    gen = torch.Generator().manual_seed(77)
    n = OUTLIER_N
    g = 1e-2 * torch.randn(n, generator=gen)
    g[OUTLIER_AT[where]] = 1e3
    p = 0.3 * torch.randn(n, generator=gen)
    z = torch.zeros(n)
    return p, g, z, z.clone(), dict(HYPER, step=1, wd=0.0, max_norm=1.0, inv_world=1.0)


# the toy module of the FlatAdam tests: slot padding of 3, 1, 3, 0, 1, 1, 0, 3, 0, 1 floats; 2 176 440 floats in the arena,
# so the slots behind the sixth tensor lie in the second and third sweep of k_sumsq and the last one in the second sweep of
# k_clip_adam
TOY_SHAPES = ((1,), (3,), (5,), (8, 8), (1023,), (1031, 1021), (64, 64), (70001,), (1024, 1024), (7,))
TOY_ZERO_GRAD = 7            # this tensor's gradient is identically zero (weight decay still moves it)
TOY_STEPS = 20
TOY_WD = 1e-2
TOY_LR = (1e-3,) * 10 + (4e-4,) * 10          # param_groups[0]['lr'] changes half-way


def toy_params():
    """|p| >= 0.1: no weight changes sign within TOY_STEPS steps of at most ~3e-3 each"""
    gen = torch.Generator().manual_seed(4242)
    out = []
    for s in TOY_SHAPES:
        sign = torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0)
        out.append(sign * (0.1 + 0.3 * torch.randn(*s, generator=gen).abs()))
    return out


TOY_NO_GRAD = (4, (5, 12))    # toy_grads(no_grad=True): this tensor has no gradient on these (1-based) steps


def toy_grads(steps=TOY_STEPS, no_grad=False):
    """per step one fp32 gradient per tensor; the global norm alternates between ~3 (clipped) and ~0.3 (not clipped) in
    runs of different length.  Every gradient element keeps the sign of its weight: wd * p + g * coef and
    b1 * m + (1 - b1) * gg then never cancel.  The scales of the bound are relative to |gg| and |m|, and a sum that
    cancels to 1e-5 of its terms (one among two million elements does, every step) has no relative accuracy in fp32."""
    gen = torch.Generator().manual_seed(2424)
    numel = sum(torch.Size(s).numel() for s in TOY_SHAPES)
    signs = [torch.sign(p) for p in toy_params()]
    out = []
    for k in range(steps):
        norm = 3.0 if (k % 5) in (0, 1, 3) else 0.3
        gs = [sg * torch.randn(*s, generator=gen).abs() * (norm / math.sqrt(numel)) for s, sg in zip(TOY_SHAPES, signs)]
        gs[TOY_ZERO_GRAD] = torch.zeros(*TOY_SHAPES[TOY_ZERO_GRAD])
        if no_grad and k + 1 in TOY_NO_GRAD[1]:
            gs[TOY_NO_GRAD[0]] = None
        out.append(gs)
    return out


def worst_per_step(worst, ratios, t):
    """fold the ratios of step t into `worst`: p, m, v divided by t (their bound grows with t), the norm as it is"""
    for k, x in ratios.items():
        worst[k] = max(worst.get(k, 0.0), x / (t if k != 'norm' else 1))
    return worst


def parity_log(case, emul=None, got=None):
    """append one line of worst ratios to the file $T2V_ADAM_PARITY names (profiles/adam_parity.txt is made this way)"""
    import os
    path = os.environ.get('T2V_ADAM_PARITY')
    if not path:
        return
    fmt = lambda r: ' '.join('%s=%.3f' % (k, r[k]) for k in ('p', 'm', 'v', 'norm') if k in r)
    with open(path, 'a') as f:
        f.write('%-44s %s\n' % (case, ' | '.join(('%s: %s' % (nm, fmt(r))) for nm, r in (('fp32-cpu', emul), ('hip', got)) if r)))
