"""fp64 reference of the weight average that t2v_clip_adam_ema_step_guarded keeps beside Adam (csrc/optim.hip,
optim.FlatAdam(ema_decay=)), an fp32 emulation of its arithmetic in numpy, and the error bound that tests/test_ema_gpu.py and
tests/test_ema_engine_gpu.py hold the kernel to.  Plain torch / numpy on the CPU.

The update, as include/t2vae.h documents it:
    rate_t = max(rate, 9 / (10 + t))  with warm-up, else rate        (TensorFlow's min(decay, (1 + t) / (10 + t)) as a rate)
    s      = s + rate_t * (p_new - s)                                 (p_new: the fp32 parameter the step stored)
rate = 1 - decay crosses the C ABI as a float, rounded once from the double 1 - decay: every side of a comparison works
with rate32(decay), that fp32 value (as adam_ref does with the betas).

The bound.  Per step the fp32 form commits one rounding of the result (<= 2^-24 |s|) plus roundings of the rate and of the
difference (each <= 2^-24 rate_t |p - s|); an error already in s is carried forward with the factor 1 - rate_t < 1.  So after
t steps, per element,
    |s32 - s64| <= K * t * 2^-24 * scale,      scale = the running maximum over the steps of |s| + 2 rate_t |p - s|
(|s| and |p - s| of the fp64 side, before the step's update).  K is fixed the way adam_ref.K_STEP is: twice the worst ratio the
numpy emulation below reaches against the fp64 reference, over the cases of the GPU tests and over a longer trial (200 steps,
70 001 elements, decays 0.5 / 0.99 / 0.9999, with and without warm-up); the factor 2 allows for the kernel's fused
multiply-add and for the weights the shadow follows being another trajectory's.  tests/test_ema_ref.py re-measures the emulation on
every case.  K is never taken from the kernel's output.
"""
import numpy as np
import torch

EPS32 = 2.0 ** -24


def rate32(decay):
    """1 - decay in double, rounded once to fp32: the value the kernel runs at, as a Python float"""
    return float(np.float32(1.0 - float(decay)))


def rate_t(rate, warmup, t):
    """the rate of update t (0-based) in double"""
    return max(rate, 9.0 / (10.0 + float(t))) if warmup else rate


def ema_ref(s, p_new, rate, warmup, t):
    """one update on float64 copies -> (s_new, scale); scale = |s| + 2 rate_t |p_new - s| from the values before the update"""
    s = s.detach().to(dtype=torch.float64)
    p = p_new.detach().to(device=s.device, dtype=torch.float64)
    r = rate_t(rate, warmup, t)
    d = p - s
    return s + r * d, s.abs() + 2.0 * r * d.abs()


def ema_emul32(s, p_new, rate, warmup, t):
    """the same update in numpy fp32, every operation rounded on its own (no fused multiply-add), rate_t formed in fp32
    as the kernel forms it: 9.0f / (10.0f + (float)t)"""
    s = np.asarray(s, dtype=np.float32)
    p = np.asarray(p_new, dtype=np.float32)
    r = np.float32(rate)
    if warmup:
        r = np.maximum(r, np.float32(9.0) / (np.float32(10.0) + np.float32(t)))
    d = (p - s).astype(np.float32)
    return (s + (r * d).astype(np.float32)).astype(np.float32)


def worst_ratio(got, ref, scale, t=1):
    """max over the elements of |got - ref| / (t * 2^-24 * scale): the K this result needs at step t.  An element with scale 0
    must be exact (else inf); NaN or inf anywhere gives inf.  Evaluated in float64 where `ref` lives."""
    ref = torch.as_tensor(ref).to(dtype=torch.float64).reshape(-1)
    got = torch.as_tensor(got).detach().to(device=ref.device, dtype=torch.float64).reshape(-1)
    scale = torch.as_tensor(scale).to(device=ref.device, dtype=torch.float64).reshape(-1)
    if got.numel() != ref.numel() or not bool(torch.isfinite(got).all()):
        return float('inf')
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(err > 0, err / (float(t) * EPS32 * scale), torch.zeros_like(err))
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
    return float(r.max())


# ---- the single-step cases of tests/test_ema_gpu.py: (warm-up, t).  With warm-up the rate is 0.9, 0.6 and (t = 10^6: the
# decay's own) 1e-4; without it 1e-4 whatever t says.
DECAY = 0.9999
STEP_CASES = ((True, 0), (True, 5), (True, 10 ** 6), (False, 3))


def shadow_for(p, seed=0):
    """a shadow that trails the weights p (fp32 CPU tensor): p + N(0, 0.02^2), seeded by the size"""
    gen = torch.Generator().manual_seed(31337 + seed + p.numel() % 9973)
    return (p.float() + 0.02 * torch.randn(p.numel(), generator=gen).view_as(p)).float()


# ---- a trajectory on prescribed weights (the emulation's long trial, and what test_ema_ref.py checks the oracle on)
def trial_weights(n, steps, seed=7):
    """fp32 weights of `steps` steps: a random start of ~0.3 and a random walk of ~1e-3 per step (an Adam step at lr 1e-3)"""
    gen = torch.Generator().manual_seed(seed)
    p = (0.3 * torch.randn(n, generator=gen)).float()
    out = []
    for _ in range(steps):
        p = (p + 1e-3 * torch.randn(n, generator=gen)).float()
        out.append(p)
    return out


def trajectory_ratio(weights, decay, warmup, s0=None):
    """the emulation against the reference along `weights` (one fp32 tensor per step), both started from s0 (default: the
    first weights): the worst over the steps of worst_ratio(..., t), the scale being the running maximum"""
    rate = rate32(decay)
    s64 = (weights[0] if s0 is None else s0).double()
    s32 = s64.float().numpy()
    scale = torch.zeros_like(s64)
    worst = 0.0
    for t, p in enumerate(weights):
        s64, sc = ema_ref(s64, p, rate, warmup, t)
        scale = torch.maximum(scale, sc)
        s32 = ema_emul32(s32, p.numpy(), rate, warmup, t)
        worst = max(worst, worst_ratio(torch.from_numpy(s32), s64, scale, t + 1))
    return worst


# ---- K of the bound: twice the worst ratio of the emulation (tests/test_ema_ref.py re-measures every figure)
#   single step, the 48 cases of test_ema_gpu.py (6 sizes x 2 regimes x STEP_CASES)       1.549
#   20 steps along the toy trajectories of adam_ref (decay 0.99 warm-up, 0.9999 none)      0.836
#   200 steps, 70 001 elements, decays 0.5 / 0.99 / 0.9999: without warm-up                0.731
#                                                            with warm-up                  0.472
# (a single step's worst case is the first warm-up update, rate 0.9, where |p - s| dwarfs |s|: the three roundings of the
# increment and the one of the result then add up to almost 2 * 2^-24 * 2 rate |p - s|.)
EMUL = dict(step=1.55, toy=0.84, trial=0.74, trial_warmup=0.48)
K_EMA = 2.0 * max(EMUL.values())


def bound(scale, t=1):
    """the tolerance per element at step t (1-based) for a running-maximum scale"""
    return K_EMA * float(t) * EPS32 * scale
