"""References for the KL control of the training loss (csrc/kl_control.hip, loss_function.Tacotron2Loss_VAE with kl_free_bits /
kl_capacity): the objective written with torch autograd from its definition — no hand-derived gradient — and a numpy reference of
the monitor.  Shared by tests/test_klc_ref.py (CPU: the reference against the oracle and against its own definition) and
tests/test_kl_control_gpu.py (the kernel against the fp64 reference).

  kl[b,d] = 0.5 (mu^2 + exp(logvar) - logvar - 1)     k[d] = mean_b kl[b,d]     KL = sum_b sum_d kl[b,d]
  K' = B sum_d max(k[d], lambda), dimension d floored when k[d] <= lambda (lambda == 0: off, K' = KL)
  T = |K' - B C|  (C < 0: off, T = K')                 total = recon + w T

Inputs: mu[:, d] = randn * 0.03 * 1.2^d and logvar[:, d] = randn * 0.3 * min(0.03 * 1.2^d, 1) at D = 32: with lambda = 0.05 twelve to
fifteen dimensions lie under the floor and K'/B is between 60 and 155 nats, so C = 20 and C = 300 straddle every case.  The seeds
keep every k[d] at least 1 % away from lambda (tests/test_klc_ref.py asserts it), so that round-off cannot decide which dimensions
are floored."""
import functools

import numpy as np
import torch
from torch.nn import functional as F

D = 32
LAMBDA = 0.05
CAPACITIES = (20.0, 300.0)
BATCHES = (1, 2, 3, 6, 16, 64)
# (B, T) of the parity cases: mel (B, 80, T), gate (B, T).  (6, 400): every one of the launch's 64 workgroups has mel work
SHAPES = tuple((B, 5) for B in BATCHES) + ((6, 400),)
# (name, free bits, capacity): free bits alone, capacity alone below and above K'/B, both together
MODES = (('free_bits', LAMBDA, -1.0), ('capacity_below', 0.0, CAPACITIES[0]), ('capacity_above', 0.0, CAPACITIES[1]),
         ('both_below', LAMBDA, CAPACITIES[0]), ('both_above', LAMBDA, CAPACITIES[1]))
# seed 1000 + B keeps the 1 % margin at every B but 16 (0.8 % there): B = 16 has a seed of its own
SEEDS = {16: 2016}


def seed_of(B):
    return SEEDS.get(B, 1000 + B)


@functools.lru_cache(maxsize=None)
def inputs(B, T=5, dims=D):
    """(mel, post, gate, mu, logvar, mel_t, gate_t) fp32 on the host; the latents depend on B and dims alone (drawn first).
    Past dimension 31 the scales start over (1.2^d would leave fp32's range); fewer than 32 dimensions take the upper end of the
    ladder, so that the largest gradient of every case is of order one and the bounds mean the same at every shape."""
    g = torch.Generator().manual_seed(seed_of(B))
    scale = 0.03 * 1.2 ** ((torch.arange(dims) + max(0, 32 - dims)) % 32).double()
    mu = (torch.randn(B, dims, generator=g, dtype=torch.float64) * scale).float()
    logvar = (torch.randn(B, dims, generator=g, dtype=torch.float64) * 0.3 * scale.clamp(max=1.0)).float()
    mel, post = torch.randn(B, 80, T, generator=g), torch.randn(B, 80, T, generator=g)
    gate = torch.randn(B, T, generator=g) * 3
    mel_t, gate_t = torch.randn(B, 80, T, generator=g), (torch.rand(B, T, generator=g) > 0.9).float()
    return mel, post, gate, mu, logvar, mel_t, gate_t


def kl_terms(mu, logvar):
    return 0.5 * (mu * mu + logvar.exp() - logvar - 1)


def objective(tensors, w, free_bits=0.0, capacity=-1.0, dtype=torch.float64):
    """The objective in `dtype` with gradients from autograd.  Returns a dict: total, recon, kl (raw), kp (K'), T, s, floored
    (bool (D,)), n_floored, k ((D,)), grads (dmel, dpost, dgate, dmu, dlogvar)."""
    mel, post, gate, mu, logvar = (t.detach().to(dtype).clone().requires_grad_(True) for t in tensors[:5])
    mel_t, gate_t = tensors[5].to(dtype), tensors[6].to(dtype)
    B = mu.shape[0]
    recon = (F.mse_loss(mel, mel_t) + F.mse_loss(post, mel_t)
             + F.binary_cross_entropy_with_logits(gate.reshape(-1, 1), gate_t.reshape(-1, 1)))
    kl_bd = kl_terms(mu, logvar)
    kl = kl_bd.sum()
    k = kl_bd.mean(0)
    floored = torch.zeros_like(k, dtype=torch.bool)
    if free_bits > 0:
        floored = k.detach() <= free_bits
        kp = B * torch.where(floored, torch.full_like(k, free_bits), k).sum()
    else:
        kp = kl
    if capacity >= 0:
        diff = kp - B * capacity
        T = diff.abs()                  # autograd's sign(diff): 0 at equality
        s = float(torch.sign(diff.detach()))
    else:
        T, s = kp, 1.0
    total = recon + w * T
    grads = torch.autograd.grad(total, (mel, post, gate, mu, logvar))
    return {'total': total.detach(), 'recon': recon.detach(), 'kl': kl.detach(), 'kp': kp.detach(), 'T': T.detach(), 's': s,
            'floored': floored, 'n_floored': int(floored.sum()), 'k': k.detach(), 'grads': grads}


def floor_margin(k, free_bits):
    """the smallest |k[d] - lambda| / lambda over the dimensions"""
    return float(((k.double() - free_bits).abs() / free_bits).min())


def monitor_reference(batches):
    """What the monitor holds after one launch per (mu, logvar) pair of `batches` (fp32 arrays (B_i, D)), from all rows at once in
    fp64 (two passes: no merge): {'n', 'launches', 'mean', 'm2', 'sum_kl'}."""
    mus = np.concatenate([np.asarray(m, dtype=np.float64) for m, _ in batches])
    lvs = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in batches])
    mean = mus.mean(axis=0)
    return {'n': len(mus), 'launches': len(batches), 'mean': mean, 'm2': ((mus - mean) ** 2).sum(axis=0),
            'sum_kl': (0.5 * (mus * mus + np.exp(lvs) - lvs - 1)).sum(axis=0)}
