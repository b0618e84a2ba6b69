"""tests/guided_ref.py on its own (no GPU): its gradient is autograd's, an identity alignment costs nothing, and nothing outside
the lengths contributes."""
import torch

import guided_ref as G

LENS = dict(in_lengths=(21, 10, 1), out_lengths=(7, 4, 1))


def _align(B=3, T=7, T_in=21, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(B, T, T_in, generator=g, dtype=torch.float64), -1)


def test_reference_gradient_equals_autograd():
    for sigma in (0.4, 0.2):
        a = _align().requires_grad_(True)
        G.loss(a, sigma=sigma, **LENS).backward()
        want = G.grad(LENS['in_lengths'], LENS['out_lengths'], 7, 21, sigma)
        # (autograd multiplies W by the rounded 1 / D where grad() divides: two fp64 roundings against one)
        assert ((a.grad - want).abs() <= 2.0 ** -51 * want.abs()).all()
        assert torch.equal(a.grad == 0, want == 0) and want.abs().max() > 0


def test_identity_alignment_with_equal_lengths_costs_nothing():
    n = 9
    a = torch.eye(n, dtype=torch.float64).unsqueeze(0)
    assert G.loss(a, (n,), (n,)).item() == 0.0
    # and one step off the diagonal costs 1 - exp(-(1 / n)^2 / (2 sigma^2)) per row that has moved
    shifted = torch.roll(a, 1, 2)
    w1 = 1.0 - torch.exp(torch.tensor(-(1.0 / n) ** 2 / (2 * 0.4 ** 2), dtype=torch.float64))
    w8 = 1.0 - torch.exp(torch.tensor(-(8.0 / n) ** 2 / (2 * 0.4 ** 2), dtype=torch.float64))
    want = ((n - 1) * w1 + w8) / (n * n)
    assert abs(G.loss(shifted, (n,), (n,)).item() - want.item()) < 1e-15


def test_nothing_outside_the_lengths_contributes():
    a = _align()
    base = G.loss(a, **LENS)
    b = a.clone()
    for i, (n, t) in enumerate(zip(LENS['in_lengths'], LENS['out_lengths'])):
        b[i, t:] = 7.0
        b[i, :, n:] = -3.0
    assert G.loss(b, **LENS).item() == base.item()
    w = G.weights(LENS['in_lengths'], LENS['out_lengths'], 7, 21)
    for i, (n, t) in enumerate(zip(LENS['in_lengths'], LENS['out_lengths'])):
        assert w[i, t:].abs().max().item() == 0.0 if t < 7 else True
        assert w[i, :, n:].abs().max().item() == 0.0 if n < 21 else True
        assert w[i, :t, :n].min().item() >= 0.0 and w[i, :t, :n].max().item() < 1.0
    # lengths of one: no division by zero, a single free cell
    assert w[2, 0, 0].item() == 0.0 and torch.isfinite(w).all()
    assert G.denominator(**LENS) == 21 * 7 + 10 * 4 + 1
