"""Guided attention loss in fp64 torch, written from the formula — TEST INFRASTRUCTURE, NOT PRODUCT.

  W[b][t][j] = 1 - exp(-(j / N_b - t / T_b)^2 / (2 sigma^2))    for t < T_b and j < N_b, else 0
  D = sum_b T_b N_b,   L = sum A W / D,   dL/dA = W / D

(Tachibana et al., DCTTS; ESPnet's GuidedAttentionLoss, default sigma 0.4.)  Indices run from 0."""
import torch


def weights(in_lengths, out_lengths, T, T_in, sigma=0.4):
    """W (B, T, T_in) in fp64"""
    N = torch.as_tensor(in_lengths).double().view(-1, 1, 1)
    Tb = torch.as_tensor(out_lengths).double().view(-1, 1, 1)
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1)
    j = torch.arange(T_in, dtype=torch.float64).view(1, 1, T_in)
    w = 1.0 - torch.exp(-(j / N - t / Tb) ** 2 / (2.0 * sigma ** 2))
    return torch.where((t < Tb) & (j < N), w, torch.zeros_like(w))


def denominator(in_lengths, out_lengths):
    return float((torch.as_tensor(in_lengths).double() * torch.as_tensor(out_lengths).double()).sum())


def loss(align, in_lengths, out_lengths, sigma=0.4):
    """L as a 0-d fp64 tensor (differentiable in align)"""
    B, T, T_in = align.shape
    return (align.double() * weights(in_lengths, out_lengths, T, T_in, sigma)).sum() / denominator(in_lengths, out_lengths)


def grad(in_lengths, out_lengths, T, T_in, sigma=0.4):
    """dL/dA = W / D (B, T, T_in) in fp64"""
    return weights(in_lengths, out_lengths, T, T_in, sigma) / denominator(in_lengths, out_lengths)
