"""Tacotron2Loss_VAE (reference loss_function.py:6-44): 2×MSE + BCE-with-logits + w(step)·KL
(+ hparams.guided_attention_weight × the guided attention loss, a recipe switch that is off by default)."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F


def kl_anneal_weight(kind, step, lag, k, x0, upper):
    if kind == 'logistic':
        return float(upper / (upper + np.exp(-k * (step - x0))))   # np.exp like the reference (1-ulp exact)
    if kind == 'linear':
        return min(upper, step / x0) if step > lag else 0
    if kind == 'constant':
        return 0.001
    return None   # reference falls through to None for unknown names


class Tacotron2Loss_VAE(nn.Module):
    def __init__(self, hparams):
        super().__init__()
        self.anneal_function = hparams.anneal_function
        self.lag, self.k = hparams.anneal_lag, hparams.anneal_k
        self.x0, self.upper = hparams.anneal_x0, hparams.anneal_upper
        # (getattr: the reference's hparams know neither)
        self.guided_weight = float(getattr(hparams, 'guided_attention_weight', 0.0))
        self.guided_sigma = float(getattr(hparams, 'guided_attention_sigma', 0.4))
        self.guided = None      # the detached, unweighted guided attention term of the most recent training call

    def kl_anneal_function(self, anneal_function, lag, step, k, x0, upper):
        return kl_anneal_weight(anneal_function, step, lag, k, x0, upper)

    def forward(self, model_output, targets, step, lengths=None):
        """lengths = (input_lengths, output_lengths): what the guided attention term needs (guided_attention_weight > 0).
        The term is a training aid: it is added where gradients are recorded and left out under no_grad (validation)."""
        if self.guided_weight > 0 and lengths is None:
            raise ValueError("guided_attention_weight > 0 needs lengths=(input_lengths, output_lengths)")
        total, recon, kl, w = self._reference(model_output, targets, step)
        if self.guided_weight > 0:
            if torch.is_grad_enabled():
                import t2v_hip
                g = t2v_hip.GuidedAttention.apply(model_output[3], lengths[0], lengths[1], self.guided_sigma)
                self.guided = g.detach()
                total = total + self.guided_weight * g
        return total, recon, kl, w

    def _reference(self, model_output, targets, step):
        mel_out, mel_post, gate_out, _, mu, logvar = model_output[:6]
        w = kl_anneal_weight(self.anneal_function, step, self.lag, self.k, self.x0, self.upper)
        if mel_out.is_cuda:      # fused value+gradient kernel
            import t2v_hip
            total, out4 = t2v_hip.VAELoss.apply(mel_out, mel_post, gate_out, mu, logvar, targets[0].detach(),
                                                targets[1].detach(), w)
            return total, out4[1], out4[2], w
        mel_target, gate_target = targets[0].detach(), targets[1].detach().reshape(-1, 1)
        recon = (F.mse_loss(mel_out, mel_target) + F.mse_loss(mel_post, mel_target)
                 + F.binary_cross_entropy_with_logits(gate_out.reshape(-1, 1), gate_target))
        kl = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())   # SUM over batch and latent dims
        w = kl_anneal_weight(self.anneal_function, step, self.lag, self.k, self.x0, self.upper)
        return recon + w * kl, recon, kl, w
