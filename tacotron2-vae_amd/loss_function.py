"""Tacotron2Loss_VAE (reference loss_function.py:6-44): 2×MSE + BCE-with-logits + w(step)·KL
(+ hparams.guided_attention_weight × the guided attention loss, a recipe switch that is off by default;
 hparams.kl_free_bits / hparams.kl_capacity reshape the KL term of the training loss, both off by default)."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F


def kl_anneal_weight(kind, step, lag, k, x0, upper, cycle=10000, ratio=0.5):
    if kind == 'logistic':
        return float(upper / (upper + np.exp(-k * (step - x0))))   # np.exp like the reference (1-ulp exact)
    if kind == 'linear':
        return min(upper, step / x0) if step > lag else 0
    if kind == 'constant':
        return 0.001
    if kind == 'cyclical':      # Fu et al. 2019: ramp over the first `ratio` of every cycle, then hold (ratio 0: hold all the way)
        p = (step % cycle) / cycle
        return float(upper * min(1.0, p / ratio)) if ratio > 0 else float(upper)
    return None   # reference falls through to None for unknown names


class Tacotron2Loss_VAE(nn.Module):
    def __init__(self, hparams):
        super().__init__()
        self.anneal_function = hparams.anneal_function
        self.lag, self.k = hparams.anneal_lag, hparams.anneal_k
        self.x0, self.upper = hparams.anneal_x0, hparams.anneal_upper
        # (getattr: the reference's hparams know none of these)
        self.guided_weight = float(getattr(hparams, 'guided_attention_weight', 0.0))
        self.guided_sigma = float(getattr(hparams, 'guided_attention_sigma', 0.4))
        self.guided = None      # the detached, unweighted guided attention term of the most recent training call
        self.cycle = int(getattr(hparams, 'anneal_cycle', 10000))
        self.ratio = float(getattr(hparams, 'anneal_ratio', 0.5))
        self.free_bits = float(getattr(hparams, 'kl_free_bits', 0.0))
        self.capacity = float(getattr(hparams, 'kl_capacity', -1.0))
        if not self.free_bits >= 0:
            raise ValueError("kl_free_bits is nats per latent dimension: 0 (off) or more, got %r" % self.free_bits)
        if self.capacity != self.capacity:
            raise ValueError("kl_capacity is nats per utterance (negative: off), got %r" % self.capacity)
        if self.cycle < 1:
            raise ValueError("anneal_cycle is steps per cycle: 1 or more, got %r" % self.cycle)
        if not 0 <= self.ratio <= 1:
            raise ValueError("anneal_ratio is the share of a cycle spent ramping: 0..1, got %r" % self.ratio)
        self.monitor = None     # a t2v_hip.KLMonitor the training loss launch updates (the engine installs it)
        # detached K', T and the number of floored dimensions of the most recent training call that went through the KL control launch
        self.kl_floored_sum = self.kl_objective = self.kl_floored_dims = None

    @property
    def kl_control(self):
        return self.free_bits > 0 or self.capacity >= 0

    def kl_weight(self, step):
        return kl_anneal_weight(self.anneal_function, step, self.lag, self.k, self.x0, self.upper, self.cycle, self.ratio)

    def kl_anneal_function(self, anneal_function, lag, step, k, x0, upper):
        return kl_anneal_weight(anneal_function, step, lag, k, x0, upper, self.cycle, self.ratio)

    def forward(self, model_output, targets, step, lengths=None):
        """lengths = (input_lengths, output_lengths): what the guided attention term needs (guided_attention_weight > 0).
        The term is a training aid: it is added where gradients are recorded and left out under no_grad (validation).
        Free bits and the capacity target are training aids in the same way: under no_grad the loss is the reference's."""
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
        w = self.kl_weight(step)
        controlled = (self.kl_control or self.monitor is not None) and torch.is_grad_enabled()
        if mel_out.is_cuda and controlled:      # value + gradient + monitor update, still one launch (csrc/kl_control.hip)
            import t2v_hip
            total, out8 = t2v_hip.VAELossKLC.apply(mel_out, mel_post, gate_out, mu, logvar, targets[0].detach(),
                                                   targets[1].detach(), w, self.free_bits, self.capacity, self.monitor)
            self.kl_floored_sum, self.kl_objective, self.kl_floored_dims = out8[4], out8[5], out8[6]
            return total, out8[1], out8[2], w
        if mel_out.is_cuda:      # fused value+gradient kernel
            import t2v_hip
            total, out4 = t2v_hip.VAELoss.apply(mel_out, mel_post, gate_out, mu, logvar, targets[0].detach(),
                                                targets[1].detach(), w)
            return total, out4[1], out4[2], w
        if controlled and self.kl_control:
            raise NotImplementedError("kl_free_bits / kl_capacity run in the HIP loss launch: the outputs must be on the GPU")
        mel_target, gate_target = targets[0].detach(), targets[1].detach().reshape(-1, 1)
        recon = (F.mse_loss(mel_out, mel_target) + F.mse_loss(mel_post, mel_target)
                 + F.binary_cross_entropy_with_logits(gate_out.reshape(-1, 1), gate_target))
        kl = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())   # SUM over batch and latent dims
        return recon + w * kl, recon, kl, w
