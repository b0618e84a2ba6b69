"""`stft.STFT` with the reference's constructor and `transform` / `inverse` / `forward` surface (reference stft.py:42-140),
backed by the HIP kernels of csrc/vocoder.hip (hand-written 1024-point real FFT per wavefront) instead of convolutions
with a dense DFT basis.  Only the front end's geometry n_fft = win = 1024, hop = 256, 'hann' is built."""
import numpy as np
import torch
from torch import nn


def fft_tables(n_fft):
    """periodic Hann window (scipy `get_window('hann', n, fftbins=True)`), exp(-2 pi i k/512) (512,2) and
    exp(-2 pi i k/1024) (513,2) as float32 — the tables of the packed 512-point FFT."""
    n = np.arange(n_fft)
    window = (0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)).astype(np.float32)
    k = np.arange(n_fft // 2)
    tw512 = np.stack((np.cos(2 * np.pi * k / (n_fft // 2)), -np.sin(2 * np.pi * k / (n_fft // 2))), 1).astype(np.float32)
    k = np.arange(n_fft // 2 + 1)
    tw1024 = np.stack((np.cos(2 * np.pi * k / n_fft), -np.sin(2 * np.pi * k / n_fft)), 1).astype(np.float32)
    return dict(window=window, tw512=tw512, tw1024=tw1024)


class STFT(nn.Module):
    """Reference signature; any geometry but (1024, 256, 1024, 'hann') raises NotImplementedError.  The tables are plain
    attributes, so the module adds no state_dict keys (TacotronSTFT's stay ['mel_basis']).  CPU input is copied to the
    GPU; results come back on the input's device.  `lengths` (optional) are per-utterance sample counts for `transform`
    and frame counts for `inverse`; everything past a length is zero."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window='hann'):
        super().__init__()
        if (filter_length, hop_length, win_length, window) != (1024, 256, 1024, 'hann'):
            raise NotImplementedError("the HIP STFT is built for filter_length=win_length=1024, hop_length=256, 'hann'")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.forward_transform = None
        self._host_tables = fft_tables(filter_length)
        self._dev_tables = {}

    def tables(self, device):
        key = str(device)
        if key not in self._dev_tables:
            self._dev_tables[key] = {k: torch.from_numpy(v).to(device) for k, v in self._host_tables.items()}
        return self._dev_tables[key]

    @staticmethod
    def on_gpu(x):
        import t2v_hip
        if not torch.cuda.is_available():
            raise t2v_hip.T2VHipError("STFT needs a GPU: its transforms are HIP-only")
        return (x if x.is_cuda else x.cuda()).float()

    def transform(self, input_data, lengths=None):
        """(B, N) samples -> magnitude, phase (B, 513, N//256 + 1).  Needs N > 512 (the reflect pad of 512)."""
        import t2v_hip
        x = self.on_gpu(input_data)
        self.num_samples = x.size(1)
        magnitude, phase = t2v_hip.stft_polar(x, lengths, self.tables(x.device))
        return magnitude.to(input_data.device), phase.to(input_data.device)

    def inverse(self, magnitude, phase, lengths=None):
        """magnitude, phase (B, 513, T) -> (B, 1, (T-1)*256), as the reference's conv_transpose1d output."""
        import t2v_hip
        m, p = self.on_gpu(magnitude), self.on_gpu(phase)
        return t2v_hip.istft(m, p, lengths, self.tables(m.device)).unsqueeze(1).to(magnitude.device)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)
