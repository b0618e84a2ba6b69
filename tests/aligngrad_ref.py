"""The steered decoder cases of tests/steer_ref.py with a loss that reads the alignments — TEST INFRASTRUCTURE, NOT PRODUCT.

oracle_with_align(case, dtype, scale) is steer_ref.oracle's body with the loss sum(mel * wm) + sum(gate * wg) + sum(align * wa),
wa = scale * randn(B, T, T_in) from a fixed seed: non-zero everywhere, also at positions j >= N_b of an item, where alpha is
exactly 0 and a gradient that leaked past the mask would show.  SCALE holds the scale of every case the device tests use; the
condition they have to meet (the alignment term moves grad and d_memory by more than the parity bound) is checked on the oracle
alone in tests/test_aligngrad_ref.py."""
import functools

import torch

import steer_ref as S

# the chunked case: 18 items run as two chunks of 16 and 2
CHUNKED = (18, 20, 3, tuple(range(20, 2, -1)))
# fp32 cases of tests/test_align_grad_gpu.py and what each reaches
CASES = (S.CASES[0],        # (2, 20, 5)    16-position slices
         S.CASES[1],        # (6, 84, 6)    32-position slices
         S.CASES[2],        # (3, 97, 5)    96-position slices, short form
         S.CASES[3],        # (16, 40, 3)   fp32: launch per step only
         S.CASES[5],        # (2, 225, 4)   96-position slices on eight waves
         S.CASES[7],        # (2, 570, 3)   launch-per-step forward with one-launch reverse
         CHUNKED)
assert [c[:3] for c in CASES] == [(2, 20, 5), (6, 84, 6), (3, 97, 5), (16, 40, 3), (2, 225, 4), (2, 570, 3), (18, 20, 3)]

WA_SEED = 20250


def wa(case, scale, dtype=torch.float32):
    """the weights of the alignment term, (B, T, T_in)"""
    B, T_in, T = case[:3]
    g = torch.Generator().manual_seed(WA_SEED)
    return (scale * torch.randn(B, T, T_in, generator=g)).to(dtype)


# scale of wa per case: chosen so that the alignment term is seen (tests/test_aligngrad_ref.py), committed
SCALE = {c: 1.0 for c in CASES}


@functools.lru_cache(maxsize=4)
def oracle_with_align(case, dtype, scale):
    """(mel, gate, align, {parameter: gradient}, d memory) as steer_ref.oracle, the loss extended by sum(align * wa).
    Cached; never modify the result."""
    import t2v_oracle as O
    dec, memory, mels, lengths, wm, wg = S.inputs(case)
    sd = {'decoder.' + k: v.detach().to(dtype).requires_grad_(True) for k, v in dec.state_dict().items()}
    mem = memory.to(dtype).requires_grad_(True)
    mel, gate, align = O.decoder_forward(sd, mem, mels.to(dtype), lengths, p_att=0.0, p_dec=0.0)
    ((mel * wm.to(dtype)).sum() + (gate * wg.to(dtype)).sum() + (align * wa(case, scale, dtype)).sum()).backward()
    grads = {k[len('decoder.'):]: v.grad for k, v in sd.items()}
    return mel.detach(), gate.detach(), align.detach(), grads, mem.grad


@functools.lru_cache(maxsize=None)
def floor_with_align(case, scale=None):
    """{quantity: fp32 oracle minus fp64 oracle} with the alignment term, measured as steer_ref.compare measures"""
    scale = SCALE[case] if scale is None else scale
    return {k: v[0] for k, v in S.compare(oracle_with_align(case, torch.float32, scale),
                                          oracle_with_align(case, torch.float64, scale)).items()}
