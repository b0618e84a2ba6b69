"""The windowed free-running decoder on the CPU — TEST INFRASTRUCTURE, NOT PRODUCT.

oracle/t2v_oracle.py masks a frame's energies with st.mask inside decoder_step, so the attention window of
Decoder.attention_window is a loop of its own around decoder_init, prenet_forward and decoder_step that sets, before
every step,

    p = st.alpha.argmax(1, keepdim=True)                    (the first index on a tie: 0 at frame 0, where alpha is all zero)
    st.mask = (pos < p - back) | (pos > p + ahead) | (pos >= len)

The gate is ignored, the frame count is fixed and dropout is off.  t2v_oracle.py itself is untouched.

Inputs: the steered memory of tests/steer_ref.py (location_dense * 60 on the CPU decoder), then a ramp: item i of length n gets
0.8 u on its memory rows 0, ahead, 2 ahead, ... and on row n - 1, u = pinv(W_mem) sign(v) in fp64 as in steer_ref.steer.  The
energy then grows by about 0.8 |v|_1 at those rows, so that a window of `ahead` positions in front of p always holds the next
rung: the window marches across the tile and chunk cuts of the kernels, while the unconstrained decoder puts most of its mass
on rungs far outside it.
"""
import functools

import torch

import steer_ref as S

RAMP_GAIN = 0.8

# (T_in, lengths, (back, ahead), frames)
_L84 = (84, 80, 71, 66, 50, 37, 20, 5)
CASES = ((20, (20, 7), (1, 3), 6),                       # smallest; ragged
         (84, _L84, (1, 3), 8),                          # a group of 8: launch-per-stage on both paths, per-item kernels
         (84, _L84, (0, 1), 8),                          # strictly monotonic: stay or advance by one
         (97, (97, 96, 17), (2, 20), 6),                 # persistent B = 3, 8 tiles; crosses 16 / 32 / 64 / 80; item 2 ends up pinned at symbol 16
         (224, (224, 129, 60, 9), (1, 60), 5),           # T_in at the persistent kernel's limit, B = 4; crosses 128
         (225, (225,), (1, 60), 5),                      # first T_in past the persistent kernel, 16 tiles
         (555, (555, 290), (3, 130), 6),                 # the chunked form; crosses 128, 256, 288, 384, 480, 512
         # the persistent kernel at the two corners of what its LDS holds (include/t2vae.h: T_in <= 224 at B = 1, 128 at B = 4)
         (224, (224,), (1, 60), 5),                      # B = 1, shared seed; crosses 128 and 192 on chip
         (128, (128, 97, 60, 9), (1, 40), 5))            # B = 4, per item
# what the persistent decode launch takes (include/t2vae.h, t2v_decoder_persist_supported): T_in at most this at B = 1 .. 4
PERSIST_MAX_T = (224, 192, 160, 128)


def case_id(case):
    return 'Tin%d-B%d-w%d_%d' % (case[0], len(case[1]), case[2][0], case[2][1])


def persistent_fits(B, T_in):
    return B <= len(PERSIST_MAX_T) and T_in <= PERSIST_MAX_T[B - 1]


def rungs(n, ahead):
    """the memory rows of an item of length n that the ramp raises"""
    return sorted(set(range(0, n, max(1, ahead))) | {n - 1})


@functools.lru_cache(maxsize=None)
def inputs(T_in, lens, ahead):
    """(CPU decoder with location_dense * 60, steered and ramped memory (B, T_in, 512) fp32)"""
    dec, memory = S.inputs((len(lens), T_in, 1, tuple(lens)))[:2]
    al = dec.attention_layer
    with torch.no_grad():
        w_mem = al.memory_layer.linear_layer.weight.detach().double()
        v = al.v.linear_layer.weight.detach().double()[0]
        u = torch.linalg.pinv(w_mem) @ torch.sign(v)
        mem = memory.detach().double().clone()
        for i, n in enumerate(lens):
            mem[i, rungs(int(n), ahead)] += RAMP_GAIN * u
    return dec, mem.to(memory.dtype)


def decode(sd, memory, lens, window, frames):
    """`frames` free-running frames of the oracle's decoder under `window` ((back, ahead), or None: the length mask alone).
    Returns (mel (B, 80, frames), gate (B, frames), align (B, frames, T_in), p (B, frames): the window centre of every frame)."""
    import t2v_oracle as O
    B, T_in, _ = memory.shape
    pos = torch.arange(T_in)[None, :]
    length = torch.as_tensor(lens, dtype=torch.long)[:, None]
    st = O.decoder_init(sd, memory, None)
    x = memory.new_zeros(B, 80)
    mels, gates, aligns, centres = [], [], [], []
    with torch.no_grad():
        for _ in range(frames):
            p = st.alpha.argmax(1, keepdim=True)
            st.mask = pos >= length
            if window is not None:
                st.mask = (pos < p - window[0]) | (pos > p + window[1]) | st.mask
            m, g, a = O.decoder_step(sd, st, O.prenet_forward(sd, x, None, 0.0))
            mels.append(m), gates.append(g.squeeze(1)), aligns.append(a), centres.append(p.squeeze(1))
            x = m
    return torch.stack(mels).permute(1, 2, 0).contiguous(), torch.stack(gates).t().contiguous(), \
        torch.stack(aligns).transpose(0, 1).contiguous(), torch.stack(centres).t().contiguous()


def state_dict(dec, dtype):
    return {'decoder.' + k: v.detach().to(dtype) for k, v in dec.state_dict().items()}


@functools.lru_cache(maxsize=None)
def reference(case, dtype, window='case'):
    """decode() of a case in `dtype`; window: 'case' (the case's own), None, or another (back, ahead).  Cached: never modify."""
    T_in, lens, win, frames = case
    dec, memory = inputs(T_in, lens, win[1])
    return decode(state_dict(dec, dtype), memory.to(dtype), lens, win if window == 'case' else window, frames)


@functools.lru_cache(maxsize=None)
def floors(case):
    """{quantity: windowed fp32 reference minus windowed fp64 reference}, measured as steer_ref.compare measures"""
    return {k: v[0] for k, v in S.compare(reference(case, torch.float32)[:3], reference(case, torch.float64)[:3]).items()}


def top_two_gap(align, lens):
    """smallest difference between the largest and the second largest weight over the frames of every item (positions < len);
    an item of length 1 has no second weight and is left out"""
    gap = float('inf')
    for b, n in enumerate(lens):
        if n < 2:
            continue
        top = align[b, :, :n].double().topk(2, dim=1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    return gap


def outside_mass(align, p, lens, window):
    """(B, frames): the share of each frame's weights outside [p - back, p + ahead] ∩ [0, len), p given per frame"""
    T_in = align.shape[2]
    pos = torch.arange(T_in)[None, None, :]
    c = p[:, :, None]
    out = (pos < c - window[0]) | (pos > c + window[1]) | (pos >= torch.as_tensor(lens)[:, None, None])
    return (align.double() * out).sum(2)
