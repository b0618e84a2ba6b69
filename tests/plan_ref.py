"""The length regulator and the planned free-running decoder on the CPU — TEST INFRASTRUCTURE, NOT PRODUCT.

regulate() is the integer definition of t2v_duration_plan (include/t2vae.h) in numpy:

    q_j = rint(float64(dur_j) * float64(rate_j) * 65536)  (ties to even),  C = cumsum(q) in int64,  E_j = (C_j + 32768) >> 16
    symbol j owns the frames E_{j-1} <= t < E_j;  n_plan = min(E_last, T_max);  behind n_plan the plan holds its last value

decode() is the loop of tests/window_ref.py around the unmodified oracle's decoder_init, prenet_forward and decoder_step, with
the window's centre taken from a plan instead of the previous weights: before frame t

    p = clamp(plan[b, min(t, n_plan[b] - 1)], 0, len_b - 1)
    st.mask = (pos < p - back) | (pos > p + ahead) | (pos >= len)

The gate is ignored, the frame count is fixed and dropout is off.  t2v_oracle.py and window_ref.py are untouched.

Inputs: the steered memory of tests/steer_ref.py (location_dense * 60 on the CPU decoder, + 0.4 u on both sides of every cut of
the kernels).  A plan is data and need not be contiguous, so the plans below jump from cut to cut: within 8 to 12 frames every
case puts its window on both sides of the cuts (16, 32, 64, 80, 128, 192, 256, 288, 384, 480, 512) its text contains.
"""
import functools

import numpy as np
import torch

import steer_ref as S
import window_ref as W

MAX_FRAMES_PER_SYMBOL = 2.0 ** 20


# ------------------------------------------------------------------------------------------------ the length regulator
def regulate(dur, n_ids, T_max, rate=None):
    """dur (B, S) float32, n_ids B counts, rate None, a number or (B, S) float32.  Returns (plan (B, T_max) int32, n_plan (B,)
    int32); a refused row (a negative or non-finite dur * rate, or one above 2^20) has n_plan -1 and a plan of zeros."""
    dur = np.asarray(dur, dtype=np.float32)
    B, n_sym = dur.shape
    r = np.ones_like(dur) if rate is None else np.broadcast_to(np.asarray(rate, dtype=np.float32), dur.shape)
    plan = np.zeros((B, T_max), dtype=np.int32)
    n_plan = np.zeros(B, dtype=np.int32)
    for b in range(B):
        L = int(min(max(int(n_ids[b]), 0), n_sym))
        x = dur[b, :L].astype(np.float64) * r[b, :L].astype(np.float64)
        if not np.all(np.isfinite(x)) or np.any(x < 0) or np.any(x > MAX_FRAMES_PER_SYMBOL):
            n_plan[b] = -1
            continue
        q = np.rint(x * 65536.0).astype(np.int64)
        E = (np.cumsum(q, dtype=np.int64) + 32768) >> 16
        n = int(min(int(E[-1]), T_max)) if L else 0
        n_plan[b] = n
        t = np.arange(n, dtype=np.int64)
        row = np.searchsorted(E, t, side='right').astype(np.int32)          # the first j with E_j > t
        plan[b, :n] = row
        plan[b, n:] = row[-1] if n else 0
    return plan, n_plan


# ------------------------------------------------------------------------------------------------ the planned decoder
def centres(plan, n_plan, lens, frames, t0=0):
    """(B, frames) int64: p of the frames t0 .. t0 + frames - 1"""
    plan = torch.as_tensor(plan, dtype=torch.long)
    B = plan.shape[0]
    t = torch.arange(t0, t0 + frames)[None, :].expand(B, frames)
    idx = torch.minimum(t, torch.as_tensor(n_plan, dtype=torch.long)[:, None] - 1)
    q = plan.gather(1, idx)
    return torch.minimum(q.clamp(min=0), torch.as_tensor(lens, dtype=torch.long)[:, None] - 1)


def decode(sd, memory, lens, window, plan, n_plan, frames):
    """`frames` free-running frames of the oracle's decoder under the plan and `window` = (back, ahead).
    Returns (mel (B, 80, frames), gate (B, frames), align (B, frames, T_in), p (B, frames))."""
    import t2v_oracle as O
    B, T_in, _ = memory.shape
    pos = torch.arange(T_in)[None, :]
    length = torch.as_tensor(lens, dtype=torch.long)[:, None]
    P = centres(plan, n_plan, lens, frames)
    st = O.decoder_init(sd, memory, None)
    x = memory.new_zeros(B, 80)
    mels, gates, aligns = [], [], []
    with torch.no_grad():
        for t in range(frames):
            p = P[:, t:t + 1]
            st.mask = (pos < p - window[0]) | (pos > p + window[1]) | (pos >= length)
            m, g, a = O.decoder_step(sd, st, O.prenet_forward(sd, x, None, 0.0))
            mels.append(m), gates.append(g.squeeze(1)), aligns.append(a)
            x = m
    return torch.stack(mels).permute(1, 2, 0).contiguous(), torch.stack(gates).t().contiguous(), \
        torch.stack(aligns).transpose(0, 1).contiguous(), P


# ------------------------------------------------------------------------------------------------ cases
_L84 = (84, 80, 71, 66, 50, 37, 20, 5)
_M84 = (0, 15, 16, 31, 32, 63, 64, 79)


def _rows(*rows):
    n = max(len(r) for r in rows)
    return tuple(tuple(r) + (r[-1],) * (n - len(r)) for r in rows)


# (T_in, lengths, (back, ahead), frames, plan rows, n_plan).  A plan value may lie beyond its item (clamped to len - 1), and
# n_plan may be shorter than the run (the last symbol is held).
CASES = (
    # smallest; ragged; item 1 (7 symbols) reaches its last symbol and is then sent beyond it
    (20, (20, 7), (1, 1), 8, _rows((0, 1, 3, 15, 16, 17, 19, 19), (0, 2, 4, 6, 6, 8, 12, 19)), (8, 8)),
    # a group of 8: launch-per-stage on both paths, per-item kernels; one-hot; every item walks the cuts its length holds
    (84, _L84, (0, 0), 8, tuple(tuple((v + i) % 84 for v in _M84) for i in range(8)), (8,) * 8),
    # persistent B = 3, 8 tiles; crosses 16 / 32 / 64 / 80; item 2's plan ends after 4 frames and is held
    (97, (97, 96, 17), (1, 3), 10, _rows((0, 14, 15, 30, 31, 62, 63, 78, 79, 96), (1, 15, 16, 31, 32, 63, 64, 79, 80, 95),
                                         (0, 5, 15, 16)), (10, 10, 4)),
    # the persistent kernel at the two corners of what its LDS holds
    (224, (224,), (1, 3), 10, _rows((0, 15, 16, 126, 127, 128, 190, 191, 192, 223)), (10,)),
    (128, (128, 97, 60, 9), (0, 0), 8, _rows((0, 15, 16, 63, 64, 79, 80, 127), (96, 80, 79, 64, 63, 32, 31, 0),
                                             (59, 60, 16, 15, 32, 31, 0, 58), (0, 8, 9, 3, 127, 4, 8, 0)), (8, 8, 8, 8)),
    # B = 4 at T_in = 224 does not fit the persistent kernel: the launch-per-stage loop on both paths
    (224, (224, 129, 60, 9), (1, 1), 8, _rows((127, 128, 191, 192, 222, 223, 0, 16), (0, 127, 128, 129, 64, 63, 16, 15),
                                              (0, 31, 32, 59, 60, 15, 16, 58), (8, 7, 0, 1, 9, 200, 4, 5)), (8, 8, 6, 8)),
    # first T_in past the persistent kernel, 16 tiles
    (225, (225,), (1, 3), 8, _rows((0, 127, 128, 191, 192, 223, 224, 300)), (8,)),
    # the chunked form; item 0 crosses 256, 288, 384, 480, 512; item 1 (290 symbols) 128, 192, 256, 288 and is sent beyond its end
    (555, (555, 290), (1, 3), 12, _rows((0, 254, 255, 287, 288, 383, 384, 479, 480, 511, 512, 554),
                                        (127, 128, 191, 192, 254, 255, 256, 286, 287, 288, 289, 400)), (12, 12)),
)
PERSIST_MAX_T = W.PERSIST_MAX_T


def case_id(case):
    return 'Tin%d-B%d-w%d_%d' % (case[0], len(case[1]), case[2][0], case[2][1])


persistent_fits = W.persistent_fits
state_dict = W.state_dict


@functools.lru_cache(maxsize=None)
def inputs(T_in, lens):
    """(CPU decoder with location_dense * 60, steered memory (B, T_in, 512) fp32) of steer_ref"""
    dec, memory = S.inputs((len(lens), T_in, 1, tuple(lens)))[:2]
    return dec, memory


def shifted(case, how):
    """the plan rows of a case shifted by one frame (frame t takes what frame t - 1 had; frame 0 keeps its own) or by one symbol
    (+ 1, or - 1 where + 1 would leave the item, so that the clamp cannot hide the shift)"""
    T_in, lens, win, frames, plan, n_plan = case
    if how == 'frame':
        return tuple((r[0],) + r[:-1] for r in plan)
    assert how == 'symbol', how
    return tuple(tuple((min(v, n - 1) + 1) if min(v, n - 1) + 1 <= n - 1 else n - 2 for v in r) if n > 1 else r
                 for r, n in zip(plan, lens))


@functools.lru_cache(maxsize=None)
def reference(case, dtype, how=None, window=None):
    """decode() of a case in `dtype`; how: None, 'frame' or 'symbol' (shifted()); window: None (the case's own) or another
    (back, ahead).  Cached: never modify."""
    T_in, lens, win, frames, plan, n_plan = case
    dec, memory = inputs(T_in, lens)
    rows = plan if how is None else shifted(case, how)
    return decode(state_dict(dec, dtype), memory.to(dtype), lens, window or win, rows, n_plan, frames)


@functools.lru_cache(maxsize=None)
def floors(case):
    """{quantity: planned fp32 reference minus planned fp64 reference}, measured as steer_ref.compare measures"""
    return {k: v[0] for k, v in S.compare(reference(case, torch.float32)[:3], reference(case, torch.float64)[:3]).items()}


def outside(p, lens, window, T_in):
    """(B, frames, T_in) bool: the positions outside [p - back, p + ahead] ∩ [0, len)"""
    pos = torch.arange(T_in)[None, None, :]
    c = p[:, :, None]
    return (pos < c - window[0]) | (pos > c + window[1]) | (pos >= torch.as_tensor(lens)[:, None, None])
