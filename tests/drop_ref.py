"""Host replica of the device's dropout keep-masks — TEST INFRASTRUCTURE, NOT PRODUCT.

A numpy uint64 restatement of t2v_rng_u32 / t2v_drop_scale (csrc/t2v_common.h): the masks are a pure function of
(seed, stream, t, idx), so the host can know every mask a kernel draws and hand it to the oracle
(oracle/t2v_oracle.py: _apply_keep, decoder_forward(drop={'lstm': ...})) — dropout-on runs then compare like dropout-off ones.

    x  = seed ^ (stream << 58) ^ (t << 32) ^ idx              (all 64-bit)
    x += 0x9E3779B97F4A7C15;  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^= x >> 31
    u  = float32(hi32(x) >> 8) * 2^-24                         (24 bits: exact in fp32)
    keep iff u >= float32(p);   factor = keep ? 1 / (1 - p) : 0;   p <= 0: everything is kept

The index arithmetic of the two helpers is read from the kernels:
  decoder LSTM state (decoder_fwd.hip, decoder_train_persist.hip, decoder_bwd.hip, decoder_train_bwd_persist.hip):
      idx = b_local * 1024 + unit, b_local counted inside the chunk of <= 16 items, the chunk's seed = t2v_hip._chunk_seed(seed, b0);
      streams T2V_RNG_ATT_H .. T2V_RNG_DEC_C = 1 .. 4 (t2v_kernels.h); step t of a cell draws its h and c masks at t; the c mask
      of step t multiplies the cell state that step t + 1 reads.
  ConvBNAct1d (bn_act.hip): idx = the flat offset ((b * C + c) * T + t) of the (B, C, T) output, t = rng_t of the launch.
"""
import numpy as np
import torch

RNG_ATT_H, RNG_ATT_C, RNG_DEC_H, RNG_DEC_C = 1, 2, 3, 4          # t2v_kernels.h
H = 1024                                                          # T2V_H: units of either decoder LSTM cell
_M64 = (1 << 64) - 1


def rng_u32(seed, stream, t, idx):
    """t2v_rng_u32, broadcast over t and idx (arrays or ints; both are uint32 on the device).  Returns uint32."""
    t = np.atleast_1d(np.asarray(t)).astype(np.uint32).astype(np.uint64)
    idx = np.atleast_1d(np.asarray(idx)).astype(np.uint32).astype(np.uint64)
    head = np.uint64((int(seed) & _M64) ^ (((int(stream) & 0xFFFFFFFF) << 58) & _M64))
    with np.errstate(over='ignore'):          # unsigned 64-bit wrap-around is the arithmetic
        x = head ^ (t << np.uint64(32)) ^ idx
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.uint32)


def keep_mask(seed, stream, t, idx, p):
    """True where t2v_drop_scale(seed, stream, t, idx, p) != 0.  numpy bool, the broadcast shape of t and idx."""
    r = rng_u32(seed, stream, t, idx)
    if np.float32(p) <= np.float32(0.0):
        return np.ones(r.shape, dtype=bool)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def drop_scale(seed, stream, t, idx, p):
    """t2v_drop_scale: the fp32 factor, 0 or 1 / (1 - p)."""
    k = keep_mask(seed, stream, t, idx, p)
    if np.float32(p) <= np.float32(0.0):
        return k.astype(np.float32)
    return np.where(k, np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)


def decoder_state_keeps(seed, b0, B, T, p_att, p_dec):
    """Keep-masks of the decoder's LSTM state dropout for the items b0 .. b0 + B - 1 of a batch and the steps 0 .. T - 1:
    a list of T dicts {'att_h', 'att_c', 'dec_h', 'dec_c'} of torch bool (B, 1024), what O.decoder_forward(drop={'lstm': ...})
    takes.  `seed` is the seed of the whole call ((dropout_seed * 1000003 + call) & (2^63 - 1), model.py Decoder.forward)."""
    import t2v_hip
    chunk = t2v_hip.MAX_DEC_B
    unit = np.arange(H, dtype=np.uint64)[None, :]
    steps = np.arange(T, dtype=np.uint64)[:, None, None]
    out = {}
    for name, stream, p in (('att_h', RNG_ATT_H, p_att), ('att_c', RNG_ATT_C, p_att),
                            ('dec_h', RNG_DEC_H, p_dec), ('dec_c', RNG_DEC_C, p_dec)):
        rows = []
        for b in range(b0, b0 + B):
            c0 = b // chunk * chunk
            idx = np.uint64(b - c0) * np.uint64(H) + unit                                      # (1, 1024)
            rows.append(keep_mask(t2v_hip._chunk_seed(seed, c0), stream, steps, idx[None], p))   # (T, 1, 1024)
        out[name] = torch.from_numpy(np.concatenate(rows, 1))                                   # (T, B, 1024)
    return [{k: v[t] for k, v in out.items()} for t in range(T)]


def conv_keep(seed, stream, rng_t, B, C, T, p):
    """Keep-mask of one ConvBNAct1d launch: torch bool (B, C, T)."""
    idx = np.arange(B * C * T, dtype=np.uint64)
    return torch.from_numpy(keep_mask(seed, stream, rng_t, idx, p).reshape(B, C, T))
