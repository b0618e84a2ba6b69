"""The host replica of the device's dropout mask function (tests/drop_ref.py) on its own: no GPU.  That it IS the device's
function is checked bit for bit on the GPU (tests/test_dropout_parity_gpu.py)."""
import warnings

import numpy as np
import pytest

import drop_ref as R

SEED = (1234 * 1000003 + 1) & 0x7FFFFFFFFFFFFFFF


def _splitmix_int(seed, stream, t, idx):
    """the same function on Python's unbounded integers, reduced mod 2^64 by hand"""
    m = (1 << 64) - 1
    x = (seed ^ (stream << 58) ^ (t << 32) ^ idx) & m
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    x ^= x >> 31
    return x >> 32


def test_replica_is_deterministic_and_wraps_without_warnings():
    t = np.arange(30)[:, None]
    idx = np.arange(6144)[None, :]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        # seeds with the top bits set: every add and multiply below overflows 64 bits
        for seed in (SEED, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0):
            a = R.rng_u32(seed, 4, t, idx)
            b = R.rng_u32(seed, 4, t, idx)
            assert a.dtype == np.uint32 and a.shape == (30, 6144)
            assert np.array_equal(a, b)
            k = R.keep_mask(seed, 4, t, idx, 0.1)
            assert k.dtype == bool and np.array_equal(k, R.keep_mask(seed, 4, t, idx, 0.1))
            s = R.drop_scale(seed, 4, t, idx, 0.1)
            assert s.dtype == np.float32
            assert np.array_equal(s != 0, k) and np.all(s[k] == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))
        # scalars go the same way
        assert R.rng_u32(0xFFFFFFFFFFFFFFFF, 63, 0xFFFFFFFF, 0xFFFFFFFF).shape == (1,)


def test_replica_matches_unbounded_integer_arithmetic():
    """64-bit wrap-around: numpy's uint64 result equals the function evaluated on Python integers mod 2^64"""
    rs = np.random.RandomState(0)
    for _ in range(200):
        seed = int(rs.randint(0, 2 ** 31)) << 33 | int(rs.randint(0, 2 ** 31)) << 2 | int(rs.randint(0, 4))
        stream, t, idx = int(rs.randint(0, 64)), int(rs.randint(0, 2 ** 31)) * 2 + 1, int(rs.randint(0, 2 ** 31)) * 2
        assert int(R.rng_u32(seed, stream, t, idx)[0]) == _splitmix_int(seed, stream, t, idx)
    assert int(R.rng_u32(0, 0, 0, 0)[0]) == _splitmix_int(0, 0, 0, 0)


def test_replica_changes_with_stream_t_and_idx_alone():
    idx = np.arange(4096)
    base = R.rng_u32(SEED, 1, 3, idx)
    for other in (R.rng_u32(SEED, 2, 3, idx), R.rng_u32(SEED, 1, 4, idx), R.rng_u32(SEED, 1, 3, idx + 1),
                  R.rng_u32(SEED + 1, 1, 3, idx)):
        # 32-bit draws: two equal ones among 4096 pairs have probability 1e-6
        assert (other != base).mean() > 0.999
    k = R.keep_mask(SEED, 1, 3, idx, 0.5)
    for other in (R.keep_mask(SEED, 2, 3, idx, 0.5), R.keep_mask(SEED, 1, 4, idx, 0.5), R.keep_mask(SEED, 1, 3, idx + 1, 0.5)):
        # independent fair coins disagree on half of 4096 positions, +- 5 sigma = 160
        assert abs(int((other != k).sum()) - 2048) < 160


def test_p_zero_keeps_everything():
    t = np.arange(7)[:, None]
    idx = np.arange(1000)[None, :]
    assert R.keep_mask(SEED, 2, t, idx, 0.0).all()
    assert np.all(R.drop_scale(SEED, 2, t, idx, 0.0) == np.float32(1.0))
    assert R.conv_keep(SEED, 9, 5, 2, 3, 11, 0.0).all()


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_share_is_binomial(p):
    n = 1 << 18
    t = np.arange(64)[:, None]
    idx = np.arange(n // 64)[None, :]
    share = R.keep_mask(SEED, 3, t, idx, p).mean()
    sigma = (p * (1.0 - p) / n) ** 0.5
    assert abs(share - (1.0 - p)) < 5.0 * sigma, (share, sigma)


def test_helpers_index_like_the_kernels():
    """decoder_state_keeps: idx = b_local * 1024 + unit under the chunk's seed; conv_keep: idx = flat offset of (B, C, T)"""
    import t2v_hip
    B, T = 20, 3
    keeps = R.decoder_state_keeps(SEED, 0, B, T, 0.5, 0.25)
    assert len(keeps) == T and sorted(keeps[0]) == ['att_c', 'att_h', 'dec_c', 'dec_h']
    unit = np.arange(1024)
    for name, stream, p in (('att_h', 1, 0.5), ('att_c', 2, 0.5), ('dec_h', 3, 0.25), ('dec_c', 4, 0.25)):
        for t in range(T):
            m = keeps[t][name].numpy()
            assert m.shape == (B, 1024) and m.dtype == bool
            for b in (0, 1, 15, 16, 19):
                c0 = b // 16 * 16
                assert np.array_equal(m[b], R.keep_mask(t2v_hip._chunk_seed(SEED, c0), stream, t, (b - c0) * 1024 + unit, p)), (name, t, b)
    # a window of the batch is the same rows
    part = R.decoder_state_keeps(SEED, 14, 4, T, 0.5, 0.25)
    assert all(np.array_equal(part[t][k].numpy(), keeps[t][k].numpy()[14:18]) for t in range(T) for k in keeps[t])
    ck = R.conv_keep(77, 3, 11, 2, 5, 7, 0.5).numpy()
    assert ck.shape == (2, 5, 7)
    assert ck[1, 3, 4] == R.keep_mask(77, 3, 11, (1 * 5 + 3) * 7 + 4, 0.5)[0]
    assert np.array_equal(ck.ravel(), R.keep_mask(77, 3, 11, np.arange(70), 0.5))
