"""csrc/loudness.hip on the device against the fp64 definitions of loudness_ref.py.  The rows are the smallest at which the
kernels can go wrong: one sample, the lengths around one and two 400 ms blocks, around one lane's chunk and one workgroup
tile (the filter state is scanned across both), and the 6 s burst signal on which the relative gate matters; at 16 and 48 kHz
(hop sums from whole chunks) and at 22.05 kHz (a hop boundary inside a chunk).

Tolerances: integrated and ungated loudness within 0.01 LU of the reference (a tenth of the 0.1 LU that EBU Tech 3341 allows a
conforming meter), block and frame levels within 0.05 dB wherever the reference level is above -70 LUFS on rows without DC, the
row with a DC offset of 0.5 held to its integrated loudness only, and the gated block count exact, the reference first showing
that no block lies within 0.5 dB of either gate.  The kernel keeps the filter state in fp64 (samples and sums of squares are
fp32): with an fp32 state the 0.05 dB bound is missed on this burst signal at 48 kHz, where the frames right behind the
0.5-amplitude burst, at -65 LUFS, came out 0.09 and 0.18 dB off on the device, and sequential fp32 loops on the CPU (direct
form I, transposed form II) 0.27 to 0.32 dB: the high pass's double pole lies 0.005 from z = 1 and amplifies the rounding of
its state about 1 400 times."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R

pytestmark = pytest.mark.gpu

RATES = (16000, 48000, 22050)
LU_TOL = 0.01
DB_TOL = 0.05
GATE_MARGIN = 0.5


def _bits(t):
    return t.cpu().numpy().tobytes()


def _cases(sr):
    """[(name, samples fp32, has DC)]"""
    import t2v_hip
    hop = sr // 10
    blk = 4 * hop
    rng = np.random.RandomState(sr)
    lengths = [('one sample', 1), ('block - 1', blk - 1), ('block', blk), ('block + hop - 1', blk + hop - 1),
               ('block + hop', blk + hop), ('one chunk', t2v_hip.LOUDNESS_CHUNK), ('one chunk + 1', t2v_hip.LOUDNESS_CHUNK + 1),
               ('one tile + 1', t2v_hip.LOUDNESS_TILE + 1)]
    cases = [(name, (0.1 * rng.randn(n)).astype(np.float32), False) for name, n in lengths]
    cases.append(('bursts', R.gating_signal(sr).astype(np.float32), False))
    cases.append(('dc', (0.5 + 0.1 * rng.randn(blk + 3 * hop + 17)).astype(np.float32), True))
    return cases


def _batch(cases, extra=129):
    lengths = [len(x) for _, x, _ in cases]
    y = np.full((len(cases), max(lengths) + extra), np.nan, dtype=np.float32)
    for b, (_, x, _) in enumerate(cases):
        y[b, :len(x)] = x
    return y, lengths


@pytest.fixture(scope='module')
def measured():
    """per rate: (cases, reference per row, (Loudness, block powers) of the NaN-padded batch), each computed once"""
    import t2v_hip
    out = {}
    for sr in RATES:
        cases = _cases(sr)
        ref = [R.measure(x.astype(np.float64), sr) for _, x, _ in cases]
        y, lengths = _batch(cases)
        got = t2v_hip.loudness(torch.from_numpy(y).cuda(), lengths, sr, return_blocks=True)
        out[sr] = (cases, ref, got, lengths)
    return out


def _close_lu(got, want, tol):
    return got == want if math.isinf(want) else abs(got - want) <= tol


@pytest.mark.parametrize('sr', RATES)
def test_batch_against_the_fp64_reference(measured, sr):
    cases, ref, (got, blocks), lengths = measured[sr]
    frames = got.frame_ms.cpu().numpy()
    blocks = blocks.cpu().numpy()
    assert frames.shape == (len(cases), max(lengths) // 256 + 1)
    assert not np.isnan(frames).any() and not np.isnan(blocks).any()                 # a NaN of the padding never shows
    worst = dict(integrated=0.0, ungated=0.0, block=0.0, frame=0.0)
    for b, ((name, x, dc), want) in enumerate(zip(cases, ref)):
        # a condition on the inputs: no block is a toss-up at either gate
        assert want['margin_abs'] > GATE_MARGIN and want['margin_rel'] > GATE_MARGIN, (sr, name, want['margin_abs'], want['margin_rel'])
        assert got.n_blocks[b] == want['n_blocks'], (sr, name)
        assert got.gated_blocks[b] == want['gated_blocks'], (sr, name, got.gated_blocks[b], want['gated_blocks'])
        for key in ('integrated', 'ungated'):
            g, w = getattr(got, key)[b], want[key]
            if not math.isinf(w):
                worst[key] = max(worst[key], abs(g - w))
            print("%d Hz %-16s %-10s %.6f (reference %.6f)" % (sr, name, key, g, w))
        assert _close_lu(got.integrated[b], want['integrated'], LU_TOL), (sr, name, got.integrated[b], want['integrated'])
        nb, nf = want['n_blocks'], len(x) // 256 + 1
        assert np.all(blocks[b, nb:] == 0) and not np.signbit(blocks[b, nb:]).any(), (sr, name)
        assert np.all(frames[b, nf:] == 0) and not np.signbit(frames[b, nf:]).any(), (sr, name)
        if want['gated_blocks']:
            assert got.gated_sum[b] == pytest.approx(want['gated_sum'], rel=10.0 ** (LU_TOL / 10.0) - 1.0)
        else:
            assert got.gated_sum[b] == 0.0
        if dc:
            continue
        assert _close_lu(got.ungated[b], want['ungated'], LU_TOL), (sr, name, got.ungated[b], want['ungated'])
        assert _close_lu(got.momentary_max[b], want['momentary_max'], DB_TOL), (sr, name)
        for key, mine, theirs in (('block', blocks[b, :nb], want['block_powers']), ('frame', frames[b, :nf], want['frame_ms'])):
            level = R.energy_db(theirs)
            loud = level > -70.0
            if loud.any():
                err = np.abs(R.energy_db(mine.astype(np.float64))[loud] - level[loud])
                worst[key] = max(worst[key], float(err.max()))
                assert err.max() <= DB_TOL, (sr, name, key, float(err.max()))
    print("%d Hz worst errors: integrated %.2e LU, ungated %.2e LU, block level %.2e dB, frame level %.2e dB"
          % (sr, worst['integrated'], worst['ungated'], worst['block'], worst['frame']))
    bursts = [b for b, c in enumerate(cases) if c[0] == 'bursts'][0]
    assert got.integrated[bursts] - got.ungated[bursts] > 1.0                       # the relative gate is at work
    assert 0 < got.gated_blocks[bursts] < got.n_blocks[bursts]


def test_rows_without_a_loudness():
    import t2v_hip
    rng = np.random.RandomState(7)
    y = np.full((3, 16500), np.nan, dtype=np.float32)
    y[0, :6399] = 0.1 * rng.randn(6399)                                              # shorter than one block
    y[1, :16000] = 0.0                                                               # digital silence
    y[2, :16000] = 1e-5 * rng.randn(16000)                                           # about -100 LUFS: under the absolute gate
    got = t2v_hip.loudness(torch.from_numpy(y).cuda(), [6399, 16000, 16000], 16000)
    assert got.integrated == [float('-inf')] * 3 and got.gated_blocks == [0, 0, 0] and got.gated_sum == [0.0, 0.0, 0.0]
    assert got.n_blocks == [0, 7, 7]
    assert got.momentary_max[0] == float('-inf') and got.ungated[1] == float('-inf') and got.momentary_max[1] == float('-inf')
    assert math.isfinite(got.ungated[0]) and -105.0 < got.ungated[2] < -95.0
    assert float(got.frame_ms[1].abs().max()) == 0.0


@pytest.mark.parametrize('sr', RATES)
def test_a_row_alone_in_the_batch_and_at_another_stride(measured, sr):
    import t2v_hip
    cases, ref, (got, blocks), lengths = measured[sr]
    for b, (name, x, _) in enumerate(cases):
        n, nb, nf = len(x), ref[b]['n_blocks'], len(x) // 256 + 1
        alone, alone_blocks = t2v_hip.loudness(torch.from_numpy(x[None].copy()).cuda(), [n], sr, return_blocks=True)
        wide = np.full((2, n + 333), np.nan, dtype=np.float32)
        wide[0, :5] = 0.25
        wide[1, :n] = x
        other, other_blocks = t2v_hip.loudness(torch.from_numpy(wide).cuda(), [5, n], sr, return_blocks=True)
        for key in ('integrated', 'ungated', 'momentary_max', 'gated_sum', 'gated_blocks', 'n_blocks'):
            a, c, d = getattr(alone, key)[0], getattr(other, key)[1], getattr(got, key)[b]
            assert np.float64(a).tobytes() == np.float64(c).tobytes() == np.float64(d).tobytes(), (sr, name, key, a, c, d)
        want = _bits(got.frame_ms[b, :nf])
        assert _bits(alone.frame_ms[0, :nf]) == want and _bits(other.frame_ms[1, :nf]) == want, (sr, name)
        assert tuple(alone.frame_ms.shape) == (1, nf)
        if nb:
            want = _bits(blocks[b, :nb])
            assert _bits(alone_blocks[0, :nb]) == want and _bits(other_blocks[1, :nb]) == want, (sr, name)


def test_scale_rows_equals_numpy():
    import t2v_hip
    rng = np.random.RandomState(9)
    y = rng.uniform(-1, 1, (4, 1000)).astype(np.float32)
    n = [1000, 1, 257, 640]
    for b, k in enumerate(n):
        y[b, k:] = np.nan
    g = np.array([0.5, 3.0, 10.0 ** (-7.3 / 20.0), 1.0], dtype=np.float32)
    t = torch.from_numpy(y.copy()).cuda()
    out = t2v_hip.scale_rows(t, n, g.tolist())
    assert out is t
    got = t.cpu().numpy()
    for b, k in enumerate(n):
        assert got[b, :k].tobytes() == (y[b, :k] * g[b]).tobytes(), b
        assert got[b, k:].tobytes() == y[b, k:].tobytes(), b                         # columns past the length are untouched
    t2 = torch.from_numpy(y.copy()).cuda()
    t2v_hip.scale_rows(t2, torch.tensor(n).cuda(), torch.from_numpy(g).cuda())
    assert _bits(t2) == got.tobytes()


def test_bad_arguments_raise_and_the_library_stays_usable():
    import t2v_hip
    x = torch.zeros(2, 7000, device='cuda')
    good = lambda: t2v_hip.loudness(x, [7000, 300], 16000)
    for call, exc in ((lambda: t2v_hip.loudness(x, [7000, 300], 11025), ValueError),
                      (lambda: t2v_hip.loudness(x, [7000, 300], 96000), ValueError),
                      (lambda: t2v_hip.loudness(x, [7000, 0]), ValueError),
                      (lambda: t2v_hip.loudness(x, [7001, 300]), ValueError),
                      (lambda: t2v_hip.loudness(x, [7000]), ValueError),
                      (lambda: t2v_hip.loudness(x, [7000.0, 300.0]), ValueError),
                      (lambda: t2v_hip.loudness(x, [True, True]), ValueError),
                      (lambda: t2v_hip.loudness(x.cpu(), [7000, 300]), t2v_hip.T2VHipError),
                      (lambda: t2v_hip.loudness(x.double(), [7000, 300]), ValueError),
                      (lambda: t2v_hip.loudness(x[0], [7000]), ValueError),
                      (lambda: t2v_hip.scale_rows(x.cpu(), [7000, 300], [1.0, 1.0]), t2v_hip.T2VHipError),
                      (lambda: t2v_hip.scale_rows(x, [7000, 300], [1.0]), ValueError),
                      (lambda: t2v_hip.scale_rows(x, [7000, 7001], [1.0, 1.0]), ValueError),
                      (lambda: t2v_hip.scale_rows(x[:, ::2], [3500, 300], [1.0, 1.0]), ValueError)):
        with pytest.raises(exc):
            call()
        r = good()
        assert r.n_blocks == [1, 0] and r.integrated == [float('-inf')] * 2
    with pytest.raises(ValueError, match='11025'):
        t2v_hip.loudness(x, [7000, 300], 11025)
    # the C ABI's own refusals: a short frame stride, a hop outside 8 .. 48 kHz
    lib = t2v_hip.load_library()
    n = torch.tensor([7000, 300], dtype=torch.int32, device='cuda')
    table = torch.from_numpy(t2v_hip.loudness_table(16000).copy()).cuda()
    ms, blocks = torch.zeros(2, 28, device='cuda'), torch.zeros(2, 1, device='cuda')
    rows = torch.zeros(2, 8, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(lib.t2v_loudness_scratch_bytes(2, 7000, 1600), dtype=torch.uint8, device='cuda')
    args = lambda hop, stride: (t2v_hip._p(x), t2v_hip._p(n), 7000, 2, t2v_hip._p(table), hop, t2v_hip._p(ms), stride,
                                t2v_hip._p(blocks), 1, t2v_hip._p(rows), t2v_hip._p(scratch), t2v_hip._stream())
    assert lib.t2v_loudness(*args(1600, 27)) == -2                                   # T2V_ERR_ARG
    assert lib.t2v_loudness(*args(700, 28)) == -1                                    # T2V_ERR_DIMS
    assert lib.t2v_loudness(*args(1600, 28)) == 0
    torch.cuda.synchronize()
    assert rows.cpu()[:, 4].tolist() == [1, 0]
