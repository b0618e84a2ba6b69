"""t2v_hip.mel_dtw (csrc/dtw.hip) against an fp64 numpy DTW of the same recurrence: values, determinism, properties, errors
and the wrapper's group split.

Tolerance (derived, not measured): a path sum is at most Tx + Ty fp32 additions of non-negative terms, each local cost an
80-term sum of squares and a square root, so |dist - ref| <= ref * (Tx + Ty + 128) * 2^-23, twice the first-order bound."""
import pytest
import torch

from test_evaluate import dtw_ref

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (1, 7), (37, 5), (63, 64), (64, 65), (257, 1025), (600, 913), (1000, 1000), (2048, 2048)]


def _tol(ref, tx, ty):
    return ref * (tx + ty + 128) * 2.0 ** -23


def _mels(lengths, stride, seed):
    """(B, 80, stride) random log-mels, NaN past each length"""
    g = torch.Generator().manual_seed(seed)
    m = torch.full((len(lengths), 80, stride), float('nan'))
    for b, n in enumerate(lengths):
        m[b, :, :n] = torch.randn(80, n, generator=g) * 2 - 4
    return m


@pytest.fixture(scope='module')
def batch():
    import t2v_hip
    assert max(max(c) for c in CASES) == t2v_hip.DTW_MAX_FRAMES        # the supported maximum is among the cases
    nx, ny = [c[0] for c in CASES], [c[1] for c in CASES]
    x, y = _mels(nx, max(nx), 1), _mels(ny, max(ny) + 3, 2)
    ref = [dtw_ref(x[b, :, :nx[b]].numpy(), y[b, :, :ny[b]].numpy()) for b in range(len(CASES))]
    return x, nx, y, ny, ref


def test_batch_matches_fp64(batch):
    import t2v_hip
    x, nx, y, ny, ref = batch
    d = t2v_hip.mel_dtw(x.cuda(), nx, y.cuda(), ny).cpu().double().numpy()
    for b, (tx, ty) in enumerate(CASES):
        err = abs(d[b] - ref[b])
        print("(%d, %d): dist %.9g ref %.9g rel err %.3g bound %.3g" % (tx, ty, d[b], ref[b], err / ref[b], _tol(1.0, tx, ty)))
    for b, (tx, ty) in enumerate(CASES):
        assert abs(d[b] - ref[b]) <= _tol(ref[b], tx, ty), (tx, ty, d[b], ref[b])


def test_alone_matches_fp64_and_batch_bits(batch):
    import t2v_hip
    x, nx, y, ny, ref = batch
    d = t2v_hip.mel_dtw(x.cuda(), nx, y.cuda(), ny).cpu()
    again = t2v_hip.mel_dtw(x.cuda(), nx, y.cuda(), ny).cpu()
    assert again.numpy().tobytes() == d.numpy().tobytes()                           # a second run: the same bits
    for b, (tx, ty) in enumerate(CASES):
        # alone, cut to its own length: other strides, no padding at all
        a = t2v_hip.mel_dtw(x[b:b + 1, :, :tx].contiguous().cuda(), [tx], y[b:b + 1, :, :ty].contiguous().cuda(), [ty]).cpu()
        assert abs(float(a[0]) - ref[b]) <= _tol(ref[b], tx, ty), (tx, ty, float(a[0]), ref[b])
        assert a.numpy().tobytes() == d[b:b + 1].numpy().tobytes(), (tx, ty, float(a[0]), float(d[b]))


def test_self_distance_is_zero_and_symmetry(batch):
    import t2v_hip
    x, nx, y, ny, ref = batch
    xd, yd = x.cuda(), y.cuda()
    z = t2v_hip.mel_dtw(xd, nx, xd.clone(), nx).cpu()
    assert (z == 0).all(), z
    dxy = t2v_hip.mel_dtw(xd, nx, yd, ny).cpu().double().numpy()
    dyx = t2v_hip.mel_dtw(yd, ny, xd, nx).cpu().double().numpy()         # x_stride != y_stride both ways
    for b, (tx, ty) in enumerate(CASES):
        assert abs(dyx[b] - ref[b]) <= _tol(ref[b], tx, ty), (tx, ty)
        assert abs(dxy[b] - dyx[b]) <= _tol(ref[b], tx, ty), (tx, ty, dxy[b], dyx[b])


def test_single_frames_give_the_frame_distance():
    import t2v_hip
    x, y = _mels([1], 1, 3), _mels([1], 4, 4)
    d = float(t2v_hip.mel_dtw(x.cuda(), [1], y.cuda(), [1])[0])
    want = float(((x[0, :, 0].double() - y[0, :, 0].double()) ** 2).sum().sqrt())
    assert abs(d - want) <= want * 129 * 2.0 ** -23


def test_length_containers_agree():
    import t2v_hip
    nx, ny = [40, 17, 3], [9, 55, 64]
    x, y = _mels(nx, 48, 5).cuda(), _mels(ny, 64, 6).cuda()
    a = t2v_hip.mel_dtw(x, nx, y, ny).cpu()
    b = t2v_hip.mel_dtw(x, torch.tensor(nx), y, torch.tensor(ny, dtype=torch.int32)).cpu()
    c = t2v_hip.mel_dtw(x, torch.tensor(nx).cuda(), y, torch.tensor(ny, dtype=torch.int32).cuda()).cpu()
    assert torch.isfinite(a).all()
    assert a.numpy().tobytes() == b.numpy().tobytes() == c.numpy().tobytes()


def test_errors_leave_the_library_usable():
    import t2v_hip
    x, y = _mels([20, 20], 24, 7).cuda(), _mels([30, 30], 30, 8).cuda()
    good = t2v_hip.mel_dtw(x, [20, 20], y, [30, 30]).cpu()
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(x, [0, 20], y, [30, 30])                        # length 0
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(x, [20, 20], y, [30, 31])                       # length > stride
    big = torch.zeros(1, 80, t2v_hip.DTW_MAX_FRAMES + 1).cuda()
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(big, [t2v_hip.DTW_MAX_FRAMES + 1], y[:1], [30])   # length > maximum
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(x[:, :79].contiguous(), [20, 20], y[:, :79].contiguous(), [30, 30])     # n_mel != 80
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(x, [20, 20], y[:1], [30])                       # mismatched B
    with pytest.raises(ValueError):
        t2v_hip.mel_dtw(x, [20], y, [30, 30])                           # mismatched B in the lengths
    # the C entry itself refuses another channel count
    lib = t2v_hip.load_library()
    n = torch.tensor([20, 20], dtype=torch.int32).cuda()
    scratch = torch.empty(lib.t2v_mel_dtw_scratch_bytes(2, 24, 30), dtype=torch.uint8).cuda()
    out = torch.empty(2).cuda()
    rc = lib.t2v_mel_dtw(t2v_hip._p(x), t2v_hip._p(n), 24, t2v_hip._p(y), t2v_hip._p(n), 30, 2, 79, t2v_hip._p(out),
                         t2v_hip._p(scratch), t2v_hip._stream())
    assert rc == -1                                                     # T2V_ERR_DIMS
    # the maximum is longer than a long stride allows: a long stride alone is fine
    assert big.size(2) > t2v_hip.DTW_MAX_FRAMES
    ok = t2v_hip.mel_dtw(big, [5], y[:1], [30]).cpu()
    assert torch.isfinite(ok).all()
    after = t2v_hip.mel_dtw(x, [20, 20], y, [30, 30]).cpu()
    assert after.numpy().tobytes() == good.numpy().tobytes()
    t2v_hip.check_async_errors()


def test_group_split_gives_the_same_bits(monkeypatch):
    import t2v_hip
    nx, ny = [600, 3, 520, 77, 513, 1, 64, 300], [40, 600, 513, 90, 1, 1, 700, 300]
    x, y = _mels(nx, 600, 9).cuda(), _mels(ny, 700, 10).cuda()
    whole = t2v_hip.mel_dtw(x, nx, y, ny).cpu()
    per_pair = t2v_hip.load_library().t2v_mel_dtw_scratch_bytes(1, 600, 700)
    assert per_pair > 0
    calls = []
    real = t2v_hip.load_library().t2v_mel_dtw
    monkeypatch.setattr(t2v_hip, 'DTW_SCRATCH_CAP', 3 * per_pair)      # groups of 3, 3, 2
    lib = t2v_hip.load_library()

    class Spy(object):
        def __getattr__(self, name):
            return getattr(lib, name)

        def t2v_mel_dtw(self, *a):
            calls.append(a[6])
            return real(*a)

    monkeypatch.setattr(t2v_hip, '_lib', Spy())
    split = t2v_hip.mel_dtw(x, nx, y, ny).cpu()
    assert calls == [3, 3, 2]
    assert split.numpy().tobytes() == whole.numpy().tobytes()
    assert torch.isfinite(whole).all()
