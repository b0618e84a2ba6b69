"""t2v_hip.alignment_stats (csrc/align.hip) against the fp64 numpy reference of tests/align_ref.py.

Integers are exact: the path and the seven stats equal the reference's, ties included (equal fp32 maxima: the lowest index).
Tolerances (derived, not measured): focus and every mass_j are fp32 sums of n non-negative terms, so they lie within
n 2^-24 (reference value) of the fp64 value in any order of summation, the division of focus included.  The two threshold
counts compare mass_j with cover_min; every input's reference margin |mass_j - cover_min| exceeds that bound for every column
(align_ref.decided_row changes the seed until it does), so the counts are defined and must be exact too.  No row is left out.

Shapes: text widths 1, 63, 64, 65 and 577 (past one sweep of the 256 threads and past the training box), frame counts F - 1,
F, F + 1 and 3F + 2 around the F frames a workgroup owns, one ragged batch with n = 1 and L = 1 among five rows of different
lengths.  Padding past n and L holds 1e30 and some NaN."""
import functools

import numpy as np
import pytest
import torch

import align_ref

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 64, 65, 577)
POISON = 1e30


def _F():
    import t2v_hip
    return t2v_hip.ALIGN_FRAMES


def _poisoned(B, N, T_in, seed):
    A = np.full((B, N, T_in), POISON, dtype=np.float32)
    rs = np.random.RandomState(seed)
    for _ in range(max(4, A.size // 50)):
        A[rs.randint(B), rs.randint(N), rs.randint(T_in)] = np.nan
    return A


def _build(ns, Ls, N, T_in, seed):
    """(A (B, N, T_in) float32 with poison outside each row's n x L, references)"""
    A = _poisoned(len(ns), N, T_in, seed)
    refs = []
    for b, (n, L) in enumerate(zip(ns, Ls)):
        row, ref = align_ref.decided_row(n, L, 100 * seed + b)
        A[b, :n, :L] = row
        refs.append(ref)
    return A, refs


@functools.lru_cache(maxsize=None)
def _width_case(T_in):
    F = _F()
    ns = [F - 1, F, F + 1, 3 * F + 2]
    Ls = [T_in, max(1, T_in - 1), max(1, T_in // 2), T_in]
    A, refs = _build(ns, Ls, max(ns), T_in, T_in)
    return torch.from_numpy(A), ns, Ls, refs


@functools.lru_cache(maxsize=None)
def _ragged_case():
    F = _F()
    ns, Ls = [1, 3 * F + 2, 2 * F + 1, F + 1, F - 3], [30, 1, 577, 64, 300]
    A, refs = _build(ns, Ls, max(ns), max(Ls), 9)
    return torch.from_numpy(A), ns, Ls, refs


def _check(r, ns, Ls, refs, what):
    """asserts the module docstring's claims on every row; prints the worst float error over its bound"""
    path, mass, focus, stats = r.path.cpu().numpy(), r.mass.cpu().double().numpy(), r.focus.cpu().double().numpy(), r.stats.cpu().numpy()
    assert stats.shape == (len(ns), 8) and stats.dtype == np.int32 and path.dtype == np.int32
    worst = 0.0
    for b, (n, L, ref) in enumerate(zip(ns, Ls, refs)):
        bound = align_ref.sum_bound(n, ref['mass'])
        assert (ref['col_margin'] > bound).all(), (what, b, "the reference's margin must decide every threshold", ref['margin'])
        assert path[b, :n].tolist() == ref['path'].tolist(), (what, b)
        assert (path[b, n:] == -1).all(), (what, b)
        assert (mass[b, L:] == 0).all(), (what, b)
        err = np.abs(mass[b, :L] - ref['mass'])
        assert (err <= bound).all(), (what, b, float((err - bound).max()))
        fb = align_ref.sum_bound(n, ref['focus'])
        assert abs(focus[b] - ref['focus']) <= fb, (what, b, focus[b], ref['focus'])
        assert stats[b, :7].tolist() == ref['stats'], (what, b, stats[b].tolist(), ref['stats'])
        assert stats[b, 7] == 0
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()), abs(focus[b] - ref['focus']) / fb)
    print("%s: %d rows, worst float error / bound %.3f" % (what, len(ns), worst))


def _bits(r, b, n, L):
    return (r.focus[b:b + 1].cpu().numpy().tobytes(), r.mass[b, :L].cpu().numpy().tobytes(), r.path[b, :n].cpu().numpy().tobytes(),
            r.stats[b].cpu().numpy().tobytes())


def _alone_and_viewed(A, ns, Ls, r):
    """every row gives the batch's bits alone (cut to its own n x L: another stride, no padding) and through a slice of a
    larger poisoned tensor; the input is bit-identical after the calls"""
    import t2v_hip
    B, N, T_in = A.shape
    Ad = A.cuda()
    before = Ad.clone()
    for b, (n, L) in enumerate(zip(ns, Ls)):
        alone = t2v_hip.alignment_stats(Ad[b:b + 1, :n, :L].contiguous(), [n], [L])
        assert alone.path.shape == (1, n) and alone.mass.shape == (1, L)
        assert _bits(alone, 0, n, L) == _bits(r, b, n, L), b
    big = torch.from_numpy(_poisoned(B, N + 7, T_in + 5, 77)).cuda()
    big[:, 3:N + 3, 2:T_in + 2] = Ad
    view = big[:, 3:N + 3, 2:T_in + 2]
    assert not view.is_contiguous() and view.stride() == ((N + 7) * (T_in + 5), T_in + 5, 1)
    big_before = big.clone()
    rv = t2v_hip.alignment_stats(view, ns, Ls)
    for b, (n, L) in enumerate(zip(ns, Ls)):
        assert _bits(rv, b, n, L) == _bits(r, b, n, L), b
    assert rv.path.cpu().numpy().tobytes() == r.path.cpu().numpy().tobytes()
    assert rv.mass.cpu().numpy().tobytes() == r.mass.cpu().numpy().tobytes()
    assert big.view(torch.int32).equal(big_before.view(torch.int32))
    assert Ad.view(torch.int32).equal(before.view(torch.int32))


@pytest.mark.parametrize("T_in", WIDTHS)
def test_widths_and_frame_blocks_match_fp64(T_in):
    import t2v_hip
    A, ns, Ls, refs = _width_case(T_in)
    r = t2v_hip.alignment_stats(A.cuda(), ns, Ls)
    assert r.path.shape == (4, max(ns)) and r.mass.shape == (4, T_in) and r.focus.shape == (4,)
    _check(r, ns, Ls, refs, "T_in %d" % T_in)
    _alone_and_viewed(A, ns, Ls, r)


def test_ragged_batch_matches_fp64():
    import t2v_hip
    A, ns, Ls, refs = _ragged_case()
    Ad = A.cuda()
    r = t2v_hip.alignment_stats(Ad, ns, Ls)
    _check(r, ns, Ls, refs, "ragged")
    _alone_and_viewed(A, ns, Ls, r)
    assert r.stats[0, :5].tolist() == [refs[0]['stats'][0], refs[0]['stats'][0], 0, 0, 1]      # n = 1: one frame, no transitions
    assert r.stats[1].tolist() == [0, 0, 0, 0, ns[1], 0, 0, 0] and float(r.focus[1]) == 1.0     # L = 1: every frame on it
    # the stats columns by name, the three containers of the lengths, other parameters, and twice the same bits
    assert r.n_back.tolist() == [ref['stats'][2] for ref in refs] and r.longest_gap.tolist() == [ref['stats'][6] for ref in refs]
    with pytest.raises(AttributeError):
        r.n_forward
    a = t2v_hip.alignment_stats(Ad, torch.tensor(ns), torch.tensor(Ls, dtype=torch.int32).cuda())
    assert all(_bits(a, b, n, L) == _bits(r, b, n, L) for b, (n, L) in enumerate(zip(ns, Ls)))
    pick = [3, 0, 2]
    sub = t2v_hip.alignment_stats(Ad[pick], [ns[b] for b in pick], [Ls[b] for b in pick])
    assert all(_bits(sub, k, ns[b], Ls[b]) == _bits(r, b, ns[b], Ls[b]) for k, b in enumerate(pick))
    other = [align_ref.align(A[b].numpy(), n, L, max_jump=0, cover_min=0.05) for b, (n, L) in enumerate(zip(ns, Ls))]
    if all((o['col_margin'] > align_ref.sum_bound(n, o['mass'])).all() for o, n in zip(other, ns)):
        ro = t2v_hip.alignment_stats(Ad, ns, Ls, max_jump=0, cover_min=0.05)
        assert ro.stats[:, :7].tolist() == [o['stats'] for o in other]
    else:
        raise AssertionError("cover_min = 0.05 is undecided on the ragged case: change its seed")


def _one_hot_rows(path, L, peak=0.875):
    """(n, L) float32: `peak` on the path and the rest spread evenly (exact in fp32 for L - 1 a power of two)"""
    n = len(path)
    A = np.full((n, L), (1.0 - peak) / (L - 1), dtype=np.float32)
    A[np.arange(n), path] = peak
    return A


def test_constructed_path_and_ties():
    """A path with known back-steps, jumps, a stall and a gap, and exact ties across lanes, waves and sweeps"""
    import t2v_hip
    L = 513                                                                     # three sweeps of 256 threads
    path = [0, 1, 2, 2, 2, 2, 2, 3, 9, 10, 8, 9, 10, 14, 15, 15, 300, 299, 512, 512]
    # steps: +1 +1 0 0 0 0 +1 +6 +1 -2 +1 +1 +4 +1 0 +285 -1 +213 0
    A1 = _one_hot_rows(path, L)
    n1 = len(path)
    want1 = [512, 512, 2, 4, 5, L - 12, 299 - 16]
    # two steps back, four jumps over 3 (+6 +4 +285 +213), five frames on position 2; mass: 0.875 per visit and 2^-12 per other
    # frame, so exactly the 12 distinct positions visited are covered, and the longest gap lies between 15 and 299
    ties = np.zeros((7, L), dtype=np.float32)
    ties[0, [3, 259]] = 0.5                                                     # one thread, two sweeps
    ties[1, [70, 10]] = 0.5                                                     # two waves
    ties[2, [64, 65, 63]] = 0.25                                                # neighbours across a wave boundary
    ties[3, :] = 1.0 / 1024                                                     # every position equal: position 0
    ties[4, [511, 255, 512]] = 0.125                                            # last sweep against the first
    ties[5, [200, 456]] = 0.5
    ties[5, 100] = np.float32(0.5) - np.float32(2.0 ** -25)                     # one ulp under the tied maximum
    ties[6, [512]] = 1.0
    want_tie_path = [3, 10, 63, 0, 255, 200, 512]
    N = max(n1, 7) + 2
    A = np.full((2, N, L + 3), POISON, dtype=np.float32)
    A[0, :n1, :L] = A1
    A[1, :7, :L] = ties
    ns, Ls = [n1, 7], [L, L]
    refs = [align_ref.align(A[b], n, Lb) for b, (n, Lb) in enumerate(zip(ns, Ls))]
    assert refs[0]['path'].tolist() == path and refs[0]['stats'] == want1       # the reference agrees with the hand count
    assert refs[1]['path'].tolist() == want_tie_path
    r = t2v_hip.alignment_stats(torch.from_numpy(A).cuda(), ns, Ls)
    _check(r, ns, Ls, refs, "constructed")
    assert r.stats[0, :7].tolist() == want1 and r.path[1, :7].tolist() == want_tie_path
    # the same path with max_jump = 5 and 0: jumps +6 +285 +213, and every forward step over 0
    for mj, jumps in ((5, 3), (0, 11)):
        assert int(t2v_hip.alignment_stats(torch.from_numpy(A).cuda(), ns, Ls, max_jump=mj).n_jump[0]) == jumps


def test_teacher_forced_shape_is_accepted():
    """the (B, T_out, T_in) alignments of a training forward with int64 device lengths, as model(x) returns them"""
    import t2v_hip
    A, ns, Ls, refs = _width_case(65)
    r = t2v_hip.alignment_stats(A.cuda(), torch.tensor(ns).cuda(), torch.tensor(Ls).cuda())
    _check(r, ns, Ls, refs, "int64 device lengths")


def test_errors_name_the_numbers_and_leave_the_library_usable():
    import t2v_hip
    A, ns, Ls, refs = _width_case(63)
    Ad = A.cuda()
    B, N, T_in = Ad.shape
    good = t2v_hip.alignment_stats(Ad, ns, Ls)
    bad_calls = [
        (dict(n_frames=[0] + ns[1:]), r"1\.\.%d" % N), (dict(n_frames=ns[:-1] + [N + 1]), str(N + 1)),
        (dict(n_frames=ns[:-1]), r"must be %d" % B), (dict(n_frames=[float(v) for v in ns]), r"\d"),
        (dict(text_lengths=[0] + Ls[1:]), r"1\.\.%d" % T_in), (dict(text_lengths=Ls[:-1] + [T_in + 1]), str(T_in + 1)),
        (dict(text_lengths=Ls + [1]), r"must be %d" % B),
        (dict(max_jump=-1), "-1"), (dict(max_jump=1.5), r"1\.5"), (dict(cover_min=0.0), "0"), (dict(cover_min=-0.25), r"-0\.25"),
        (dict(cover_min=float('nan')), "nan"),
    ]
    for bad, pattern in bad_calls:
        kw = dict(n_frames=ns, text_lengths=Ls)
        kw.update(bad)
        with pytest.raises(ValueError, match=pattern):
            t2v_hip.alignment_stats(Ad, **kw)
    with pytest.raises(ValueError, match=r"\(%d, %d\)" % (N, T_in)):
        t2v_hip.alignment_stats(Ad[0], ns[:1], Ls[:1])                          # rank
    with pytest.raises(ValueError, match="float64"):
        t2v_hip.alignment_stats(Ad.double(), ns, Ls)
    with pytest.raises(ValueError, match="cpu"):
        t2v_hip.alignment_stats(A, ns, Ls)                                      # device
    with pytest.raises(ValueError, match=r"empty input \(0, "):
        t2v_hip.alignment_stats(Ad[:0], [], [])
    with pytest.raises(ValueError, match=r"strides \(\d+, 1, %d\)" % N):
        t2v_hip.alignment_stats(Ad.transpose(1, 2).contiguous().transpose(1, 2), ns, Ls)     # last-dimension stride != 1: rejected
    lib = t2v_hip.load_library()
    n, L = torch.tensor(ns, dtype=torch.int32).cuda(), torch.tensor(Ls, dtype=torch.int32).cuda()
    path, mass = torch.zeros(B, N, dtype=torch.int32).cuda(), torch.zeros(B, T_in).cuda()
    focus, stats = torch.zeros(B).cuda(), torch.zeros(B, 8, dtype=torch.int32).cuda()
    scratch = torch.zeros(lib.t2v_alignment_scratch_bytes(B, N, T_in), dtype=torch.uint8).cuda()
    p = t2v_hip._p

    def call(sb=N * T_in, st=T_in, B_=B, max_jump=3, cover_min=0.5, ps=N, ms=T_in, A_=Ad, sc=scratch):
        return lib.t2v_alignment_stats(p(A_), sb, st, p(n), p(L), B_, N, T_in, max_jump, cover_min, p(path), ps, p(mass), ms,
                                       p(focus), p(stats), p(sc), t2v_hip._stream())
    assert call(max_jump=-1) == -1 and call(cover_min=0.0) == -1 and call(cover_min=-1.0) == -1       # T2V_ERR_DIMS
    assert call(B_=0) == -2 and call(st=T_in - 1) == -2 and call(sb=N * T_in - 1) == -2               # T2V_ERR_ARG
    assert call(ps=N - 1) == -2 and call(ms=T_in - 1) == -2 and call(A_=None) == -2 and call(sc=None) == -2
    assert call() == 0
    torch.cuda.synchronize()
    assert path.cpu().numpy().tobytes() == good.path.cpu().numpy().tobytes()
    assert stats.cpu().numpy().tobytes() == good.stats.cpu().numpy().tobytes()
    # lengths outside the tensor are clamped on the device, and an empty row is all zeros: nothing faults, nothing is read
    n.copy_(torch.tensor([0, -5, N + 1000, ns[3]], dtype=torch.int32))
    L.copy_(torch.tensor([Ls[0], Ls[1], T_in, 0], dtype=torch.int32))
    clean = torch.from_numpy(align_ref.ridge_row(N, T_in, 4)).cuda()[None].repeat(B, 1, 1).contiguous()
    assert call(A_=clean) == 0
    torch.cuda.synchronize()
    for b in (0, 1, 3):
        assert stats[b].tolist() == [0] * 8 and float(focus[b]) == 0.0 and (path[b] == -1).all() and (mass[b] == 0).all()
    whole = t2v_hip.alignment_stats(clean[2:3], [N], [T_in])
    assert stats[2].tolist() == whole.stats[0].tolist() and path[2].tolist() == whole.path[0].tolist()
    again = t2v_hip.alignment_stats(Ad, ns, Ls)
    assert all(_bits(again, b, a, c) == _bits(good, b, a, c) for b, (a, c) in enumerate(zip(ns, Ls)))
    t2v_hip.check_async_errors()
