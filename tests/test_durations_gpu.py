"""t2v_hip.mas and t2v_hip.segment_means (csrc/durations.hip) against the fp64 restatement of tests/mas_ref.py, and
Synthesizer.durations / evaluate(durations=True) on the tiny random-init model of tests/test_evaluate_gpu.py.

The error bound of the random-row test is derived, not measured (mas_ref.gap_bound): a cell of Q is one logf and one fp32 add per
frame, so after t + 1 frames it carries at most (t + 1) (2^-24 M + e_log), with M = n |ln FLOOR| the bound of |Q| (weights <= 1:
every term lies in [ln FLOOR, 0]) and e_log = one ulp of |ln FLOOR|, logf's stated 1 ulp on the largest value it returns.  The
kernel's Q(n-1, L-1) lies within n (2^-24 M + e_log) of the fp64 score of its own path, the fp32 value of the true optimum within
the same of the fp64 optimum, and the kernel prefers its own: the fp64 score of the kernel's path lies at most
2 n (2^-24 M + e_log) below the fp64 optimum, and `score` within that / n of the fp64 mean along the kernel's path."""
import math

import numpy as np
import pytest
import torch

import mas_ref
from test_evaluate_gpu import setup  # noqa: F401  (setup is the fixture)

pytestmark = pytest.mark.gpu

PLANT_L = (1, 2, 63, 64, 65, 257, 577)


def _plant(n, L, S, rng):
    """a random monotonic path 0 .. L-1 over n frames with steps <= S"""
    p = np.zeros(n, dtype=np.int64)
    for t in range(1, n):
        left, after = L - 1 - p[t - 1], n - 1 - t                       # symbols still to cross, transitions after this one
        lo, hi = max(0, left - after * S), min(S, left)
        p[t] = p[t - 1] + rng.randint(lo, hi + 1)
    assert mas_ref.is_feasible_path(p, n, L, S)
    return p


def _planted_rows(S, seed):
    rng = np.random.RandomState(seed)
    cases = [(L, n) for L in PLANT_L for n in (L, L + 1, 3 * L)]
    cases.append((1, 1))                                                # the ragged batch ends in n = 1, L = 1
    N, T_in = max(n for _, n in cases), max(L for L, _ in cases)
    A = np.full((len(cases), N, T_in), np.nan, dtype=np.float32)        # padding: NaN behind n and L
    plants = []
    for b, (L, n) in enumerate(cases):
        p = _plant(n, L, S, rng)
        A[b, :n, :L] = 0.1 / max(L - 1, 1)
        A[b, np.arange(n), p] = 0.9
        plants.append(p)
    return cases, A, plants


@pytest.mark.parametrize('S', [1, 2, 3])
def test_planted_paths_come_back_exactly(S):
    import t2v_hip
    cases, A, plants = _planted_rows(S, 100 + S)
    for L, n in cases:
        if L >= 2:      # any other path leaves the plant in at least one frame: ln 0.9 - ln(0.1 / (L - 1)) there, no gain elsewhere
            assert math.log(9.0 * (L - 1)) > mas_ref.gap_bound(n), (L, n)
    one_frame = sum(int((mas_ref.segments(p, L)['durations'] == 1).sum()) for (L, _), p in zip(cases, plants))
    skipped = sum(int((mas_ref.segments(p, L)['durations'] == 0).sum()) for (L, _), p in zip(cases, plants))
    assert one_frame > 0 and (skipped > 0) == (S >= 2)
    if S == 1:
        assert all((p == np.arange(L)).all() for (L, n), p in zip(cases, plants) if n == L)       # the forced diagonal
    r = t2v_hip.mas(torch.from_numpy(A).cuda(), [n for _, n in cases], [L for L, _ in cases], S)
    path, dur, sta, score = r.path.cpu().numpy(), r.durations.cpu().numpy(), r.starts.cpu().numpy(), r.score.cpu().numpy()
    for b, ((L, n), p) in enumerate(zip(cases, plants)):
        seg = mas_ref.segments(p, L)
        assert (path[b, :n] == p).all() and (path[b, n:] == -1).all(), (S, L, n)
        assert (dur[b, :L] == seg['durations']).all() and (dur[b, L:] == 0).all(), (S, L, n)
        assert (sta[b, :L] == seg['starts']).all(), (S, L, n)
        assert abs(float(score[b]) - math.log(np.float32(0.9))) <= mas_ref.gap_bound(n) / n
    t2v_hip.check_async_errors()


def test_all_equal_rows_follow_the_tie_rule():
    import t2v_hip
    cases = [(1, 1), (7, 3), (64, 64), (130, 65), (300, 257)]
    N, T_in = max(n for n, _ in cases), max(L for _, L in cases)
    A = np.full((len(cases), N, T_in), 1e30, dtype=np.float32)
    for b, (n, L) in enumerate(cases):
        A[b, :n, :L] = np.float32(1.0 / L)                              # every cell of a row ties exactly, in fp32 and in fp64
    Ad = torch.from_numpy(A).cuda()
    for S in (1, 2, 3):
        r = t2v_hip.mas(Ad, [n for n, _ in cases], [L for _, L in cases], S)
        path, dur = r.path.cpu().numpy(), r.durations.cpu().numpy()
        for b, (n, L) in enumerate(cases):
            ref = mas_ref.search(A[b], n, L, S)
            assert (path[b, :n] == ref['path']).all(), (S, n, L)
            assert (dur[b, :L] == ref['durations']).all()


def _softmax_rows(cases, seed):
    rng = np.random.RandomState(seed)
    N, T_in = max(n for n, _ in cases), max(L for _, L in cases)
    A = np.full((len(cases), N, T_in), np.nan, dtype=np.float32)
    for b, (n, L) in enumerate(cases):
        x = rng.randn(n, L) * 4.0
        e = np.exp(x - x.max(1, keepdims=True))
        A[b, :n, :L] = (e / e.sum(1, keepdims=True)).astype(np.float32)
    A[:, :, T_in - 1:][np.isnan(A[:, :, T_in - 1:])] = 1e30             # and 1e30 in a part of the padding
    return A


RANDOM_CASES = [(1, 1), (40, 17), (97, 65), (270, 260), (300, 100)]


@pytest.fixture(scope='module')
def random_rows():
    A = _softmax_rows(RANDOM_CASES, 7)
    refs = {S: [mas_ref.search(A[b], n, L, S) for b, (n, L) in enumerate(RANDOM_CASES)] for S in (1, 2, 3)}
    return A, refs


@pytest.mark.parametrize('S', [1, 2, 3])
def test_random_rows_reach_the_optimum_within_the_derived_bound(random_rows, S):
    import t2v_hip
    A, refs = random_rows
    ns, Ls = [n for n, _ in RANDOM_CASES], [L for _, L in RANDOM_CASES]
    r = t2v_hip.mas(torch.from_numpy(A).cuda(), ns, Ls, S)
    path, dur, sta, score = r.path.cpu().numpy(), r.durations.cpu().numpy(), r.starts.cpu().numpy(), r.score.cpu().numpy()
    for b, (n, L) in enumerate(RANDOM_CASES):
        p, ref, bound = path[b, :n], refs[S][b], mas_ref.gap_bound(n)
        assert mas_ref.is_feasible_path(p, n, L, S) and (path[b, n:] == -1).all(), (S, n, L)
        assert dur[b, :L].sum() == n and (dur[b, :L] == np.bincount(p, minlength=L)).all() and (dur[b, L:] == 0).all()
        assert (sta[b, :L] == np.concatenate([[0], np.cumsum(dur[b, :L])[:-1]])).all()
        own = mas_ref.path_score(A[b], p, L)
        print("S %d n %d L %d: fp64 optimum %.9g, kernel's path %.9g, gap %.3g (bound %.3g), score error %.3g (bound %.3g)"
              % (S, n, L, ref['total'], own, ref['total'] - own, bound, abs(float(score[b]) - own / n), bound / n))
        assert own <= ref['total'] + 1e-9 * abs(ref['total'])
        assert ref['total'] - own <= bound, (S, n, L)
        assert abs(float(score[b]) - own / n) <= bound / n, (S, n, L)


def test_an_infeasible_row_is_refused_and_does_not_touch_its_neighbours():
    import t2v_hip
    A = _softmax_rows([(9, 6), (9, 6), (9, 6)], 3)
    Ad = torch.from_numpy(A).cuda()
    with pytest.raises(ValueError, match="no monotonic path"):
        t2v_hip.mas(Ad, [9, 5, 9], [6, 6, 6], 1)                        # n = L - 1
    for bad in (dict(max_step=0), dict(max_step=4), dict(max_step=True), dict(max_step=1.5)):
        with pytest.raises(ValueError):
            t2v_hip.mas(Ad, [9, 9, 9], [6, 6, 6], **bad)
    with pytest.raises(ValueError):
        t2v_hip.mas(Ad, [9, 10, 9], [6, 6, 6])
    with pytest.raises(ValueError):
        t2v_hip.mas(Ad, [9, 9], [6, 6, 6])
    with pytest.raises(ValueError):
        t2v_hip.mas(torch.zeros(1, 4, t2v_hip.MAS_MAX_SYMBOLS + 1).cuda(), [4], [4])
    with pytest.raises(ValueError):
        t2v_hip.mas(Ad.transpose(1, 2).contiguous().transpose(1, 2), [9, 9, 9], [6, 6, 6])
    good = t2v_hip.mas(Ad, [9, 9, 9], [6, 6, 6], 1)
    # through the C entry the row gets NaN / -1 / 0 and the others are what they are alone
    lib, p = t2v_hip.load_library(), t2v_hip._p
    B, N, T_in = A.shape
    n = torch.tensor([9, 5, 9], dtype=torch.int32).cuda()
    L = torch.tensor([6, 6, 6], dtype=torch.int32).cuda()
    path = torch.full((B, N), 77, dtype=torch.int32).cuda()
    dur, sta = torch.full((B, T_in), 77, dtype=torch.int32).cuda(), torch.full((B, T_in), 77, dtype=torch.int32).cuda()
    score = torch.zeros(B).cuda()
    scratch = torch.zeros(lib.t2v_mas_scratch_bytes(B, N, T_in), dtype=torch.uint8).cuda()
    assert scratch.numel() == B * N * T_in and lib.t2v_mas_scratch_bytes(1, 1, t2v_hip.MAS_MAX_SYMBOLS + 1) == 0

    def call(sb=N * T_in, st=T_in, B_=B, S=1, ps=N, ss=T_in, A_=Ad, sc=scratch, T=T_in):
        return lib.t2v_mas(p(A_), sb, st, p(n), p(L), B_, N, T, S, p(path), ps, p(dur), p(sta), ss, p(score), p(sc),
                           t2v_hip._stream())
    assert call(S=0) == -1 and call(S=4) == -1                          # T2V_ERR_DIMS
    assert call(T=t2v_hip.MAS_MAX_SYMBOLS + 1, st=4096, sb=N * 4096, ss=4096) == -1
    assert call(B_=0) == -2 and call(st=T_in - 1) == -2 and call(sb=N * T_in - 1) == -2                # T2V_ERR_ARG
    assert call(ps=N - 1) == -2 and call(ss=T_in - 1) == -2 and call(A_=None) == -2 and call(sc=None) == -2
    assert call() == 0
    torch.cuda.synchronize()
    assert math.isnan(float(score[1])) and (path[1] == -1).all() and (dur[1] == 0).all() and (sta[1] == 0).all()
    for b in (0, 2):
        assert path[b].tolist() == good.path[b].tolist() and dur[b].tolist() == good.durations[b].tolist()
        assert sta[b].tolist() == good.starts[b].tolist() and float(score[b]) == float(good.score[b])
    # lengths outside the tensor are clamped on the device: nothing faults, a row clamped to nothing is the infeasible row
    n.copy_(torch.tensor([N + 1000, -3, 9], dtype=torch.int32))
    L.copy_(torch.tensor([T_in + 1000, 6, 0], dtype=torch.int32))
    assert call() == 0
    torch.cuda.synchronize()
    assert path[0].tolist() == good.path[0].tolist() and float(score[0]) == float(good.score[0])
    for b in (1, 2):
        assert math.isnan(float(score[b])) and (path[b] == -1).all() and (dur[b] == 0).all()
    t2v_hip.check_async_errors()


def _bits(r, b, n, L):
    return (r.path[b, :n].cpu().numpy().tobytes(), r.durations[b, :L].cpu().numpy().tobytes(),
            r.starts[b, :L].cpu().numpy().tobytes(), r.score[b:b + 1].cpu().numpy().tobytes())


def test_padding_and_independence(random_rows):
    import t2v_hip
    A, _ = random_rows
    ns, Ls = [n for n, _ in RANDOM_CASES], [L for _, L in RANDOM_CASES]
    Ad = torch.from_numpy(A).cuda()
    before = Ad.clone()
    for S in (1, 3):
        whole = t2v_hip.mas(Ad, ns, Ls, S)
        for b, (n, L) in enumerate(RANDOM_CASES):
            alone = t2v_hip.mas(Ad[b:b + 1, :n, :L].contiguous(), [n], [L], S)
            assert _bits(alone, 0, n, L) == _bits(whole, b, n, L), (S, b)
            assert (whole.path[b, n:] == -1).all() and (whole.durations[b, L:] == 0).all()
        pick = [3, 1, 4]
        sub = t2v_hip.mas(Ad[pick], [ns[b] for b in pick], [Ls[b] for b in pick], S)
        assert all(_bits(sub, k, ns[b], Ls[b]) == _bits(whole, b, ns[b], Ls[b]) for k, b in enumerate(pick))
        B, N, T_in = A.shape
        big = torch.full((B + 1, N + 5, T_in + 9), float('nan'), device='cuda')
        big[1:, 2:N + 2, 4:T_in + 4] = Ad
        view = big[1:, 2:N + 2, 4:T_in + 4]
        assert not view.is_contiguous()
        rv = t2v_hip.mas(view, ns, Ls, S)
        assert all(_bits(rv, b, n, L) == _bits(whole, b, n, L) for b, (n, L) in enumerate(RANDOM_CASES))
    assert Ad.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()         # the input is bit-identical afterwards
    # outputs as views inside guard-filled buffers: the rows in front of and behind them keep their guards
    lib, p = t2v_hip.load_library(), t2v_hip._p
    B, N, T_in = A.shape
    n, L = torch.tensor(ns, dtype=torch.int32).cuda(), torch.tensor(Ls, dtype=torch.int32).cuda()
    ps, ss = N + 3, T_in + 7
    path = torch.full((B + 2, ps), 1234567, dtype=torch.int32).cuda()
    dur, sta = torch.full((B + 2, ss), 1234567, dtype=torch.int32).cuda(), torch.full((B + 2, ss), 1234567, dtype=torch.int32).cuda()
    score = torch.full((B + 2,), 5.0).cuda()
    scratch = torch.zeros(lib.t2v_mas_scratch_bytes(B, N, T_in) + 64, dtype=torch.uint8).cuda()
    scratch[-64:] = 0xAB
    assert lib.t2v_mas(p(Ad), N * T_in, T_in, p(n), p(L), B, N, T_in, 1, p(path[1:]), ps, p(dur[1:]), p(sta[1:]), ss,
                       p(score[1:]), p(scratch), t2v_hip._stream()) == 0
    torch.cuda.synchronize()
    whole = t2v_hip.mas(Ad, ns, Ls, 1)
    for buf in (path, dur, sta):
        assert (buf[0] == 1234567).all() and (buf[-1] == 1234567).all()
    assert float(score[0]) == 5.0 and float(score[-1]) == 5.0 and (scratch[-64:] == 0xAB).all()
    for b, (n_, L_) in enumerate(RANDOM_CASES):
        assert path[1 + b, :n_].tolist() == whole.path[b, :n_].tolist() and (path[1 + b, n_:] == -1).all()
        assert dur[1 + b, :L_].tolist() == whole.durations[b, :L_].tolist() and (dur[1 + b, L_:] == 0).all()
    t2v_hip.check_async_errors()


def test_segment_means_against_fp64_sums():
    import t2v_hip
    rng = np.random.RandomState(5)
    cases = [(300, 257), (40, 17), (1, 1), (90, 64)]
    B, N, T_in = len(cases), 300, 257
    starts, durs = np.zeros((B, T_in), dtype=np.int32), np.zeros((B, T_in), dtype=np.int32)
    for b, (n, L) in enumerate(cases):
        seg = mas_ref.segments(_plant(n, L, 2, rng), L)                  # steps of 2: symbols of duration 0 among them
        starts[b, :L], durs[b, :L] = seg['starts'], seg['durations']
    assert (durs[:, :17] == 0).any() and (durs == 1).any()
    v = (rng.randn(B, N) * 100.0).astype(np.float32)
    counted = rng.rand(B, N) < 0.6
    vd, sd, dd = torch.from_numpy(v).cuda(), torch.from_numpy(starts).cuda(), torch.from_numpy(durs).cuda()
    for mask in (None, counted):
        r = t2v_hip.segment_means(vd, None if mask is None else torch.from_numpy(mask).cuda(), sd, dd)
        sums, counts = r.sums.cpu().numpy(), r.counts.cpu().numpy()
        for b in range(B):
            for j in range(T_in):
                s, d = int(starts[b, j]), int(durs[b, j])
                keep = np.ones(d, dtype=bool) if mask is None else mask[b, s:s + d]
                seg = v[b, s:s + d].astype(np.float64)[keep]
                assert counts[b, j] == len(seg), (b, j)
                assert abs(float(sums[b, j]) - seg.sum()) <= d * 2.0 ** -24 * np.abs(seg).sum(), (b, j)
                if d == 0:
                    assert counts[b, j] == 0 and sums[b, j] == 0.0
    m = t2v_hip.segment_means(vd, None, sd, dd).means.cpu().numpy()
    assert np.isnan(m[durs == 0]).all() and np.isfinite(m[durs > 0]).all()
    with pytest.raises(ValueError):
        t2v_hip.segment_means(vd, torch.from_numpy(counted[:, :10]).cuda(), sd, dd)
    with pytest.raises(ValueError):
        t2v_hip.segment_means(vd, None, sd.long(), dd)
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.segment_means(vd.cpu(), None, sd, dd)
    t2v_hip.check_async_errors()


PLAIN_KEYS = {'dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion'}


def test_synthesizer_durations_and_evaluate(setup):
    import t2v_hip
    from evaluation import DURATION_F0_KEYS, DURATION_KEYS, PROSODY_KEYS, duration_fields, summarize
    from synthesizer import GriffinLimVocoder
    from text import text_to_sequence
    syn, rows = setup['syn'], setup['rows'][:3]
    dec = syn.model.decoder
    S = 3
    recs = syn.evaluate(rows, 2, durations=True, max_step=S)            # groups (0, 1) and (2)
    assert dec._calls == len(rows)                                      # the teacher-forced passes took no decoder seed
    assert all(set(r) == PLAIN_KEYS | set(DURATION_KEYS) for r in recs)
    dec._calls = 0
    plain = syn.evaluate(rows, 2)
    assert all(set(r) == PLAIN_KEYS for r in plain)
    assert [{k: r[k] for k in PLAIN_KEYS} for r in recs] == plain       # without the flag: the parent's records, key for key
    # the recordings: durations sum to the true frame counts, and a row does not depend on its group
    truth_n = syn.load_mels([r[0] for r in rows])[1]
    rec = syn.durations(rows, batch_size=2, max_step=S)
    assert dec._calls == len(rows)
    Ls = [len(text_to_sequence(r[1], ['korean_cleaners'])) for r in rows]
    for i, d in enumerate(rec):
        assert set(d) == {'durations', 'starts', 'n_frames', 'n_symbols', 'align_logp'}
        assert d['n_frames'] == truth_n[i] == recs[i]['n_ref_frames'] and d['n_symbols'] == Ls[i]
        if t2v_hip.mas_feasible(d['n_frames'], Ls[i], S):
            assert sum(d['durations']) == d['n_frames'] and len(d['durations']) == Ls[i] and min(d['durations']) >= 0
            assert d['starts'] == [sum(d['durations'][:j]) for j in range(Ls[i])]
            assert mas_ref.LN_FLOOR * -1 <= d['align_logp'] <= 0.0
        else:
            assert d['durations'] is None and d['starts'] is None and d['align_logp'] is None
    assert syn.durations(rows[1:2], batch_size=1, max_step=S) == rec[1:2]
    assert syn.durations(rows[::-1], batch_size=3, max_step=S) == rec[::-1]
    # the synthesis: the same decoder seeds give the alignments evaluate() searched
    dec._calls = 0
    al = syn.alignment([r[1] for r in rows], True, [r[0] for r in rows], batch_size=2, mas=True, max_step=S)
    dec._calls = 0
    without = syn.alignment([r[1] for r in rows], True, [r[0] for r in rows], batch_size=2)
    assert [{k: v for k, v in a.items() if k not in ('mas_durations', 'align_logp')} for a in al] == without
    both = 0
    for i, (a, d, r) in enumerate(zip(al, rec, recs)):
        assert a['n_frames'] == r['n_frames']
        if t2v_hip.mas_feasible(a['n_frames'], Ls[i], S):
            assert sum(a['mas_durations']) == a['n_frames'] and len(a['mas_durations']) == Ls[i]
        else:
            assert a['mas_durations'] is None and a['align_logp'] is None
        assert {k: r[k] for k in DURATION_KEYS} == duration_fields(a['mas_durations'], d['durations'], a['align_logp'], d['align_logp'])
        both += r['dur_rmse_frames'] is not None
    assert both >= 1, "no row has a path on both sides: the comparison was never made"
    s = summarize(recs)['overall']
    assert s['n_durations'] == sum(1 for r in recs if not r['hit_max'] and r['dur_rmse_frames'] is not None)
    assert 'n_durations' not in summarize(plain)['overall']
    with pytest.raises(ValueError):
        syn.evaluate(rows, 2, durations=True, max_step=4)
    with pytest.raises(ValueError):
        syn.durations(rows, max_step=0)
    # with prosody: the pitch per symbol, over the waveforms prosody already makes
    syn.vocoder = GriffinLimVocoder(syn.stft)
    dec._calls = 0
    np.random.seed(3)
    pros = syn.evaluate(rows[:2], 2, prosody=True, durations=True, max_step=S)
    assert all(set(r) == PLAIN_KEYS | set(PROSODY_KEYS) | set(DURATION_KEYS) | set(DURATION_F0_KEYS) for r in pros)
    assert [{k: r[k] for k in DURATION_KEYS} for r in pros] == [{k: r[k] for k in DURATION_KEYS} for r in recs[:2]]
    for r in pros:
        assert r['seg_f0_rmse_cents'] is None or (math.isfinite(r['seg_f0_rmse_cents']) and r['seg_f0_rmse_cents'] >= 0.0)
        assert r['seg_f0_corr'] is None or -1.0 <= r['seg_f0_corr'] <= 1.0
    syn.vocoder = GriffinLimVocoder(syn.stft, speed=1.5)
    with pytest.raises(ValueError, match="time axis"):
        syn.evaluate(rows[:2], 2, prosody=True, durations=True)
    t2v_hip.check_async_errors()
