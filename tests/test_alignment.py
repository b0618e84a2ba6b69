"""Alignment scoring, host side: the fp64 reference (tests/align_ref.py) on hand-written matrices, evaluation.alignment_fields
and evaluation.summarize with and without alignment records, evaluate.py --alignment's argument parsing and the library's
export and binding of t2v_alignment_stats."""
import os
import re

import numpy as np
import pytest

import align_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- the reference itself
def test_reference_on_a_hand_written_matrix():
    """6 frames x 8 positions, 0.75 on the path (0, 1, 1, 5, 4, 7) and 0.25 on position 0 (1 where the path is on 0)"""
    A = np.zeros((7, 9), dtype=np.float32)
    path = [0, 1, 1, 5, 4, 7]
    for t, p in enumerate(path):
        A[t, 0] += 0.25
        A[t, p] += 0.75
    A[6, :] = 9.0                                                              # past n: never looked at
    A[:, 8] = 9.0                                                              # past L
    r = align_ref.align(A, 6, 8, max_jump=2, cover_min=0.5)
    assert r['path'].tolist() == path
    assert r['mass'].tolist() == [2.25, 1.5, 0.0, 0.0, 0.75, 0.75, 0.0, 0.75]
    assert r['focus'] == pytest.approx((1.0 + 5 * 0.75) / 6)
    # furthest 7, last 7, one step back (5 -> 4), jumps over 2: 1 -> 5 and 4 -> 7, stall (1, 1) = 2 frames,
    # uncovered 2, 3, 6: 3 of them, longest gap 2
    assert r['stats'] == [7, 7, 1, 2, 2, 3, 2]
    assert r['margin'] == pytest.approx(0.25)
    tie = np.array([[0.25, 0.5, 0.5, 0.0]], dtype=np.float32)
    assert align_ref.align(tie, 1, 4)['path'].tolist() == [1]                   # equal maxima: the lowest index
    assert align_ref.align(tie, 1, 4)['stats'] == [1, 1, 0, 0, 1, 2, 1]
    assert align_ref.align(tie, 1, 1)['stats'] == [0, 0, 0, 0, 1, 1, 1]


def test_reference_inputs_are_softmax_rows_with_decided_thresholds():
    row, ref = align_ref.decided_row(20, 33, 5)
    assert row.dtype == np.float32 and row.shape == (20, 33)
    assert np.abs(row.astype(np.float64).sum(axis=1) - 1).max() < 1e-6
    assert ref['path'][0] <= 2 and ref['path'][-1] >= 30                        # the ridge walks the text
    assert (ref['col_margin'] > align_ref.sum_bound(20, ref['mass'])).all()


# ---------------------------------------------------------------------- evaluation.alignment_fields
def test_alignment_fields():
    from evaluation import ALIGNMENT_KEYS, alignment_fields
    assert ALIGNMENT_KEYS == ('focus', 'reach', 'end_reach', 'back_share', 'jump_share', 'stall_frames', 'uncovered_share',
                              'gap_symbols', 'n_symbols')
    # one frame: no transitions, the shares are 0.0
    f = alignment_fields(0.5, [3, 3, 0, 0, 1, 9, 6, 0], 1, 10)
    assert set(f) == set(ALIGNMENT_KEYS)
    assert f == {'focus': 0.5, 'reach': 0.4, 'end_reach': 0.4, 'back_share': 0.0, 'jump_share': 0.0, 'stall_frames': 1,
                 'uncovered_share': 0.9, 'gap_symbols': 6, 'n_symbols': 10}
    # one symbol: every frame stalls on it
    f = alignment_fields(1.0, [0, 0, 0, 0, 7, 0, 0], 7, 1)                      # seven words: the reserved one is optional
    assert f['reach'] == 1.0 and f['end_reach'] == 1.0 and f['stall_frames'] == 7 and f['uncovered_share'] == 0.0
    assert f['back_share'] == 0.0 and f['n_symbols'] == 1
    # a row with a gap: 5 of 20 symbols uncovered, 4 of them in a row
    f = alignment_fields(0.8, [19, 19, 0, 1, 3, 5, 4, 0], 41, 20)
    assert f['uncovered_share'] == 0.25 and f['gap_symbols'] == 4 and f['jump_share'] == pytest.approx(1 / 40)
    assert f['reach'] == 1.0 and f['end_reach'] == 1.0
    # a row that goes back: 3 of 10 transitions, and ends early
    f = alignment_fields(0.6, [15, 11, 3, 2, 2, 0, 0, 0], 11, 16)
    assert f['back_share'] == pytest.approx(0.3) and f['jump_share'] == pytest.approx(0.2)
    assert f['reach'] == 1.0 and f['end_reach'] == 0.75
    with pytest.raises(ValueError, match="0 frames"):
        alignment_fields(0.0, [0] * 8, 0, 5)


# ---------------------------------------------------------------------- evaluation.summarize
def _rec(dtw, n, n_ref, hit, emo, **more):
    return dict({'dtw': dtw, 'n_frames': n, 'n_ref_frames': n_ref, 'hit_max': hit, 'emotion': emo}, **more)


def _al(focus, furthest, p_last, n_back, n_jump, stall, n_unc, gap, n, L):
    from evaluation import alignment_fields
    return alignment_fields(focus, [furthest, p_last, n_back, n_jump, stall, n_unc, gap, 0], n, L)


PLAIN_KEYS = {'n_rows', 'n_hit_max', 'hit_max_share', 'n_scored', 'dtw_mean', 'dtw_median', 'length_ratio_mean'}
ALIGNMENT_STATS = {'n_alignment', 'focus_mean', 'reach_mean', 'back_share_mean', 'jump_share_mean', 'uncovered_share_mean',
                   'stall_frames_mean', 'stall_frames_max', 'gap_symbols_mean', 'gap_symbols_max', 'n_read_through',
                   'read_through_share'}


def test_summarize_without_alignment_records_is_unchanged():
    from evaluation import summarize
    recs = [_rec(1.0, 100, 100, False, 0), _rec(3.0, 90, 100, False, 0), _rec(9.0, 600, 100, True, 3)]
    s = summarize(recs)
    assert s['overall'] == {'n_rows': 3, 'n_hit_max': 1, 'hit_max_share': 1 / 3, 'n_scored': 2, 'dtw_mean': 2.0,
                            'dtw_median': 2.0, 'length_ratio_mean': (1.0 + 0.9 + 6.0) / 3}
    assert s['by_emotion']['ang'] == {'n_rows': 0, 'n_hit_max': 0, 'hit_max_share': None, 'n_scored': 0, 'dtw_mean': None,
                                      'dtw_median': None, 'length_ratio_mean': None}
    assert s == summarize(recs, end_slack=0, gap_min=1, back_slack=0)           # the thresholds cut alignment keys only


def _records():
    return [
        _rec(1.0, 101, 100, False, 0, **_al(0.9, 19, 19, 0, 0, 6, 0, 0, 101, 20)),      # reads through
        _rec(2.0, 101, 100, False, 0, **_al(0.7, 19, 16, 2, 1, 8, 3, 3, 101, 20)),      # ends 3 short, 2 back, gap 3: still through
        _rec(3.0, 51, 100, False, 1, **_al(0.5, 19, 15, 0, 4, 4, 6, 2, 51, 20)),        # ends 4 short
        _rec(4.0, 51, 100, False, 1, **_al(0.6, 19, 19, 0, 5, 3, 5, 4, 51, 20)),        # a gap of 4
        _rec(5.0, 51, 100, False, 1, **_al(0.4, 19, 19, 3, 0, 2, 0, 0, 51, 20)),        # 3 steps back
        _rec(6.0, 600, 100, True, 1, **_al(0.1, 5, 2, 90, 80, 200, 15, 14, 600, 20)),   # never stopped: counted out
    ]


def test_summarize_with_alignment_records():
    from evaluation import BACK_SLACK, END_SLACK, GAP_MIN, summarize
    assert (END_SLACK, GAP_MIN, BACK_SLACK) == (3, 4, 2)
    recs = _records()
    s = summarize(recs)
    o = s['overall']
    assert set(o) == PLAIN_KEYS | ALIGNMENT_STATS
    assert o['n_rows'] == 6 and o['n_hit_max'] == 1 and o['n_scored'] == 5 and o['dtw_mean'] == pytest.approx(3.0)
    assert o['n_alignment'] == 5                                                # the row that hit max_decoder_steps is out
    assert o['focus_mean'] == pytest.approx((0.9 + 0.7 + 0.5 + 0.6 + 0.4) / 5)
    assert o['reach_mean'] == pytest.approx(1.0)
    assert o['back_share_mean'] == pytest.approx((0 + 2 / 100 + 0 + 0 + 3 / 50) / 5)
    assert o['jump_share_mean'] == pytest.approx((0 + 1 / 100 + 4 / 50 + 5 / 50 + 0) / 5)
    assert o['uncovered_share_mean'] == pytest.approx((0 + 3 + 6 + 5 + 0) / 20 / 5)
    assert o['stall_frames_mean'] == pytest.approx((6 + 8 + 4 + 3 + 2) / 5) and o['stall_frames_max'] == 8
    assert o['gap_symbols_mean'] == pytest.approx((0 + 3 + 2 + 4 + 0) / 5) and o['gap_symbols_max'] == 4
    assert o['n_read_through'] == 2 and o['read_through_share'] == pytest.approx(2 / 5)
    neu, sad = s['by_emotion']['neu'], s['by_emotion']['sad']
    assert neu['n_alignment'] == 2 and neu['n_read_through'] == 2 and neu['read_through_share'] == 1.0
    assert sad['n_rows'] == 4 and sad['n_alignment'] == 3 and sad['n_read_through'] == 0 and sad['stall_frames_max'] == 4
    ang = s['by_emotion']['ang']                                                # an empty emotion: None statistics
    assert set(ang) == PLAIN_KEYS | ALIGNMENT_STATS
    assert ang['n_alignment'] == 0 and ang['n_read_through'] == 0
    assert all(ang[k] is None for k in ALIGNMENT_STATS - {'n_alignment', 'n_read_through'})


def test_summarize_thresholds_by_keyword():
    from evaluation import reads_through, summarize
    recs = _records()
    assert summarize(recs, end_slack=4)['overall']['n_read_through'] == 3
    assert summarize(recs, gap_min=5)['overall']['n_read_through'] == 3
    assert summarize(recs, back_slack=3)['overall']['n_read_through'] == 3
    assert summarize(recs, end_slack=4, gap_min=5, back_slack=3)['overall']['read_through_share'] == 1.0
    assert summarize(recs, end_slack=2)['overall']['n_read_through'] == 1
    assert summarize(recs, back_slack=1)['overall']['n_read_through'] == 1
    assert summarize(recs, gap_min=3)['overall']['n_read_through'] == 1
    assert [reads_through(r) for r in recs[:5]] == [True, True, False, False, False]
    # the other statistics do not move with the thresholds
    a, b = summarize(recs)['overall'], summarize(recs, end_slack=0, gap_min=1, back_slack=0)['overall']
    assert {k: v for k, v in a.items() if 'read_through' not in k} == {k: v for k, v in b.items() if 'read_through' not in k}


def test_summarize_with_both_key_sets():
    from evaluation import summarize
    pro = {'f0_median_hz': 220.0, 'f0_ref_median_hz': 110.0, 'f0_spread_st': 1.0, 'f0_ref_spread_st': 2.0, 'voiced_share': 0.5,
           'voiced_ref_share': 0.6, 'f0_shift_st': 12.0}
    recs = [dict(r, **pro) for r in _records()]
    o = summarize(recs)['overall']
    assert PLAIN_KEYS | ALIGNMENT_STATS | {'n_prosody', 'f0_shift_st_mean'} <= set(o)
    assert o['n_prosody'] == 5 and o['n_alignment'] == 5


# ---------------------------------------------------------------------- command line, header and binding
def test_evaluate_cli_parses_alignment():
    import evaluate
    base = ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']
    assert evaluate.parse_args(base).alignment is False
    args = evaluate.parse_args(base + ['--alignment', '--prosody', '--condition', 'emotion'])
    assert args.alignment is True and args.prosody is True
    text = evaluate.build_arg_parser().format_help()
    assert '--alignment' in text and 'read_through_share' in text
    assert 'read_through_share' in evaluate.__doc__ and 'not calibrated' in evaluate.__doc__


def test_alignment_stats_is_declared_exported_and_bound():
    import t2v_hip
    with open(os.path.join(ROOT, 'include', 't2vae.h')) as f:
        text = f.read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    protos = dict(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    lib = t2v_hip.load_library()
    for name in ('t2v_alignment_stats', 't2v_alignment_scratch_bytes'):
        assert name in protos and name in t2v_hip.EXPORTS and hasattr(lib, name)
        assert protos[name].count(',') + 1 == len(getattr(lib, name).argtypes), name
    assert int(re.search(r'#define\s+T2V_ALIGN_FRAMES\s+(\d+)', text).group(1)) == t2v_hip.ALIGN_FRAMES
    assert t2v_hip.ALIGN_STATS == align_ref.STATS
    # the scratch: one column partial per frame block and text position, one focus partial per block, fp32
    F = t2v_hip.ALIGN_FRAMES
    assert lib.t2v_alignment_scratch_bytes(1, 1, 1) == 4 * 2
    assert lib.t2v_alignment_scratch_bytes(3, F + 1, 577) == 4 * 3 * 2 * 578
    assert lib.t2v_alignment_scratch_bytes(64, 800, 555) == 4 * 64 * ((800 + F - 1) // F) * 556
    assert lib.t2v_alignment_scratch_bytes(0, 5, 5) == 0 and lib.t2v_alignment_scratch_bytes(1, 0, 5) == 0


def test_alignment_stats_host_checks_need_no_device():
    import torch
    import t2v_hip
    with pytest.raises(t2v_hip.T2VHipError):                                    # no CPU path ...
        t2v_hip.alignment_stats(torch.zeros(1, 4, 5), [4], [5])
    with pytest.raises(ValueError, match=r"\(1, 4, 5\)"):                       # ... and a bad argument, with its shape
        t2v_hip.alignment_stats(torch.zeros(1, 4, 5), [4], [5])
    with pytest.raises(ValueError, match="float64"):
        t2v_hip.alignment_stats(torch.zeros(1, 4, 5, dtype=torch.float64), [4], [5])
    with pytest.raises(ValueError, match=r"\(4, 5\)"):
        t2v_hip.alignment_stats(torch.zeros(4, 5), [4], [5])
