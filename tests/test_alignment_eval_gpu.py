"""Synthesizer.evaluate(alignment=True), Synthesizer.alignment and evaluate.py --alignment on a random-init model (the setup
of tests/test_evaluate_gpu.py: short texts, max_decoder_steps = 24, a gate bias under which some rows stop and some never do):
the records equal evaluation.alignment_fields of the fp64 reference (tests/align_ref.py) on the alignments synthesize_batch
returns for the same texts, conditioning and decoder seeds, and without the flag nothing changes."""
import json

import numpy as np
import pytest
import align_ref
from test_evaluate_gpu import STEPS, setup  # noqa: F401  (setup is the fixture)

pytestmark = pytest.mark.gpu

PLAIN_KEYS = {'dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion'}
ONE_HOT = {0: (1, 0, 0, 0), 1: (0, 1, 0, 0), 2: (0, 0, 0, 1), 3: (0, 0, 1, 0)}       # (neu, sad, hap, ang) of the label ids


def _want(al):
    """the record fields of one alignment (1, n, L) as synthesize_batch returns it, and the bound on focus"""
    from evaluation import alignment_fields
    A = al[0].cpu().numpy()
    n, L = A.shape
    ref = align_ref.align(A, n, L)
    assert (ref['col_margin'] > align_ref.sum_bound(n, ref['mass'])).all(), "an undecided threshold: change the model seed"
    return alignment_fields(ref['focus'], ref['stats'], n, L), align_ref.sum_bound(n, ref['focus'])


def _same_fields(got, want, focus_bound, what):
    from evaluation import ALIGNMENT_KEYS
    for k in ALIGNMENT_KEYS:
        if k == 'focus':
            assert abs(got[k] - want[k]) <= focus_bound, (what, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


def test_evaluate_alignment_equals_the_reference(setup):
    from evaluation import ALIGNMENT_KEYS, summarize
    syn, rows = setup['syn'], setup['rows'][:3]
    dec = syn.model.decoder
    recs = syn.evaluate(rows, 2, alignment=True)                                # groups (0, 1) and (2)
    assert dec._calls == len(rows)
    assert all(set(r) == PLAIN_KEYS | set(ALIGNMENT_KEYS) for r in recs)
    dec._calls = 0
    plain = syn.evaluate(rows, 2)
    assert all(set(r) == PLAIN_KEYS for r in plain)
    assert [{k: r[k] for k in PLAIN_KEYS} for r in recs] == plain                # the same decoder seeds, the same scores
    assert [r['n_frames'] for r in recs] == setup['n_want'][:3]
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        dec._calls = i0                                                         # the seeds evaluate() gave this group
        outs = syn.synthesize_batch([r[1] for r in g], None, True, [r[0] for r in g])
        for b, (post, al) in enumerate(outs):
            rec = recs[i0 + b]
            assert al.shape[1] == rec['n_frames'] == post.size(2) and al.shape[2] == rec['n_symbols']
            want, bound = _want(al)
            print("row %d: %d frames x %d symbols: %s" % (i0 + b, al.shape[1], al.shape[2], {k: rec[k] for k in ALIGNMENT_KEYS}))
            _same_fields(rec, want, bound, i0 + b)
    s = summarize(recs)['overall']
    stopped = [r for r in recs if not r['hit_max']]
    assert s['n_alignment'] == len(stopped) == s['n_scored']
    if stopped:
        assert s['focus_mean'] == pytest.approx(np.mean([r['focus'] for r in stopped]))
        assert s['stall_frames_max'] == max(r['stall_frames'] for r in stopped)


def test_alignment_combines_with_prosody(setup):
    from evaluation import ALIGNMENT_KEYS, PROSODY_KEYS
    from synthesizer import GriffinLimVocoder
    syn, rows = setup['syn'], setup['rows'][:2]
    dec = syn.model.decoder
    only = syn.evaluate(rows, 2, alignment=True)
    syn.vocoder = GriffinLimVocoder(syn.stft)
    dec._calls = 0
    np.random.seed(3)
    both = syn.evaluate(rows, 2, prosody=True, alignment=True)
    assert all(set(r) == PLAIN_KEYS | set(PROSODY_KEYS) | set(ALIGNMENT_KEYS) for r in both)
    assert [{k: r[k] for k in PLAIN_KEYS | set(ALIGNMENT_KEYS)} for r in both] == only


def test_synthesizer_alignment_equals_evaluate_by_emotion(setup):
    from evaluation import ALIGNMENT_KEYS
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    recs = syn.evaluate(rows, 2, 'emotion', alignment=True)
    dec._calls = 0
    outs = syn.alignment([r[1] for r in rows], ratios=[ONE_HOT[r[3]] for r in rows], batch_size=2)
    assert dec._calls == len(rows) and len(outs) == len(rows)
    for i, (o, rec) in enumerate(zip(outs, recs)):
        assert set(o) == set(ALIGNMENT_KEYS) | {'n_frames', 'durations'}
        assert {k: o[k] for k in ALIGNMENT_KEYS} == {k: rec[k] for k in ALIGNMENT_KEYS}, i
        assert o['n_frames'] == rec['n_frames']
        d = o['durations']
        assert isinstance(d, list) and len(d) == o['n_symbols'] and sum(d) == o['n_frames'] and min(d) >= 0
        assert (max(j for j, v in enumerate(d) if v) + 1) / o['n_symbols'] == o['reach']
        assert max(d) >= o['stall_frames'] >= 1
    # one set of ratios for every text, the default batch size, and a reference recording
    dec._calls = 0
    same = [r for r in rows if r[3] == rows[1][3]][:2]                          # EMOS holds label 0 twice
    assert len(same) == 2
    one = syn.alignment([r[1] for r in same], ratios=ONE_HOT[same[0][3]])
    dec._calls = 0
    each = syn.alignment([r[1] for r in same], ratios=[ONE_HOT[r[3]] for r in same])
    assert one == each and all(sum(o['durations']) == o['n_frames'] for o in one)
    dec._calls = 0
    by_ref = syn.alignment([r[1] for r in rows[:2]], True, [r[0] for r in rows[:2]])
    dec._calls = 0
    ref_recs = syn.evaluate(rows[:2], 2, alignment=True)
    assert [{k: o[k] for k in ALIGNMENT_KEYS} for o in by_ref] == [{k: r[k] for k in ALIGNMENT_KEYS} for r in ref_recs]
    with pytest.raises(ValueError):
        syn.alignment(['가'], batch_size=0)
    with pytest.raises(ValueError):
        syn.alignment(['가', '나'], True, ['only_one.wav'])


def test_evaluate_main_alignment(setup, tmp_path, capsys):
    import evaluate
    from evaluation import ALIGNMENT_KEYS
    rows = setup['rows']
    base = ['--load_path', setup['ck'], '--filelist_path', setup['fl'], '--batch_size', '2', '--hparams',
            'max_decoder_steps=%d' % STEPS]
    out = str(tmp_path / 'score.json')
    evaluate.main(base + ['--alignment', '--out', out])
    printed = capsys.readouterr().out
    assert '"read_through_share"' in printed and 'neu: dtw_mean' in printed
    with open(out, encoding='utf-8') as f:
        d = json.load(f)
    assert [x['path'] for x in d['rows']] == [r[0] for r in rows]
    new_stats = {'n_alignment', 'focus_mean', 'reach_mean', 'back_share_mean', 'jump_share_mean', 'uncovered_share_mean',
                 'stall_frames_mean', 'stall_frames_max', 'gap_symbols_mean', 'gap_symbols_max', 'n_read_through',
                 'read_through_share'}
    for x in d['rows']:
        assert set(ALIGNMENT_KEYS) <= set(x) and 0 < x['focus'] <= 1 + 1e-6 and 0 < x['reach'] <= 1 and x['stall_frames'] >= 1
    for stats in [d['summary']['overall']] + list(d['summary']['by_emotion'].values()):
        assert new_stats <= set(stats)
    assert d['summary']['overall']['n_alignment'] == d['summary']['overall']['n_scored']
    plain_out = str(tmp_path / 'plain.json')
    evaluate.main(base + ['--out', plain_out])
    assert 'read_through' not in capsys.readouterr().out
    with open(plain_out, encoding='utf-8') as f:
        p = json.load(f)
    assert all(set(x) == PLAIN_KEYS | {'path'} for x in p['rows'])
    for stats in [p['summary']['overall']] + list(p['summary']['by_emotion'].values()):
        assert not new_stats & set(stats)
    assert [x['n_ref_frames'] for x in p['rows']] == [x['n_ref_frames'] for x in d['rows']]
