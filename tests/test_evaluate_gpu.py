"""Synthesizer.evaluate and the evaluate.py command on a random-init model: the records equal the manual composition
synthesize_batch + load_mels + fp64 numpy DTW, rows that run to max_decoder_steps are reported, scored and counted apart."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
from test_evaluate import dtw_ref
from test_refenc_ragged_gpu import _write_wavs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tacotron2-vae_amd')
STEPS = 24
TEXTS = [OTHER_TEXTS[1], OTHER_TEXTS[2], "한국어 음성 합성", OTHER_TEXTS[0], "가나다라마바사"]
EMOS = [2, 0, 3, 1, 0]


def _tol(ref, tx, ty):
    return ref * (tx + ty + 128) * 2.0 ** -23           # the kernel's bound (tests/test_dtw_gpu.py)


def _pick_bias(logits):
    """a gate bias shift under which some rows stop (after frame 2) and some never do, every logit as far from the
    threshold as the logits allow; returns (shift, expected frame counts, expected hit_max)"""
    vals = torch.sort(logits.reshape(-1)).values
    best = None
    for i in range(len(vals) - 1):
        c, margin = float(vals[i] + vals[i + 1]) / 2, float(vals[i + 1] - vals[i]) / 2
        n, hit = [], []
        for lg in logits:
            f = (lg > c).nonzero()
            n.append(int(f[0]) + 1 if len(f) else len(lg))
            hit.append(len(f) == 0)
        if any(hit) and not all(hit) and min(n) >= 2 and (best is None or margin > best[0]):
            best = (margin, c, n, hit)
    assert best is not None and best[0] > 1e-4, "no gate bias separates the rows"
    return best[1:]


@pytest.fixture()
def setup(tmp_path):
    from synthesizer import Synthesizer
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=%d" % STEPS)
    wavs = _write_wavs(tmp_path, len(TEXTS), 11, lo=4000, hi=14000)
    rows = [(w, t, '0', e) for w, t, e in zip(wavs, TEXTS, EMOS)]
    with open(fl, 'w', encoding='utf-8') as f:
        for r in rows:
            f.write('%s|%s|%s|%d\n' % r)
    syn = Synthesizer(hp).load(ck, filelist_path=fl)
    dec = syn.model.decoder
    # all gate logits of every row, decoded exactly as evaluate(batch_size=2) will decode them (same groups, same seeds)
    dec.gate_threshold, thr = 1.0, dec.gate_threshold
    logits = []
    with torch.no_grad():
        for i0 in range(0, len(rows), 2):
            g = rows[i0:i0 + 2]
            gate = syn._synthesize_ragged([r[1] for r in g], True, [r[0] for r in g], (1.0, 0.0, 0.0, 0.0))[2]
            assert gate.shape == (len(g), STEPS, 1)
            logits.append(gate[:, :, 0].cpu())
    dec.gate_threshold = thr
    shift, n_want, hit_want = _pick_bias(torch.cat(logits) - float(np.log(thr / (1 - thr))))
    with torch.no_grad():
        dec.gate_layer.linear_layer.bias -= shift
    torch.save({'iteration': 1, 'state_dict': {k: v.detach().cpu().clone() for k, v in syn.model.state_dict().items()},
                'optimizer': {}, 'learning_rate': 1e-3}, ck)
    dec._calls = 0
    return dict(hp=hp, ck=ck, fl=fl, rows=rows, syn=syn, n_want=n_want, hit_want=hit_want)


def test_evaluate_equals_the_manual_composition(setup):
    from evaluation import summarize
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    recs = syn.evaluate(rows, batch_size=2)
    assert dec._calls == len(rows)                      # as len(rows) synthesize() calls leave it
    assert [r['n_frames'] for r in recs] == setup['n_want']
    assert [r['hit_max'] for r in recs] == setup['hit_want']
    assert [r['emotion'] for r in recs] == EMOS
    dec._calls = 0
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        outs = syn.synthesize_batch([r[1] for r in g], None, True, [r[0] for r in g])
        truth, n_ref = syn.load_mels([r[0] for r in g])
        for b, (post, _) in enumerate(outs):
            rec = recs[i0 + b]
            assert rec['n_frames'] == post.size(2) and rec['n_ref_frames'] == n_ref[b]
            want = dtw_ref(post[0].cpu().numpy(), truth[b, :, :n_ref[b]].cpu().numpy())
            print("row %d: %d x %d frames, dtw %.9g ref %.9g hit_max %s" % (i0 + b, post.size(2), n_ref[b], rec['dtw'], want,
                                                                          rec['hit_max']))
            assert abs(rec['dtw'] - want) <= _tol(want, post.size(2), n_ref[b]), (i0 + b, rec['dtw'], want)
    assert dec._calls == len(rows)
    # rows that ran to max_decoder_steps: reported, scored all the same, and counted apart in the summary
    hit = [r for r in recs if r['hit_max']]
    assert hit and len(hit) < len(recs)
    assert all(r['n_frames'] == STEPS and np.isfinite(r['dtw']) and r['dtw'] > 0 for r in hit)
    s = summarize(recs)['overall']
    assert s['n_rows'] == len(recs) and s['n_hit_max'] == len(hit) and s['n_scored'] == len(recs) - len(hit)
    assert s['dtw_mean'] == pytest.approx(np.mean([r['dtw'] for r in recs if not r['hit_max']]))


def test_evaluate_by_emotion_needs_the_centroids(setup):
    from synthesizer import Synthesizer
    syn, rows = setup['syn'], setup['rows']
    bare = Synthesizer(setup['hp']).load_checkpoint(setup['ck'])
    with pytest.raises(RuntimeError, match="centroids"):
        bare.evaluate(rows, 2, 'emotion')
    with pytest.raises(ValueError):
        syn.evaluate(rows, 2, 'style')
    with pytest.raises(ValueError):
        syn.evaluate(rows, 0)
    dec = syn.model.decoder
    dec._calls = 0
    recs = syn.evaluate(rows, 3, 'emotion')
    assert dec._calls == len(rows) and len(recs) == len(rows)
    dec._calls = 0
    ratios = {0: (1, 0, 0, 0), 1: (0, 1, 0, 0), 2: (0, 0, 0, 1), 3: (0, 0, 1, 0)}          # (neu, sad, hap, ang) of label ids
    for i0 in range(0, len(rows), 3):
        g = rows[i0:i0 + 3]
        outs = syn.synthesize_batch([r[1] for r in g], None, False, None, [ratios[r[3]] for r in g])
        truth, n_ref = syn.load_mels([r[0] for r in g])
        for b, (post, _) in enumerate(outs):
            rec = recs[i0 + b]
            assert rec['n_frames'] == post.size(2) and rec['n_ref_frames'] == n_ref[b] and rec['emotion'] == g[b][3]
            want = dtw_ref(post[0].cpu().numpy(), truth[b, :, :n_ref[b]].cpu().numpy())
            assert abs(rec['dtw'] - want) <= _tol(want, post.size(2), n_ref[b]), (i0 + b, rec['dtw'], want)


def test_evaluate_cli_writes_rows_in_filelist_order(setup, tmp_path):
    syn, rows = setup['syn'], setup['rows']
    recs = syn.evaluate(rows, 2)
    base = [sys.executable, os.path.join(PKG, 'evaluate.py'), '--load_path', setup['ck'], '--filelist_path', setup['fl'],
            '--batch_size', '2', '--hparams', 'max_decoder_steps=%d' % STEPS]
    out = str(tmp_path / 'score.json')
    r = subprocess.run(base + ['--out', out], capture_output=True, text=True, timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out, encoding='utf-8') as f:
        d = json.load(f)
    assert [x['path'] for x in d['rows']] == [r_[0] for r_ in rows]
    # The numbers are checked in-process above.  Across processes only what cannot depend on a process-wide numeric mode left by
    # earlier tests of a long run (the fp32 GEMM modes move a mel by ~1e-3): the rows, their reference lengths, finite scores.
    assert [x['n_ref_frames'] for x in d['rows']] == [x['n_ref_frames'] for x in recs]
    assert [x['emotion'] for x in d['rows']] == EMOS
    assert all(np.isfinite(x['dtw']) and x['dtw'] > 0 and 1 <= x['n_frames'] <= STEPS for x in d['rows'])
    assert d['summary']['overall']['n_rows'] == len(rows)
    assert d['summary']['overall']['n_hit_max'] == sum(x['hit_max'] for x in d['rows'])
    assert '"n_hit_max"' in r.stdout
    out3 = str(tmp_path / 'score3.json')
    r = subprocess.run(base + ['--out', out3, '--limit', '3', '--condition', 'emotion'], capture_output=True, text=True,
                       timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out3, encoding='utf-8') as f:
        d3 = json.load(f)
    assert [x['path'] for x in d3['rows']] == [r_[0] for r_ in rows[:3]]
    assert d3['summary']['overall']['n_rows'] == 3
