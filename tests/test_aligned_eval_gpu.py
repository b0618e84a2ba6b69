"""Synthesizer.evaluate(aligned=True) and evaluate.py --aligned on a random-init model and written harmonic recordings
(test_prosody_gpu's setup): the records equal the composition by hand of mel_cepstrum, f0, aligned_scores and aligned_fields;
alone the flag needs no vocoder and leaves the F0 values None; and no other key moves."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_evaluate_gpu import STEPS
from test_prosody_gpu import PLAIN_KEYS, PKG, _same, setup  # noqa: F401  (setup is the fixture)

pytestmark = pytest.mark.gpu

F0_KEYS = ('vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_bias_cents', 'lf0_corr')


def test_evaluate_aligned_equals_the_manual_composition(setup):  # noqa: F811
    import t2v_hip
    from evaluation import ALIGNED_KEYS, PROSODY_KEYS, aligned_fields, summarize
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    np.random.seed(7)
    recs = syn.evaluate(rows, 2, prosody=True, aligned=True)
    assert dec._calls == len(rows)
    assert [r['n_frames'] for r in recs] == setup['n_want'] and [r['hit_max'] for r in recs] == setup['hit_want']
    assert all(set(r) == PLAIN_KEYS | set(PROSODY_KEYS) | set(ALIGNED_KEYS) for r in recs)
    np.random.seed(7)
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        texts, paths = [r[1] for r in g], [r[0] for r in g]
        dec._calls = i0
        with torch.no_grad():
            mel, mel_postnet, _, _, n_frames, _ = syn._synthesize_ragged(texts, True, paths, (1.0, 0.0, 0.0, 0.0))
        n = n_frames.tolist()
        can = [b for b in range(len(g)) if n[b] >= 4]          # the vocoder needs 4 frames
        wavs = syn.vocoder.batch(mel[can], [n[b] for b in can]) if can else []
        y_ref, n_samples = syn.load_wavs(paths)
        truth, n_ref = syn.load_mels(paths)
        f0y = t2v_hip.f0(y_ref, n_samples)
        assert f0y.size(1) >= max(n_ref)
        f0x = torch.zeros(len(g), max(n), device=mel.device)
        for k, b in enumerate(can):
            trk = t2v_hip.f0(wavs[k][None].contiguous(), [wavs[k].numel()])[0]
            assert trk.numel() == n[b]                          # (n - 1) * 256 samples: one pitch frame per mel frame
            f0x[b, :n[b]] = trk
        r = t2v_hip.aligned_scores(t2v_hip.mel_cepstrum(mel_postnet, n), n, t2v_hip.mel_cepstrum(truth, n_ref), n_ref, f0x, f0y)
        counts, sums = r.counts.cpu().tolist(), r.sums.cpu().tolist()
        for b in range(len(g)):
            rec = recs[i0 + b]
            want = aligned_fields(counts[b], sums[b], f0=b in can)
            print("row %d: %d x %d frames, K %d, %s" % (i0 + b, n[b], n_ref[b], counts[b][0], {k: rec[k] for k in ALIGNED_KEYS}))
            for k in ALIGNED_KEYS:
                assert _same(rec[k], want[k]), (i0 + b, k, rec[k], want[k])
            assert max(n[b], n_ref[b]) <= counts[b][0] <= n[b] + n_ref[b] - 1
            assert rec['mcd_db'] > 0 and np.isfinite(rec['mcd_db']) and 0 <= rec['warp_dev'] <= 1
            if b in can:
                assert rec['vde'] is not None and 0 <= rec['vde'] <= rec['ffe'] <= 1
            else:
                assert all(rec[k] is None for k in F0_KEYS)
    s = summarize(recs)
    stopped = [r for r in recs if not r['hit_max']]
    o = s['overall']
    assert o['n_aligned'] == len(stopped) == o['n_scored']
    assert o['mcd_db_mean'] == pytest.approx(np.mean([r['mcd_db'] for r in stopped]))
    have = [r['vde'] for r in stopped if r['vde'] is not None]
    assert o['vde_mean'] == (pytest.approx(np.mean(have)) if have else None)
    assert sum(e['n_aligned'] for e in s['by_emotion'].values()) == o['n_aligned']


def test_aligned_alone_needs_no_vocoder_and_moves_no_other_key(setup):  # noqa: F811
    from evaluation import ALIGNED_KEYS
    from synthesizer import Synthesizer
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    np.random.seed(11)
    before = np.random.get_state()
    plain = syn.evaluate(rows, 2)
    assert all(set(r) == PLAIN_KEYS for r in plain)                             # without the flag: the keys of before
    dec._calls = 0
    recs = syn.evaluate(rows, 2, aligned=True)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]       # no draw
    assert dec._calls == len(rows)                                              # the same decoder seeds
    assert all(set(r) == PLAIN_KEYS | set(ALIGNED_KEYS) for r in recs)
    assert [{k: r[k] for k in PLAIN_KEYS} for r in recs] == plain               # every earlier key, dtw to the bit
    for r in recs:
        assert r['mcd_db'] > 0 and 0 <= r['warp_dev'] <= 1 and all(r[k] is None for k in F0_KEYS)
    # with the pitch tracks the path is the same one: mcd_db and warp_dev keep their bits, the other keys theirs
    dec._calls = 0
    both = syn.evaluate(rows, 2, prosody=True, aligned=True)
    dec._calls = 0
    np.random.set_state(after)
    pros = syn.evaluate(rows, 2, prosody=True)
    assert [(r['mcd_db'], r['warp_dev']) for r in both] == [(r['mcd_db'], r['warp_dev']) for r in recs]
    assert [{k: v for k, v in r.items() if k not in ALIGNED_KEYS} for r in both] == pros
    # no vocoder at all
    bare = Synthesizer(setup['hp']).load_checkpoint(setup['ck'])
    assert bare.vocoder is None or not hasattr(bare.vocoder, 'batch')
    alone = bare.evaluate(rows, 2, aligned=True)
    assert [r['n_frames'] for r in alone] == setup['n_want']
    assert all(r['mcd_db'] > 0 and 0 <= r['warp_dev'] <= 1 and all(r[k] is None for k in F0_KEYS) for r in alone)
    with pytest.raises(RuntimeError, match="Griffin-Lim"):
        bare.evaluate(rows, 2, prosody=True, aligned=True)


def test_evaluate_cli_aligned(setup, tmp_path):  # noqa: F811
    from evaluation import ALIGNED_KEYS
    rows = setup['rows']
    out = str(tmp_path / 'score.json')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py'), '--load_path', setup['ck'], '--filelist_path', setup['fl'],
                        '--batch_size', '2', '--hparams', 'max_decoder_steps=%d' % STEPS, '--aligned', '--out', out],
                       capture_output=True, text=True, timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out, encoding='utf-8') as f:
        d = json.load(f)
    assert [x['path'] for x in d['rows']] == [r_[0] for r_ in rows]
    for x in d['rows']:
        assert set(ALIGNED_KEYS) <= set(x)
        assert x['mcd_db'] > 0 and 0 <= x['warp_dev'] <= 1 and x['vde'] is None and x['lf0_corr'] is None
    for stats in [d['summary']['overall']] + list(d['summary']['by_emotion'].values()):
        assert {'n_aligned', 'mcd_db_mean', 'vde_mean', 'gpe_mean', 'ffe_mean', 'lf0_rmse_cents_mean', 'lf0_corr_mean',
                'warp_dev_mean'} <= set(stats)
    assert d['summary']['overall']['n_rows'] == len(rows)
    assert d['summary']['overall']['n_aligned'] == d['summary']['overall']['n_scored']
    assert '"n_aligned"' in r.stdout and 'mcd_db_mean' in r.stdout and 'warp_dev_mean' in r.stdout
