"""Synthesizer.evaluate(style=True), Synthesizer.latent_report, latent_report.py and evaluate.py --style on a random-init model
(the setup of tests/test_evaluate_gpu.py: short texts, max_decoder_steps = 24, a gate bias under which some rows stop and some
never do); one row is reported as decoded to a single frame, too short for the reference encoder.

The style fields are checked against tests/latent_ref.py in fp64 on the very mu that model.vae_gst returned during the call (a
spy keeps every call's inputs and outputs), and the spy's inputs are checked to be the mels they should be: the post-net mels
of the same texts, conditioning and decoder seeds, and the mels of the recordings.  own_dist is host fp64 arithmetic on fp32
mu, compared to 1e-12; the silhouette comes from fp32 class sums of at most 8 distances of 32 terms, each within
(32 / 2 + 1 + 8) 2^-24 = 1.5e-6 of its value, which moves s = (b - a) / max(a, b) by at most 2 (1.5e-6 + 1.5e-6) = 6e-6; the
bound is 1e-5.  The vote and the rank are compared where the fp64 distances decide them (the gap rule of
tests/test_latent_gpu.py)."""
import json

import numpy as np
import pytest
import torch

import latent_ref as R
from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
from test_evaluate_gpu import _pick_bias
from test_refenc_ragged_gpu import _write_wavs

pytestmark = pytest.mark.gpu

STEPS = 24
GROUP = 3
TEXTS = [OTHER_TEXTS[1], OTHER_TEXTS[2], "한국어 음성 합성", OTHER_TEXTS[0], "가나다라마바사", "오늘 날씨가 좋네요", "테스트 문장입니다",
         "안녕하세요 반갑습니다", "한국어"]
EMOS = [2, 0, 3, 1, 0, 2, 1, 3]
PLAIN_KEYS = {'dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion'}
SHORT = 4              # the row that _one_short_row cuts to a single frame


def _one_short_row(syn, monkeypatch):
    """evaluate() sees row SHORT of the filelist decoded to one frame, too short for the reference encoder: the frame count
    that `_synthesize_ragged` reports for it is cut to 1 (the decoder itself stops where it stops; which rows a random model
    ends early is not ours to choose)"""
    orig = syn._synthesize_ragged

    def cut(texts, *a, **kw):
        out = list(orig(texts, *a, **kw))
        if TEXTS[SHORT] in texts:
            out[4] = out[4].clone()
            out[4][texts.index(TEXTS[SHORT])] = 1
        return tuple(out)
    monkeypatch.setattr(syn, '_synthesize_ragged', cut)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from synthesizer import Synthesizer
    d = tmp_path_factory.mktemp('style')
    hp, ck, fl = _synth(d, "max_decoder_steps=%d" % STEPS)
    wavs = _write_wavs(d, 8, 13, lo=4000, hi=12000)
    # eight recordings over four labels, and a ninth row that copies recording 2 again (one mu per distinct recording)
    rows = [(w, t, '0', e) for w, t, e in zip(wavs, TEXTS, EMOS)] + [(wavs[2], TEXTS[8], '0', EMOS[2])]
    with open(fl, 'w', encoding='utf-8') as f:
        for r in rows:
            f.write('%s|%s|%s|%d\n' % r)
    syn = Synthesizer(hp).load(ck, filelist_path=fl)
    dec = syn.model.decoder
    dec.gate_threshold, thr = 1.0, dec.gate_threshold
    logits = []
    with torch.no_grad():
        for i0 in range(0, len(rows), GROUP):
            g = rows[i0:i0 + GROUP]
            gate = syn._synthesize_ragged([r[1] for r in g], True, [r[0] for r in g], (1.0, 0.0, 0.0, 0.0))[2]
            assert gate.shape == (len(g), STEPS, 1)
            logits.append(gate[:, :, 0].cpu())
    dec.gate_threshold = thr
    shift, n_want, _ = _pick_bias(torch.cat(logits) - float(np.log(thr / (1 - thr))))
    with torch.no_grad():
        dec.gate_layer.linear_layer.bias -= shift
    torch.save({'iteration': 1, 'state_dict': {k: v.detach().cpu().clone() for k, v in syn.model.state_dict().items()},
                'optimizer': {}, 'learning_rate': 1e-3}, ck)
    dec._calls = 0
    return dict(hp=hp, ck=ck, fl=fl, rows=rows, wavs=wavs, syn=syn, n_want=n_want, dir=d)


def _spy(syn, monkeypatch):
    calls = []
    orig = syn.model.vae_gst.forward

    def forward(inputs, lengths=None):
        out = orig(inputs, lengths)
        calls.append((inputs.detach().clone(), None if lengths is None else [int(v) for v in lengths], out[1].detach().clone()))
        return out
    monkeypatch.setattr(syn.model.vae_gst, 'forward', forward)
    return calls


def test_style_fields_equal_the_reference(setup, monkeypatch):
    from evaluation import STYLE_KEYS, StyleRecords, summarize
    from latent_scores import silhouette
    syn, rows, wavs = setup['syn'], setup['rows'], setup['wavs']
    dec = syn.model.decoder
    _one_short_row(syn, monkeypatch)
    n_want = [1 if i == SHORT else n for i, n in enumerate(setup['n_want'])]
    dec._calls = 0
    plain = syn.evaluate(rows, GROUP)
    assert type(plain) is list and all(set(r) == PLAIN_KEYS for r in plain)
    assert [r['n_frames'] for r in plain] == n_want
    calls = _spy(syn, monkeypatch)
    dec._calls = 0
    recs = syn.evaluate(rows, GROUP, style=True)
    calls = list(calls)                                                          # (the spy stays on: keep what evaluate() made)
    assert dec._calls == len(rows)
    assert isinstance(recs, StyleRecords) and all(set(r) == PLAIN_KEYS | set(STYLE_KEYS) for r in recs)
    assert [{k: r[k] for k in PLAIN_KEYS} for r in recs] == plain                # the same seeds, the same scores, to the bit
    # walk the vae_gst calls: per group the conditioning, the recordings not seen before, the synthesised rows it can take
    n_all = [r['n_frames'] for r in recs]
    rec_mu, syn_mu, seen, at = {}, {}, [], 0
    for i0 in range(0, len(rows), GROUP):
        g = rows[i0:i0 + GROUP]
        uniq = list(dict.fromkeys(r[0] for r in g))
        assert calls[at][0].size(0) == len(uniq)
        at += 1
        new = [p for p in uniq if p not in seen]
        if new:
            inputs, lengths, mu = calls[at]
            at += 1
            want, n = syn.load_mels(new)
            assert lengths == n
            for j, p in enumerate(new):
                assert torch.allclose(inputs[j, :, :n[j]], want[j, :, :n[j]], rtol=0, atol=1e-5)
                rec_mu[p] = mu[j].float().cpu().numpy()
            seen += new
        can = [b for b in range(len(g)) if n_all[i0 + b] >= 2]
        if can:
            inputs, lengths, mu = calls[at]
            at += 1
            assert lengths == [n_all[i0 + b] for b in can]
            dec._calls = i0                                                     # the seeds evaluate() gave this group
            post = syn._synthesize_ragged([r[1] for r in g], True, [r[0] for r in g], (1.0, 0.0, 0.0, 0.0))[1]
            dec._calls = len(rows)
            for j, b in enumerate(can):
                assert torch.equal(inputs[j, :, :lengths[j]], post[b, :, :lengths[j]])
                syn_mu[i0 + b] = mu[j].float().cpu().numpy()
    monkeypatch.undo()
    assert at == len(calls) and seen == wavs and sorted(syn_mu) == [i for i in range(len(rows)) if i != SHORT]
    # the reference, in fp64, on those mu
    refs, labels = np.stack([rec_mu[p] for p in wavs]), np.array(EMOS)
    have = sorted(syn_mu)
    own = np.array([wavs.index(rows[i][0]) for i in have])
    ref = R.neighbours(refs, labels, np.stack([syn_mu[i] for i in have]), k=5, n_classes=4, exclude=own, target=own)
    vote = R.knn_vote(ref.idx, labels, 4)
    sil = silhouette(ref.class_sum, ref.class_cnt, np.array([rows[i][3] for i in have]))
    voted = R.decided(ref.d2, own, 5)
    ranked = R.rank_decided(ref.d2, own)
    print("style: %d rows with fields, vote decided for %d, rank for %d; ranks %s" % (len(have), voted.sum(), ranked.sum(),
                                                                                     ref.rank.tolist()))
    for j, i in enumerate(have):
        r = recs[i]
        if voted[j]:
            assert r['style_emotion'] == vote[j] and r['style_hit'] == bool(vote[j] == rows[i][3])
        if ranked[j]:
            assert r['style_own_rank'] == ref.rank[j]
        want = float(np.sqrt(ref.d2[j, own[j]]))
        assert abs(r['style_own_dist'] - want) <= 1e-12 * max(want, 1.0)
        assert abs(r['style_silhouette'] - sil[j]) <= 1e-5
        assert type(r['style_emotion']) is int and type(r['style_hit']) is bool and type(r['style_own_rank']) is int
    for i in range(len(rows)):
        if i not in syn_mu:
            assert n_all[i] < 2 and all(recs[i][k] is None for k in STYLE_KEYS)
    # what the recordings say about themselves, and the summary
    loo = R.neighbours(refs, labels, k=5, n_classes=4)
    assert recs.style_info['k'] == 5 and recs.style_info['n_recordings'] == 8
    if R.decided(loo.d2, np.arange(8), 5).all():
        assert recs.style_info['ref_accuracy'] == pytest.approx((R.knn_vote(loo.idx, labels, 4) == labels).mean())
    s = summarize(recs)
    assert s['style']['overall']['n_style'] == len(have) and s['style']['ref_accuracy'] == recs.style_info['ref_accuracy']
    assert {k: s[k] for k in ('overall', 'by_emotion')} == summarize(plain)
    assert np.array(s['style']['confusion']).sum() == len(have)
    assert json.loads(json.dumps({'summary': s, 'rows': list(recs)}))['rows'][0]['style_own_rank'] == recs[0]['style_own_rank']


def test_style_refusals_and_a_lowered_k(setup):
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    dec._calls = 0
    with pytest.raises(ValueError, match="labels"):
        syn.evaluate(rows[:3] + [(rows[0][0], rows[0][1], '0', (rows[0][3] + 1) % 4)], GROUP, style=True)
    with pytest.raises(ValueError, match="2 distinct recordings"):
        syn.evaluate([rows[2], rows[8]], GROUP, style=True)                     # two rows, one recording
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="style_k"):
            syn.evaluate(rows, GROUP, style=True, style_k=bad)
    assert dec._calls == 0                                                      # refused before anything is decoded
    few = syn.evaluate(rows[1:4], GROUP, 'emotion', style=True, style_k=5)       # 3 recordings: 2 neighbours at most
    assert few.style_info == dict(few.style_info, k=2, n_recordings=3)
    dec._calls = 0
    two = syn.evaluate(rows[1:4], GROUP, 'emotion', style=True, style_k=2)
    assert list(two) == list(few) and two.style_info == few.style_info
    dec._calls = 0


def test_latent_report_and_the_command_agree(setup, capsys):
    import latent_report
    from evaluation import EMOTIONS
    syn, wavs, d = setup['syn'], setup['wavs'], setup['dir']
    rep = syn.latent_report(wavs, EMOS, k=3, batch_size=4)
    assert rep['n'] == 8 and rep['k'] == 3 and set(rep['by_emotion']) == set(EMOTIONS) and len(rep['kl_per_dim']) == 32
    assert 0 <= rep['knn_accuracy'] <= 1 and 0 <= rep['active_units'] <= 32 and np.array(rep['confusion']).sum() == 8
    prosody, mu, logvar, z = (t.cpu().numpy() for t in syn.latents(wavs, 4))
    src, out = str(d / 'lat.npz'), str(d / 'rep.json')
    np.savez(src, prosody=prosody, mus=mu, logvars=logvar, zs=z, emotions=np.array(EMOS), paths=np.array(wavs))
    capsys.readouterr()
    latent_report.main(['--latents', src, '--k', '3', '--out', out])
    printed = capsys.readouterr().out.strip().split('\n')
    assert len(printed) == 4 and printed[0].startswith('8 utterances, k = 3')
    with open(out, encoding='utf-8') as f:
        assert json.load(f) == rep
    # the scores against the fp64 reference on the same mu
    ref = R.neighbours(mu, np.array(EMOS), k=3, n_classes=4)
    if R.decided(ref.d2, np.arange(8), 3).all():
        assert rep['knn_accuracy'] == pytest.approx((R.knn_vote(ref.idx, np.array(EMOS), 4) == np.array(EMOS)).mean())
    assert rep['silhouette_mean'] == pytest.approx(np.nanmean(R.silhouette_direct(mu, np.array(EMOS))), abs=1e-5)
    with pytest.raises(ValueError, match="key"):
        syn.latent_report(wavs, EMOS, key='prosody')
    with pytest.raises(ValueError, match="paths"):
        syn.latent_report(wavs, EMOS[:7])
    zs = syn.latent_report(wavs, EMOS, key='zs', k=3, batch_size=4)              # eval mode: z = mu
    assert zs == rep


def test_evaluate_main_style(setup, tmp_path, capsys):
    import evaluate
    from evaluation import STYLE_KEYS
    base = ['--load_path', setup['ck'], '--filelist_path', setup['fl'], '--batch_size', str(GROUP), '--limit', '6', '--hparams',
            'max_decoder_steps=%d' % STEPS]
    out = str(tmp_path / 'score.json')
    evaluate.main(base + ['--style', '--style_k', '3', '--alignment', '--out', out])
    printed = capsys.readouterr().out
    assert 'style: accuracy' in printed and '"ref_accuracy"' in printed
    with open(out, encoding='utf-8') as f:
        d = json.load(f)
    assert d['summary']['style']['k'] == 3 and d['summary']['style']['n_recordings'] == 6
    assert all(set(STYLE_KEYS) <= set(x) and 'n_symbols' in x for x in d['rows'])
    got = [x['n_frames'] for x in d['rows']]
    assert got == setup['n_want'][:6]
    assert all(x['style_emotion'] in (0, 1, 2, 3) and x['style_own_rank'] >= 0 for x in d['rows'])
    plain_out = str(tmp_path / 'plain.json')
    evaluate.main(base + ['--out', plain_out])
    printed = capsys.readouterr().out
    assert 'style: accuracy' not in printed and '"style"' not in printed
    with open(plain_out, encoding='utf-8') as f:
        p = json.load(f)
    assert 'style' not in p['summary'] and all(set(x) == PLAIN_KEYS | {'path'} for x in p['rows'])
    assert [x['dtw'] for x in p['rows']] == [x['dtw'] for x in d['rows']]
