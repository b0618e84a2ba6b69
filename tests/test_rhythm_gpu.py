"""Rhythm control end to end on a random-init model: Synthesizer.synthesize / synthesize_batch with durations=,
rhythm_from= and rhythm_scale=, evaluate(rhythm='ref') and the two command lines.  Under rhythm_window = (0, 0) every frame reads
exactly its planned symbol, so the alignments give the durations back whatever the weights are."""
import json
import os

import numpy as np
import pytest
import torch

from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
from test_refenc_ragged_gpu import _write_wavs

pytestmark = pytest.mark.gpu

TEXTS = [OTHER_TEXTS[0], OTHER_TEXTS[1], OTHER_TEXTS[2]]
PLAIN_KEYS = {'dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion'}


def _lens(texts):
    from text import text_to_sequence
    return [len(text_to_sequence(t, ['korean_cleaners'])) for t in texts]


@pytest.fixture()
def setup(tmp_path):
    from synthesizer import Synthesizer
    lens = _lens(TEXTS)
    steps = 4 * max(lens) + 8                                          # durations of 1 or 2 frames, doubled, fit
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=%d" % steps, gate_bias=1e3)      # a gate that fires at once: the plan decides
    syn = Synthesizer(hp).load(ck, filelist_path=fl)
    rng = np.random.RandomState(3)
    D = [rng.randint(1, 3, L).tolist() for L in lens]
    return dict(syn=syn, hp=hp, ck=ck, fl=fl, lens=lens, D=D, steps=steps, tmp=tmp_path)


def _counts(al, L):
    return torch.bincount(al[0].argmax(1).cpu(), minlength=L).tolist()


def test_synthesize_batch_follows_the_durations(setup):
    import t2v_hip
    syn, D, lens = setup['syn'], setup['D'], setup['lens']
    out = syn.synthesize_batch(TEXTS, durations=D, rhythm_window=(0, 0))
    for b, (mel, al) in enumerate(out):
        n = sum(D[b])
        assert mel.shape == (1, 80, n) and al.shape == (1, n, lens[b]), b
        assert _counts(al, lens[b]) == D[b], b                          # bincount(argmax(align)) is the plan
        assert torch.equal(al[0].cpu(), torch.nn.functional.one_hot(al[0].argmax(1).cpu(), lens[b]).float())
        r = t2v_hip.mas(al.contiguous(), [n], [lens[b]], 1)             # and the forced alignment of the result gives it back
        assert r.durations[0].tolist() == D[b], b
    # one text alone, through synthesize(): the same frames
    mel, al = syn.synthesize(TEXTS[0], durations=D[0], rhythm_window=(0, 0))
    assert mel.shape == (1, 80, sum(D[0])) and _counts(al, lens[0]) == D[0]
    # a scale doubles every count; per symbol: only the symbols it names
    for b, (mel, al) in enumerate(syn.synthesize_batch(TEXTS, durations=D, rhythm_scale=2.0, rhythm_window=(0, 0))):
        assert _counts(al, lens[b]) == [2 * d for d in D[b]] and mel.size(2) == 2 * sum(D[b])
    scale = [[3.0 if j == 1 else 1.0 for j in range(L)] for L in lens]
    for b, (mel, al) in enumerate(syn.synthesize_batch(TEXTS, durations=D, rhythm_scale=scale, rhythm_window=(0, 0))):
        assert _counts(al, lens[b]) == [d * (3 if j == 1 else 1) for j, d in enumerate(D[b])]
    # fractions: 0.5 frames per symbol gives every second symbol a frame (ties round up: ends 0.5, 1.0, 1.5, ... -> 1, 1, 2, 2, ...)
    mel, al = syn.synthesize(TEXTS[1], durations=[0.5] * lens[1], rhythm_window=(0, 0))
    assert _counts(al, lens[1]) == [1 if j % 2 == 0 else 0 for j in range(lens[1])]
    # the default window reads around the plan: the argmax stays within one symbol of it, and the length is the plan's
    mel, al = syn.synthesize(TEXTS[1], durations=D[1])
    plan = np.repeat(np.arange(lens[1]), D[1])
    assert mel.size(2) == sum(D[1]) and (al[0].argmax(1).cpu().numpy() - plan).__abs__().max() <= 1
    t2v_hip.check_async_errors()


def test_arguments_are_refused_with_a_reason(setup):
    syn, D, lens = setup['syn'], setup['D'], setup['lens']
    with pytest.raises(ValueError, match="text 1 has %d symbols" % lens[1]):
        syn.synthesize_batch(TEXTS, durations=[D[0], D[1][:-1], D[2]])
    with pytest.raises(ValueError):
        syn.synthesize_batch(TEXTS, durations=D[:2])
    with pytest.raises(ValueError, match="not both"):
        syn.synthesize_batch(TEXTS, durations=D, rhythm_from=['a.wav'] * 3)
    with pytest.raises(ValueError):
        syn.synthesize_batch(TEXTS, rhythm_scale=2.0)                   # a scale without a plan
    with pytest.raises(ValueError):
        syn.synthesize(TEXTS[0], rhythm_window=(0, 0))
    with pytest.raises(ValueError, match="row 1"):
        syn.synthesize_batch(TEXTS, durations=[D[0], [-1.0] * lens[1], D[2]])
    with pytest.raises(ValueError, match="text 2 gets no frame"):
        syn.synthesize_batch(TEXTS, durations=[D[0], D[1], [0.0] * lens[2]])
    with pytest.raises(ValueError):
        syn.synthesize_batch(TEXTS, durations=D, rhythm_window=(1,))
    # without the new arguments the call is the parent's: the gate (bias 1e3) ends every text on its first frame
    assert [m.size(2) for m, _ in syn.synthesize_batch(TEXTS)] == [1, 1, 1]


def test_rhythm_from_a_recording_and_evaluate(setup):
    import t2v_hip
    from evaluation import DURATION_KEYS
    syn, lens, tmp = setup['syn'], setup['lens'], setup['tmp']
    # frames >= symbols, and twice the frames <= max_decoder_steps (a longer plan is cut there)
    wavs = _write_wavs(tmp, 3, 17, lo=max(lens) * 256 + 2048, hi=(setup['steps'] // 2 - 2) * 256)
    rows = [(w, t, '0', e) for w, t, e in zip(wavs, TEXTS, (0, 2, 1))]
    want = syn.durations(rows)
    assert all(r['durations'] is not None and min(r['durations']) >= 1 for r in want)
    calls = syn.model.decoder._calls
    out = syn.synthesize_batch(TEXTS, rhythm_from=wavs, rhythm_window=(0, 0))
    assert syn.model.decoder._calls == calls + 3                       # the forced alignments took no decoder seed
    for b, (mel, al) in enumerate(out):
        assert mel.size(2) == want[b]['n_frames'] and _counts(al, lens[b]) == want[b]['durations'], b
    mel, al = syn.synthesize(TEXTS[2], rhythm_from=wavs[2], rhythm_scale=2.0, rhythm_window=(0, 0))
    assert _counts(al, lens[2]) == [2 * d for d in want[2]['durations']]
    # a recording too short for its text has no path: refused, naming the text
    short = _write_wavs(tmp, 1, 18, lo=600, hi=700)[0]
    with pytest.raises(ValueError, match="text 1 has %d symbols" % lens[1]):
        syn.synthesize_batch(TEXTS[:2], rhythm_from=[wavs[0], short])
    # evaluate: every synthesis with the rhythm of its own recording
    recs = syn.evaluate(rows, 2, rhythm='ref', rhythm_window=(0, 0), durations=True)
    assert all(set(r) == PLAIN_KEYS | set(DURATION_KEYS) | {'rhythm'} and r['rhythm'] == 'ref' for r in recs)
    for r, w in zip(recs, want):
        assert r['n_frames'] == r['n_ref_frames'] == w['n_frames'] and not r['hit_max']
        assert r['dur_rmse_frames'] == 0.0 and r['dur_log_ratio_spread'] == 0.0       # rhythm is out of the comparison
    soft = syn.evaluate(rows, 2, rhythm='ref', durations=True)          # the default window: the length is still the recording's
    assert [r['n_frames'] for r in soft] == [w['n_frames'] for w in want] and all(r['rhythm'] == 'ref' for r in soft)
    plain = syn.evaluate(rows, 2, durations=True)
    assert all(set(r) == PLAIN_KEYS | set(DURATION_KEYS) for r in plain)              # without the argument: the parent's keys
    assert [r['n_frames'] for r in plain] == [1, 1, 1]
    with pytest.raises(ValueError):
        syn.evaluate(rows, 2, rhythm='text')
    with pytest.raises(ValueError):
        syn.evaluate(rows, 2, rhythm_window=(0, 0))
    t2v_hip.check_async_errors()


def test_command_lines(setup, capsys):
    import evaluate as E
    import synthesizer as S
    tmp, lens, D = setup['tmp'], setup['lens'], setup['D']
    wavs = _write_wavs(tmp, 2, 19, lo=max(lens[0], lens[2]) * 256 + 2048, hi=40 * 256)
    fl = str(tmp / 'rows.txt')
    with open(fl, 'w', encoding='utf-8') as f:
        for w, t in zip(wavs, (TEXTS[0], TEXTS[2])):
            f.write('%s|%s|0|0\n' % (w, t))
    base = ['--load_path', setup['ck'], '--filelist_path', fl, '--hparams', 'max_decoder_steps=%d' % setup['steps']]
    keys = {}
    for name, extra in (('plain', []), ('rhythm', ['--rhythm', 'ref', '--rhythm_window', '0,0'])):
        out = str(tmp / (name + '.json'))
        E.main(base + ['--out', out] + extra)
        keys[name] = json.load(open(out))
    assert set(keys['rhythm']) == set(keys['plain']) | {'rhythm', 'rhythm_window'}
    assert keys['rhythm']['rhythm'] == 'ref' and keys['rhythm']['rhythm_window'] == [0, 0]
    assert all('rhythm' not in r for r in keys['plain']['rows']) and all(r['rhythm'] == 'ref' for r in keys['rhythm']['rows'])
    assert [r['n_frames'] for r in keys['rhythm']['rows']] == [r['n_ref_frames'] for r in keys['rhythm']['rows']]
    # synthesizer.py --durations FILE.npz (what extract_durations.py writes) and --rhythm_scale
    npz = str(tmp / 'd.npz')
    offsets = np.cumsum([0, lens[0], lens[2]]).astype(np.int64)
    np.savez(npz, offsets=offsets, durations=np.array(D[0] + D[2], dtype=np.int32))
    S.main(['--load_path', setup['ck'], '--filelist_path', setup['fl'], '--sample_path', str(tmp / 's'), '--text', TEXTS[0],
            '--text', TEXTS[2], '--durations', npz, '--rhythm_scale', '2', '--rhythm_window', '0,0',
            '--hparams', 'max_decoder_steps=%d' % setup['steps']])
    for i, b in enumerate((0, 2)):
        assert np.load(str(tmp / 's' / ('%d.npy' % i))).shape == (80, 2 * sum(D[b]))
    capsys.readouterr()
