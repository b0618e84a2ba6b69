"""Synthesizer.evaluate under every combination of its five optional scores (alignment, prosody, style, aligned, energy), on
test_energy_eval_gpu's setup (five harmonic recordings, 32 decoder steps, the Griffin-Lim vocoder, groups of 2) with one row
reported as decoded to 1 frame and one to 3 frames: at 3 frames the reference encoder takes a row (2 or more) and the vocoder
does not (4 or more), at 1 frame neither does, so the two sets of rows differ.

Every combination must give each score the values that the score gives alone (or, where two scores feed a third, together
with the score it shares with), to the bit: the same decoder seeds, the same np.random draws, no key more and none less."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import yin_ref
from test_batch_synthesis_gpu import _synth
from test_energy_eval_gpu import SAMPLES, STEPS
from test_evaluate_gpu import EMOS, TEXTS, _pick_bias
from test_prosody_gpu import FREQS, PLAIN_KEYS

pytestmark = pytest.mark.gpu

FLAGS = ('alignment', 'prosody', 'style', 'aligned', 'energy')
SUBSETS = [frozenset(c) for k in range(len(FLAGS) + 1) for c in itertools.combinations(FLAGS, k)]
BASELINES = [frozenset(), frozenset(['alignment']), frozenset(['prosody']), frozenset(['style']), frozenset(['aligned']),
             frozenset(['energy']), frozenset(['prosody', 'aligned']), frozenset(['energy', 'aligned'])]
F0_ALIGNED_KEYS = ('vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_bias_cents', 'lf0_corr')
# which of a flag's keys describe the synthesised side (None for a row without a waveform)
SYN_PROSODY_KEYS = ('f0_median_hz', 'f0_spread_st', 'voiced_share', 'f0_shift_st')
SYN_ENERGY_KEYS = ('loudness_lufs', 'loudness_shift_lu', 'energy_spread_db')


def _exact(a, b):
    """equal to the bit: None with None, NaN with NaN, a number with the same number of the same type"""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from scipy.io.wavfile import write
    from synthesizer import Synthesizer
    d = tmp_path_factory.mktemp('combinations')
    hp, ck, fl = _synth(d, "max_decoder_steps=%d" % STEPS)
    wavs = []
    for i in range(len(TEXTS)):
        wavs.append(os.path.join(str(d), 'h%02d.wav' % i))
        write(wavs[-1], 16000, np.round(yin_ref.harmonic_tone(FREQS[i], SAMPLES[i], phase_seed=i) * 32767 * 0.9).astype(np.int16))
    rows = [(w, t, '0', e) for w, t, e in zip(wavs, TEXTS, EMOS)]
    with open(fl, 'w', encoding='utf-8') as f:
        for r in rows:
            f.write('%s|%s|%s|%d\n' % r)
    syn = Synthesizer(hp).load(ck, vocoder='griffin_lim', filelist_path=fl)
    dec = syn.model.decoder
    dec.gate_threshold, thr = 1.0, dec.gate_threshold
    logits = []
    with torch.no_grad():
        for i0 in range(0, len(rows), 2):
            g = rows[i0:i0 + 2]
            logits.append(syn._synthesize_ragged([r[1] for r in g], True, [r[0] for r in g], (1.0, 0.0, 0.0, 0.0))[2][:, :, 0].cpu())
    dec.gate_threshold = thr
    shift, n_want, hit_want = _pick_bias(torch.cat(logits) - float(np.log(thr / (1 - thr))))
    with torch.no_grad():
        dec.gate_layer.linear_layer.bias -= shift
    # two rows are reported shorter than they were decoded (test_style_eval_gpu's _one_short_row, on the instance for the life
    # of the module).  At 1 frame: the last row, a group of its own, so that one group has no waveform at all (if it is too
    # short to be cut, the longest row).  At 3 frames: the longest other row whose neighbour in its group keeps a waveform, so
    # that one group has a waveform for some of its rows only (if there is none, the longest other row).
    longest = sorted(range(len(rows)), key=lambda i: -n_want[i])
    one = len(rows) - 1 if n_want[-1] >= 4 else longest[0]
    rest = [i for i in longest if i != one]
    paired = [i for i in rest if (i ^ 1) in rest and n_want[i ^ 1] >= 4]
    three = (paired or rest)[0]
    assert n_want[one] >= 4 and n_want[three] >= 4, n_want                      # both are cuts
    cuts = {TEXTS[one]: 1, TEXTS[three]: 3}
    orig = syn._synthesize_ragged

    def cut(texts, *a, **kw):
        out = list(orig(texts, *a, **kw))
        out[4] = out[4].clone()
        for text, frames in cuts.items():                   # (a cut only: under another conditioning a row may stop sooner)
            if text in texts:
                out[4][texts.index(text)] = min(int(out[4][texts.index(text)]), frames)
        return tuple(out)
    syn._synthesize_ragged = cut
    print("frames decoded %s; row %d is reported at 1 frame and row %d at 3" % (n_want, one, three))
    n_want = [1 if i == one else 3 if i == three else n for i, n in enumerate(n_want)]
    dec._calls = 0
    return dict(syn=syn, rows=rows, n_want=n_want, one=one, three=three, baselines={})


def _run(setup, condition, on):
    """(records, np.random state after the call) of one evaluate call from the seed 7 and a fresh decoder counter"""
    syn = setup['syn']
    np.random.seed(7)
    syn.model.decoder._calls = 0
    recs = syn.evaluate(setup['rows'], 2, condition, **{f: True for f in on})
    return recs, np.random.get_state()


def _baselines(setup, condition):
    """the runs that each group of keys is compared with, made once per condition and left unchanged"""
    if condition not in setup['baselines']:
        setup['baselines'][condition] = {on: _run(setup, condition, on) for on in BASELINES}
    return setup['baselines'][condition]


@pytest.mark.parametrize('condition,on', [('ref', s) for s in SUBSETS] + [('emotion', SUBSETS[0]), ('emotion', SUBSETS[-1])],
                         ids=lambda v: v if isinstance(v, str) else '+'.join(f for f in FLAGS if f in v) or 'plain')
def test_every_combination_equals_its_parts(setup, condition, on):
    from evaluation import (ALIGNED_KEYS, ALIGNMENT_KEYS, ENERGY_ALIGNED_KEYS, ENERGY_KEYS, PROSODY_KEYS, STYLE_KEYS, StyleRecords)
    syn, rows = setup['syn'], setup['rows']
    base = _baselines(setup, condition)
    recs, state = _run(setup, condition, on)
    assert syn.model.decoder._calls == len(rows) and len(recs) == len(rows)                       # 3
    if condition == 'ref':
        assert [r['n_frames'] for r in recs] == setup['n_want']
    assert recs[setup['one']]['n_frames'] == 1 and recs[setup['three']]['n_frames'] <= 3
    # 1: the keys
    keys_of = dict(alignment=ALIGNMENT_KEYS, prosody=PROSODY_KEYS, style=STYLE_KEYS, aligned=ALIGNED_KEYS, energy=ENERGY_KEYS)
    want_keys = set(PLAIN_KEYS)
    for f in on:
        want_keys |= set(keys_of[f])
    if 'energy' in on and 'aligned' in on:
        want_keys |= set(ENERGY_ALIGNED_KEYS)
    assert all(set(r) == want_keys for r in recs)

    # 2: every group of keys against the run that makes it
    def same(keys, baseline):
        for i, (got, want) in enumerate(zip(recs, base[frozenset(baseline)][0])):
            for k in keys:
                assert _exact(got[k], want[k]), (i, k, got[k], want[k])
    same(sorted(PLAIN_KEYS), [])
    for f in ('alignment', 'prosody', 'style', 'energy'):
        if f in on:
            same(keys_of[f], [f])
    if 'aligned' in on:
        same(('mcd_db', 'warp_dev'), ['aligned'])
        if 'prosody' in on:
            same(F0_ALIGNED_KEYS, ['prosody', 'aligned'])
        else:
            assert all(r[k] is None for r in recs for k in F0_ALIGNED_KEYS)
        if 'energy' in on:
            same(ENERGY_ALIGNED_KEYS, ['energy', 'aligned'])
    # 4: the type of the result
    assert isinstance(recs, StyleRecords) == ('style' in on) and isinstance(recs, list)
    if 'style' in on:
        assert recs.style_info == base[frozenset(['style'])][0].style_info
        assert all(type(a) is type(b) for a, b in zip(recs.style_info.values(), base[frozenset(['style'])][0].style_info.values()))
    else:
        assert type(recs) is list
    # 5: the draws
    if 'prosody' in on or 'energy' in on:
        assert _state_equal(state, base[frozenset(['prosody'])][1])
        assert _state_equal(state, base[frozenset()][1]) == all(r['n_frames'] < 4 for r in recs)   # one draw per waveform
    else:
        np.random.seed(7)
        assert _state_equal(state, np.random.get_state())
    # 6: the short rows, the two that were cut among them: under 4 frames no waveform, under 2 no style
    no_wav = [r for r in recs if r['n_frames'] < 4]
    assert recs[setup['one']] in no_wav and recs[setup['three']] in no_wav
    if 'prosody' in on:
        assert all(r[k] is None for r in no_wav for k in SYN_PROSODY_KEYS)
        assert all(r['f0_ref_median_hz'] is not None for r in no_wav)
        assert all(r['voiced_share'] is not None for r in recs if r not in no_wav)
    if 'energy' in on:
        assert all(r[k] is None for r in no_wav for k in SYN_ENERGY_KEYS)
        assert all(r['energy_ref_spread_db'] is not None for r in no_wav)
        assert all(r['energy_spread_db'] is not None for r in recs if r not in no_wav)
    if 'style' in on:
        for r in recs:
            assert all((r[k] is None) == (r['n_frames'] < 2) for k in STYLE_KEYS), r
        if condition == 'ref':
            assert recs[setup['three']]['style_hit'] is not None and recs[setup['one']]['style_hit'] is None
