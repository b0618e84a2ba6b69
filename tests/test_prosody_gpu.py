"""Synthesizer.pitch, Synthesizer.evaluate(prosody=True) and evaluate.py --prosody on a random-init model and written
harmonic recordings: the records equal the manual composition (np.random seeded, the decode, GriffinLimVocoder.batch on the
pre-Postnet mel, t2v_hip.f0 on both sides, the statistics in numpy), and without the flag nothing changes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yin_ref
from test_batch_synthesis_gpu import _synth
from test_evaluate_gpu import EMOS, STEPS, TEXTS, _pick_bias
from test_prosody import TONE_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tacotron2-vae_amd')
PLAIN_KEYS = {'dtw', 'n_frames', 'n_ref_frames', 'hit_max', 'emotion'}
FREQS = (120.0, 233.3, 180.0, 310.0, 95.0, 150.0, 400.0)
SAMPLES = (9000, 4100, 14000, 6000, 12345, 4100, 7777)


def _write_harmonic_wavs(dirpath, count, tag='h'):
    """16 kHz int16 wavs of steady five-harmonic tones FREQS[i] of SAMPLES[i] samples (as _write_wavs of
    test_refenc_ragged_gpu.py writes its noisy sines, which are too noisy to be voiced)"""
    from scipy.io.wavfile import write
    paths = []
    for i in range(count):
        x = yin_ref.harmonic_tone(FREQS[i], SAMPLES[i], phase_seed=i)
        p = os.path.join(str(dirpath), '%s%02d.wav' % (tag, i))
        write(p, 16000, np.round(x * 32767 * 0.9).astype(np.int16))
        paths.append(p)
    return paths


def _stats(track):
    """(median, spread in semitones, voiced share) of a track in numpy, None under 5 voiced frames"""
    track = np.asarray(track, dtype=np.float64)
    v = track[track > 0]
    share = len(v) / len(track)
    if len(v) < 5:
        return None, None, share
    med = float(np.median(v))
    return med, float(np.std(12 * np.log2(v / med))), share


def _same(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got == pytest.approx(want, rel=1e-9, abs=1e-12))


def test_pitch_tracks_in_input_order(tmp_path):
    import hparams as HP
    import t2v_hip
    from synthesizer import Synthesizer
    syn = Synthesizer(HP.create_hparams())
    paths = _write_harmonic_wavs(tmp_path, len(FREQS))
    tracks = syn.pitch(paths, batch_size=3)                 # groups sorted by length: (2, 4, 0), (6, 3, 1), (5)
    assert len(tracks) == len(paths)
    for i, (p, trk) in enumerate(zip(paths, tracks)):
        assert trk.dim() == 1 and trk.is_cuda and trk.numel() == SAMPLES[i] // 256 + 1
        y, n = syn.load_wavs([p])
        assert n == [SAMPLES[i]]
        alone = t2v_hip.f0(y, n)[0]
        assert trk.cpu().numpy().tobytes() == alone.cpu().numpy().tobytes(), i
        v = trk[trk > 0].cpu().double().numpy()
        print("%s: %.1f Hz, %d of %d frames voiced, median %.3f" % (os.path.basename(p), FREQS[i], len(v), trk.numel(), np.median(v)))
        assert len(v) >= trk.numel() - 6
        assert abs(np.median(v) / FREQS[i] - 1) <= TONE_BOUND
    assert [t.cpu().numpy().tobytes() for t in syn.pitch(paths, batch_size=64)] == [t.cpu().numpy().tobytes() for t in tracks]
    with pytest.raises(ValueError):
        syn.pitch([])
    from scipy.io.wavfile import write
    other = str(tmp_path / 'sr8k.wav')
    write(other, 8000, np.zeros(4000, dtype=np.int16))
    with pytest.raises(ValueError, match="SR doesn't match"):
        syn.pitch([paths[0], other])
    with pytest.raises(ValueError, match="SR doesn't match"):
        syn.load_mels([other])


@pytest.fixture()
def setup(tmp_path):
    """test_evaluate_gpu's setup with harmonic recordings and the Griffin-Lim vocoder: a gate bias under which some rows stop
    and some never do"""
    from synthesizer import Synthesizer
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=%d" % STEPS)
    wavs = _write_harmonic_wavs(tmp_path, len(TEXTS))
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
    torch.save({'iteration': 1, 'state_dict': {k: v.detach().cpu().clone() for k, v in syn.model.state_dict().items()},
                'optimizer': {}, 'learning_rate': 1e-3}, ck)
    dec._calls = 0
    return dict(hp=hp, ck=ck, fl=fl, rows=rows, syn=syn, n_want=n_want, hit_want=hit_want)


def test_evaluate_prosody_equals_the_manual_composition(setup, tmp_path):
    import t2v_hip
    from evaluation import PROSODY_KEYS, summarize
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    np.random.seed(7)
    recs = syn.evaluate(rows, 2, prosody=True)
    assert dec._calls == len(rows)
    assert [r['n_frames'] for r in recs] == setup['n_want'] and [r['hit_max'] for r in recs] == setup['hit_want']
    assert all(set(r) == PLAIN_KEYS | set(PROSODY_KEYS) for r in recs)
    np.random.seed(7)
    checked_written = False
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        texts, paths = [r[1] for r in g], [r[0] for r in g]
        dec._calls = i0
        with torch.no_grad():
            mel, _, _, _, n_frames, _ = syn._synthesize_ragged(texts, True, paths, (1.0, 0.0, 0.0, 0.0))
        n = n_frames.tolist()
        can = [b for b in range(len(g)) if n[b] >= 4]          # the vocoder needs 4 frames
        state = np.random.get_state()
        wavs = syn.vocoder.batch(mel[can], [n[b] for b in can]) if can else []
        if len(can) == len(g) and not checked_written:
            # the waveforms are the ones synthesize_batch(paths=...) writes from the same decoder seeds and np.random state
            after = np.random.get_state()
            np.random.set_state(state)
            dec._calls = i0
            outs = [str(tmp_path / ('syn%d.wav' % b)) for b in range(len(g))]
            syn.synthesize_batch(texts, outs, True, paths)
            from scipy.io.wavfile import read
            for b in range(len(g)):
                assert read(outs[b])[1].tobytes() == wavs[b].cpu().numpy().tobytes()
            np.random.set_state(after)
            checked_written = True
        y_ref, n_ref = syn.load_wavs(paths)
        ref_tracks = t2v_hip.f0(y_ref, n_ref).cpu().numpy()
        for b in range(len(g)):
            rec = recs[i0 + b]
            rmed, rspread, rshare = _stats(ref_tracks[b, :n_ref[b] // 256 + 1])
            assert rmed is not None and rshare > 0.8                            # a harmonic recording has a pitch
            assert abs(rmed / FREQS[i0 + b] - 1) <= TONE_BOUND
            if b in can:
                w = wavs[can.index(b)]
                assert w.numel() == (n[b] - 1) * 256
                med, spread, share = _stats(t2v_hip.f0(w[None].contiguous(), [w.numel()])[0].cpu().numpy())
            else:
                med = spread = share = None
            print("row %d: %d frames, synthesised median %s Hz spread %s st voiced %s; recording %.2f Hz spread %.4f st voiced %.2f"
                  % (i0 + b, n[b], med, spread, share, rmed, rspread, rshare))
            want = {'f0_median_hz': med, 'f0_ref_median_hz': rmed, 'f0_spread_st': spread, 'f0_ref_spread_st': rspread,
                    'voiced_share': share, 'voiced_ref_share': rshare,
                    'f0_shift_st': None if med is None else 12 * np.log2(med / rmed)}
            for k, v in want.items():
                assert _same(rec[k], v), (i0 + b, k, rec[k], v)
            if share is not None and round(share * n[b]) < 5:
                assert rec['f0_median_hz'] is None and rec['f0_spread_st'] is None and rec['f0_shift_st'] is None
    s = summarize(recs)['overall']
    counted = [r for r in recs if not r['hit_max'] and r['f0_shift_st'] is not None]
    assert s['n_prosody'] == len(counted) <= s['n_scored']
    assert s['n_rows'] == len(recs) and s['n_hit_max'] == sum(setup['hit_want'])
    if counted:
        assert s['f0_shift_st_mean'] == pytest.approx(np.mean([r['f0_shift_st'] for r in counted]))
    else:
        assert s['f0_shift_st_mean'] is None and s['f0_spread_ratio_mean'] is None
    stopped = [r for r in recs if not r['hit_max']]
    assert s['voiced_ref_share_mean'] == pytest.approx(np.mean([r['voiced_ref_share'] for r in stopped]))


def test_evaluate_without_the_flag_is_unchanged(setup):
    from synthesizer import Synthesizer
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    np.random.seed(11)
    before = np.random.get_state()
    plain = syn.evaluate(rows, 2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]       # no draw
    assert dec._calls == len(rows)
    assert all(set(r) == PLAIN_KEYS for r in plain)
    dec._calls = 0
    with_f0 = syn.evaluate(rows, 2, prosody=True)
    assert dec._calls == len(rows)                                              # the same decoder seeds
    assert [{k: r[k] for k in PLAIN_KEYS} for r in with_f0] == plain             # and the same scores, to the bit
    assert not np.array_equal(np.random.get_state()[1], after[1])               # Griffin-Lim drew its phases
    bare = Synthesizer(setup['hp']).load_checkpoint(setup['ck'])
    with pytest.raises(RuntimeError, match="Griffin-Lim"):
        bare.evaluate(rows, 2, prosody=True)
    bare.vocoder = lambda mel: mel
    with pytest.raises(RuntimeError, match="Griffin-Lim"):
        bare.evaluate(rows, 2, prosody=True)


def test_evaluate_cli_prosody(setup, tmp_path):
    from evaluation import PROSODY_KEYS
    rows = setup['rows']
    out = str(tmp_path / 'score.json')
    r = subprocess.run([sys.executable, os.path.join(PKG, 'evaluate.py'), '--load_path', setup['ck'], '--filelist_path', setup['fl'],
                        '--batch_size', '2', '--hparams', 'max_decoder_steps=%d' % STEPS, '--prosody', '--out', out],
                       capture_output=True, text=True, timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out, encoding='utf-8') as f:
        d = json.load(f)
    assert [x['path'] for x in d['rows']] == [r_[0] for r_ in rows]
    for x in d['rows']:
        assert set(PROSODY_KEYS) <= set(x)
        assert x['f0_ref_median_hz'] is not None and x['voiced_ref_share'] > 0.8
    for stats in [d['summary']['overall']] + list(d['summary']['by_emotion'].values()):
        assert {'n_prosody', 'f0_shift_st_mean', 'f0_shift_st_abs_mean', 'f0_spread_ratio_mean', 'voiced_share_mean',
                'voiced_ref_share_mean'} <= set(stats)
    assert d['summary']['overall']['n_rows'] == len(rows)
    assert '"n_prosody"' in r.stdout
