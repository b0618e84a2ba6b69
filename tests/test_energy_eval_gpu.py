"""The routes that use the loudness meter, on the device: Synthesizer.loudness on written wavs (one read through
resample=True), prepare_corpus.main with --lufs in both scopes and without it, and Synthesizer.evaluate(energy=True) on a
random-init model and written harmonic recordings (test_prosody_gpu's setup, with enough decoder steps for a 400 ms block):
the records equal the composition by hand of the vocoder, t2v_hip.loudness and evaluation.energy_fields, the path values equal
loudness_ref's on the returned path, and no other key moves."""
import json
import os

import numpy as np
import pytest
import torch

import loudness_ref as R
import yin_ref
from test_batch_synthesis_gpu import _synth
from test_evaluate_gpu import EMOS, TEXTS, _pick_bias
from test_loudness_gpu import DB_TOL, LU_TOL
from test_prosody_gpu import FREQS, PLAIN_KEYS, _same

pytestmark = pytest.mark.gpu

STEPS = 32                                   # (32 - 1) * 256 = 7 936 samples: a row that runs to the end holds one 400 ms block
SAMPLES = (9000, 7000, 14000, 8000, 12345)   # every recording holds one, so a row that runs to the end has a loudness shift


def _noise_wav(path, sr, seconds, amp, seed, spikes=0.0):
    from scipy.io.wavfile import write
    rng = np.random.RandomState(seed)
    x = amp * rng.randn(int(seconds * sr))
    if spikes:
        x[1000::3000] = spikes
    s = np.round(np.clip(x, -1.0, 32767.0 / 32768.0) * 32768.0).astype(np.int16)
    write(str(path), sr, s)
    return s.astype(np.float64) / 32768.0


def _read(path):
    from scipy.io.wavfile import read
    rate, s = read(str(path))
    assert s.dtype == np.int16
    return rate, s.astype(np.float64) / 32768.0


# ---------------------------------------------------------------------- Synthesizer.loudness
def test_synthesizer_loudness_equals_the_reference(tmp_path):
    from synthesizer import Synthesizer
    specs = [('a.wav', 16000, 1.1, 0.2, 1), ('b48.wav', 48000, 0.9, 0.05, 2), ('c.wav', 16000, 0.3, 0.1, 3)]
    paths = [str(tmp_path / s[0]) for s in specs]
    for p, (_, sr, seconds, amp, seed) in zip(paths, specs):
        _noise_wav(p, sr, seconds, amp, seed)
    syn = Synthesizer(resample=True)
    got = syn.loudness(paths, batch_size=2)
    assert len(got) == 3
    for p, g in zip(paths, got):
        y, n = syn.load_wavs([p])                                                   # what the meter saw: 16 kHz samples
        want = R.measure(y[0, :n[0]].cpu().double().numpy(), 16000)
        assert set(g) == {'loudness_lufs', 'momentary_max_lufs', 'energy_db'}
        print("%s: %.4f LUFS (reference %.4f)" % (os.path.basename(p), g['loudness_lufs'], want['integrated']))
        if np.isinf(want['integrated']):
            assert g['loudness_lufs'] == float('-inf') and g['momentary_max_lufs'] == float('-inf')
        else:
            assert abs(g['loudness_lufs'] - want['integrated']) <= LU_TOL
            assert abs(g['momentary_max_lufs'] - want['momentary_max']) <= DB_TOL
        db = g['energy_db']
        assert db.is_cuda and db.dim() == 1 and db.numel() == n[0] // 256 + 1
        level = R.energy_db(want['frame_ms'])
        loud = level > -70.0
        assert loud.any() and np.abs(db.cpu().double().numpy()[loud] - level[loud]).max() <= DB_TOL
    assert np.isinf(got[2]['loudness_lufs']) and not np.isinf(got[0]['loudness_lufs'])      # 0.3 s holds no block
    with pytest.raises(ValueError, match="SR doesn't match"):
        Synthesizer().loudness(paths)
    with pytest.raises(ValueError):
        syn.loudness([])


# ---------------------------------------------------------------------- prepare_corpus.py --lufs
def _prepare(tmp_path, rows, extra):
    import prepare_corpus as PC
    filelist = tmp_path / 'in.txt'
    filelist.write_text(''.join('|'.join(r) + '\n' for r in rows), encoding='utf-8')
    out_dir, out_list, report_path = tmp_path / 'out', tmp_path / 'out.txt', tmp_path / 'rep.json'
    report = PC.main(['--filelist_path', str(filelist), '--out_dir', str(out_dir), '--out_filelist', str(out_list), '--report',
                      str(report_path)] + extra)
    assert report == json.loads(report_path.read_text(encoding='utf-8'))
    return report, [line.split('|')[0] for line in out_list.read_text(encoding='utf-8').splitlines()]


def test_prepare_corpus_lufs_per_utterance(tmp_path):
    src = [str(tmp_path / n) for n in ('loud.wav', 'quiet.wav', 'spiky.wav', 'short.wav')]
    before = [_noise_wav(src[0], 16000, 1.0, 0.2, 1), _noise_wav(src[1], 44100, 1.2, 0.01, 2),
              _noise_wav(src[2], 16000, 1.0, 0.003, 3, spikes=0.9), _noise_wav(src[3], 16000, 0.3, 0.1, 4)]
    report, written = _prepare(tmp_path, [(p, 'text', '0', '0') for p in src], ['--lufs', '-23', '--batch_size', '3'])
    assert report['n_written'] == 4 and report['loudness']['target_lufs'] == -23.0 and report['loudness']['scope'] == 'utterance'
    assert 'speakers' not in report
    peak_lin = 10.0 ** (-1.0 / 20.0)
    for i in (0, 1):
        rate, x = _read(written[i])
        m = R.measure(x, 16000)
        rec = report['rows'][i]
        print("%s: %.3f LUFS -> %.3f LUFS, gain %.3f dB" % (os.path.basename(src[i]), rec['loudness_lufs'], m['integrated'], rec['gain_db']))
        assert rate == 16000 and abs(m['integrated'] + 23.0) <= 0.05                # the margin covers the int16 rounding
        assert rec['gain_limited'] is False and rec['gain_db'] == pytest.approx(-23.0 - rec['loudness_lufs'])
        assert rec['peak'] == pytest.approx(np.abs(x).max(), abs=1.0 / 32768.0) and rec['clipped_samples'] == 0
    assert abs(report['rows'][0]['loudness_lufs'] - R.measure(before[0], 16000)['integrated']) <= LU_TOL
    # the wav that would clip: its gain stops where the peak reaches --peak_db
    rate, x = _read(written[2])
    rec = report['rows'][2]
    assert rec['gain_limited'] is True and rec['gain_db'] < -23.0 - rec['loudness_lufs']
    assert R.measure(x, 16000)['integrated'] < -23.0 - 1.0
    assert np.abs(x).max() == pytest.approx(peak_lin, abs=1.5 / 32768.0) and rec['clipped_samples'] == 0
    assert rec['peak'] == pytest.approx(peak_lin, rel=1e-5)
    # no block, no loudness: written unscaled
    rate, x = _read(written[3])
    rec = report['rows'][3]
    assert rec['loudness_lufs'] is None and rec['gain_db'] == 0.0 and rec['gain_limited'] is False
    assert np.abs(x).max() == pytest.approx(np.abs(before[3]).max(), abs=1.0 / 32768.0)
    tot = report['loudness']
    have = [r['loudness_lufs'] for r in report['rows'][:3]]
    assert tot['rows'] == 3 and tot['mean_lufs'] == pytest.approx(np.mean(have)) and tot['spread_lu'] == pytest.approx(np.std(have))


def test_prepare_corpus_lufs_per_speaker(tmp_path):
    import prepare_corpus as PC
    amps = [('s1', 0.2), ('s1', 0.05), ('s2', 0.02), ('s2', 0.08)]
    src = [str(tmp_path / ('w%d.wav' % i)) for i in range(4)]
    before = [R.measure(_noise_wav(p, 16000, 1.0 + 0.1 * i, a, 10 + i), 16000) for i, (p, (_, a)) in enumerate(zip(src, amps))]
    report, written = _prepare(tmp_path, [(p, 'text', spk, str(i % 4)) for i, (p, (spk, _)) in enumerate(zip(src, amps))],
                               ['--lufs', '-23', '--lufs_scope', 'speaker', '--batch_size', '3'])
    after = [R.measure(_read(p)[1], 16000) for p in written]
    assert set(report['speakers']) == {'s1', 's2'} and report['loudness']['scope'] == 'speaker'
    for spk, idx in (('s1', (0, 1)), ('s2', (2, 3))):
        pooled = R.pooled([after[i]['gated_sum'] for i in idx], [after[i]['gated_blocks'] for i in idx])
        s = report['speakers'][spk]
        print("%s: pooled %.3f LUFS -> %.3f LUFS, gain %.3f dB" % (spk, s['loudness_lufs'], pooled, s['gain_db']))
        assert abs(pooled + 23.0) <= 0.05                                           # the speaker is on target
        assert s['rows'] == 2 and s['gain_limited'] is False and s['gain_db'] == pytest.approx(-23.0 - s['loudness_lufs'])
        want = R.pooled([before[i]['gated_sum'] for i in idx], [before[i]['gated_blocks'] for i in idx])
        assert abs(s['loudness_lufs'] - want) <= LU_TOL
        d_before = before[idx[0]]['integrated'] - before[idx[1]]['integrated']
        d_after = after[idx[0]]['integrated'] - after[idx[1]]['integrated']
        assert abs(d_before) > 5.0 and abs(d_after - d_before) <= 0.02               # the emotions keep their level difference
        for i in idx:
            assert report['rows'][i]['gain_db'] == s['gain_db'] and report['rows'][i]['gain_limited'] is False
    with pytest.raises(SystemExit, match="third column"):
        two = tmp_path / 'two.txt'
        two.write_text(src[0] + '|text\n', encoding='utf-8')
        PC.main(['--filelist_path', str(two), '--out_dir', str(tmp_path / 'o2'), '--out_filelist', str(tmp_path / 'o2.txt'),
                 '--lufs', '-23', '--lufs_scope', 'speaker'])
    with pytest.raises(SystemExit, match="11025"):
        PC.main(['--filelist_path', str(tmp_path / 'in.txt'), '--out_dir', str(tmp_path / 'o3'), '--out_filelist',
                 str(tmp_path / 'o3.txt'), '--lufs', '-23', '--sampling_rate', '11025'])


def test_prepare_corpus_without_lufs_is_unchanged(tmp_path):
    import t2v_hip
    src = [str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')]
    _noise_wav(src[0], 16000, 0.5, 0.2, 1)
    _noise_wav(src[1], 48000, 0.4, 0.05, 2)
    from scipy.io.wavfile import read, write
    stereo = str(tmp_path / 'stereo.wav')                                          # skipped from its header, between the two
    write(stereo, 16000, np.zeros((500, 2), dtype=np.int16))
    report, written = _prepare(tmp_path, [(p, 'text', '0', '0') for p in (src[0], stereo, src[1])], ['--batch_size', '1'])
    assert set(report) == {'target_rate', 'trim_db', 'pad_frames', 'n_rows', 'n_written', 'n_skipped', 'by_source_rate', 'rows'}
    assert report['n_rows'] == 3 and report['n_written'] == 2 and report['n_skipped'] == 1
    assert set(report['rows'][1]) == {'path', 'skipped'} and 'channels' in report['rows'][1]['skipped']
    assert [os.path.basename(w) for w in written] == ['a.wav', 'b.wav']             # the filelist keeps the order of its rows
    for p, out, rec in zip(src, written, [report['rows'][0], report['rows'][2]]):
        assert set(rec) == {'source_rate', 'target_rate', 'samples_in', 'samples_resampled', 'samples_out', 'trimmed_head_s',
                            'trimmed_tail_s', 'peak', 'clipped_samples', 'all_silent', 'path', 'out_path'}
        sr, s = read(p)
        y, n = t2v_hip.resample(torch.from_numpy(s[None]).cuda(), [len(s)], sr, 16000)
        bounds = t2v_hip.trim_bounds(y, n, 40.0, 2)
        pcm, counts, stats = t2v_hip.crop(y, bounds, pcm16=True, return_stats=True)
        assert read(out)[1].tobytes() == pcm[0, :counts[0]].cpu().numpy().tobytes()
        assert rec['peak'] == stats[0][1] and rec['clipped_samples'] == stats[0][0] and rec['samples_out'] == counts[0]


# ---------------------------------------------------------------------- Synthesizer.evaluate(energy=True)
@pytest.fixture()
def setup(tmp_path):
    """test_prosody_gpu's setup with STEPS decoder steps: harmonic recordings, the Griffin-Lim vocoder and a gate bias under
    which some rows stop and some never do"""
    from synthesizer import Synthesizer
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=%d" % STEPS)
    from scipy.io.wavfile import write
    wavs = []
    for i in range(len(TEXTS)):
        wavs.append(os.path.join(str(tmp_path), 'h%02d.wav' % i))
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
    dec._calls = 0
    return dict(hp=hp, ck=ck, rows=rows, syn=syn, n_want=n_want, hit_want=hit_want)


def test_evaluate_energy_equals_the_manual_composition(setup):
    import t2v_hip
    from evaluation import ALIGNED_KEYS, ENERGY_ALIGNED_KEYS, ENERGY_KEYS, PROSODY_KEYS, energy_fields, summarize
    from synthesizer import Synthesizer
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    np.random.seed(7)
    recs = syn.evaluate(rows, 2, prosody=True, aligned=True, energy=True)
    assert dec._calls == len(rows)
    assert [r['n_frames'] for r in recs] == setup['n_want'] and [r['hit_max'] for r in recs] == setup['hit_want']
    every = PLAIN_KEYS | set(PROSODY_KEYS) | set(ALIGNED_KEYS) | set(ENERGY_KEYS) | set(ENERGY_ALIGNED_KEYS)
    assert all(set(r) == every for r in recs)
    # the same seeds without the flag: every other key keeps its value
    dec._calls = 0
    np.random.seed(7)
    without = syn.evaluate(rows, 2, prosody=True, aligned=True)
    assert all(set(r) == PLAIN_KEYS | set(PROSODY_KEYS) | set(ALIGNED_KEYS) for r in without)
    assert [{k: v for k, v in r.items() if k not in ENERGY_KEYS + ENERGY_ALIGNED_KEYS} for r in recs] == without
    # alone it draws what prosody=True draws, and adds exactly ENERGY_KEYS
    dec._calls = 0
    np.random.seed(7)
    alone = syn.evaluate(rows, 2, energy=True)
    state_alone = np.random.get_state()
    assert all(set(r) == PLAIN_KEYS | set(ENERGY_KEYS) for r in alone)
    assert [{k: r[k] for k in ENERGY_KEYS} for r in alone] == [{k: r[k] for k in ENERGY_KEYS} for r in recs]
    dec._calls = 0
    np.random.seed(7)
    syn.evaluate(rows, 2, prosody=True)
    assert np.array_equal(np.random.get_state()[1], state_alone[1]) and np.random.get_state()[2] == state_alone[2]
    dec._calls = 0
    assert all(set(r) == PLAIN_KEYS for r in syn.evaluate(rows, 2, energy=False))
    # by hand
    np.random.seed(7)
    seen = dict(loud=0, none=0, path=0)
    for i0 in range(0, len(rows), 2):
        g = rows[i0:i0 + 2]
        texts, paths = [r[1] for r in g], [r[0] for r in g]
        dec._calls = i0
        with torch.no_grad():
            mel, mel_postnet, _, _, n_frames, _ = syn._synthesize_ragged(texts, True, paths, (1.0, 0.0, 0.0, 0.0))
        n = n_frames.tolist()
        can = [b for b in range(len(g)) if n[b] >= 4]
        wavs = syn.vocoder.batch(mel[can], [n[b] for b in can]) if can else []
        y_ref, n_samples = syn.load_wavs(paths)
        truth, n_ref = syn.load_mels(paths)
        ref = t2v_hip.loudness(y_ref, n_samples, 16000)
        ref_db = t2v_hip.energy_db(ref.frame_ms).cpu().double().numpy()
        r = t2v_hip.aligned_scores(t2v_hip.mel_cepstrum(mel_postnet, n), n, t2v_hip.mel_cepstrum(truth, n_ref), n_ref, return_path=True)
        K, path = r.n_points.cpu().tolist(), r.path.cpu().numpy()
        for b in range(len(g)):
            rec = recs[i0 + b]
            track_ref = ref_db[b, :n_ref[b]]
            if b in can:
                w = wavs[can.index(b)]
                one = t2v_hip.loudness(w[None].contiguous(), [w.numel()], 16000)
                track = t2v_hip.energy_db(one.frame_ms)[0].cpu().double().numpy()
                assert len(track) == n[b]                                           # one energy frame per mel frame
                want = energy_fields(one.integrated[0], track, ref.integrated[b], track_ref)
                rmse, corr = R.path_energy(track, track_ref, path[b, :K[b]])
                assert want['energy_spread_db'] == pytest.approx(R.spread_db(track))
                seen['path'] += rmse is not None
            else:
                want = energy_fields(None, None, ref.integrated[b], track_ref)
                rmse = corr = None
            print("row %d: %d x %d frames, %s, rmse %s corr %s" % (i0 + b, n[b], n_ref[b], {k: rec[k] for k in ENERGY_KEYS}, rmse, corr))
            for k in ENERGY_KEYS:
                assert _same(rec[k], want[k]), (i0 + b, k, rec[k], want[k])
            assert _same(rec['energy_rmse_db'], rmse) and _same(rec['energy_corr'], corr), (i0 + b, rec['energy_rmse_db'], rmse)
            assert rec['energy_ref_spread_db'] is not None
            seen['loud'] += rec['loudness_shift_lu'] is not None
            seen['none'] += rec['loudness_shift_lu'] is None
    print(seen)
    assert seen['loud'] > 0 and seen['path'] > 0, seen                            # a row that ran to the end has every value
    s = summarize(recs)
    counted = [r for r in recs if not r['hit_max'] and r['loudness_shift_lu'] is not None]
    e = s['energy']['overall']
    assert e['n_energy'] == len(counted) and set(s['energy']['by_emotion']) == {'neu', 'sad', 'ang', 'hap'}
    assert {'energy_rmse_db_mean', 'energy_corr_mean', 'loudness_shift_lu_abs_mean', 'energy_spread_ratio_mean'} <= set(e)
    if counted:
        assert e['loudness_shift_lu_mean'] == pytest.approx(np.mean([r['loudness_shift_lu'] for r in counted]))
    assert 'energy' not in summarize(without)
    # no Griffin-Lim vocoder: the error of prosody=True
    bare = Synthesizer(setup['hp']).load_checkpoint(setup['ck'])
    with pytest.raises(RuntimeError, match="Griffin-Lim"):
        bare.evaluate(rows, 2, energy=True)
