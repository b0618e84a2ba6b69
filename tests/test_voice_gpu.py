"""t2v_voice_quality on the device: every plane against the fp64 reference (voice_ref) within four times what the reference's
own arithmetic loses in fp32, the bits of a row alone and in a batch at other strides, the silent and the padding frames, and
the refusals of the entry point; then the routes that use it: Synthesizer.evaluate(voice=True) on test_energy_eval_gpu's setup
against the composition by hand, and Synthesizer.voice_quality against the per-wav call."""
import numpy as np
import pytest
import torch

import voice_ref as R
from test_energy_eval_gpu import setup  # noqa: F401  (the fixture: harmonic recordings, 32 decoder steps, a gate bias)
from test_prosody_gpu import PLAIN_KEYS, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rows():
    """gpu_rows() with their fp64 planes, computed once"""
    return [(name, x, R.voice_quality(x)) for name, x in R.gpu_rows()]


def _batch(xs, stride, dev):
    y = torch.full((len(xs), stride), 7.0)                      # what lies past a row's samples is never read
    for b, x in enumerate(xs):
        y[b, :len(x)] = torch.from_numpy(x)
    return y.to(dev)


def _raw(y, n, t_stride):
    """the entry point itself: (B, 6, t_stride) with the planes' padding"""
    import t2v_hip
    lib = t2v_hip.load_library()
    out = torch.full((y.size(0), 6, t_stride), float('nan'), device=y.device)
    nn = torch.tensor(n, dtype=torch.int32, device=y.device)
    rc = lib.t2v_voice_quality(t2v_hip._p(y), t2v_hip._p(nn), y.size(1), y.size(0), t2v_hip._p(out), t_stride, t2v_hip._stream())
    assert rc == 0, rc
    return out


def test_every_plane_equals_the_reference(rows):
    import t2v_hip
    assert t2v_hip.VOICE_FEATS == R.FEATS and t2v_hip.VOICE_FRAMES == R.FRAMES_PER_WORKGROUP
    assert t2v_hip.VOICE_SILENT_DB == R.SILENT_DB
    dev = torch.device('cuda:0')
    xs = [x for _, x, _ in rows]
    n = [len(x) for x in xs]
    got = t2v_hip.voice_quality(_batch(xs, max(n) + 777, dev), n)          # y_stride larger than needed
    assert isinstance(got, t2v_hip.VoiceQuality) and got._fields == R.FEATS
    host = {k: getattr(got, k).cpu().double().numpy() for k in R.FEATS}
    worst = dict.fromkeys(R.GPU_TOL, 0.0)
    lag_bad = lag_exempt = total = 0
    for b, (name, x, want) in enumerate(rows):
        T = R.n_frames(len(x))
        total += T
        for k in R.GPU_TOL:
            worst[k] = max(worst[k], float(np.abs(host[k][b, :T] - want[k]).max()))
        sure = want['lag_margin'] > R.GPU_TOL['cpp_db']
        lag_exempt += int((~sure).sum())
        lag_bad += int((host['cpp_lag'][b, :T][sure] != want['cpp_lag'][sure]).sum())
        assert np.array_equal(host['level_db'][b, :T] == R.SILENT_DB, want['level_db'] == R.SILENT_DB), name
        for k in R.FEATS:
            assert not host[k][b, T:].any(), (name, k)
    for k in R.GPU_TOL:
        print("%-14s max |gpu - fp64| %.3e   tolerance %.3e" % (k, worst[k], R.GPU_TOL[k]))
    print("cpp_lag: %d of %d frames left out, %d of the others differ" % (lag_exempt, total, lag_bad))
    assert lag_exempt <= R.LAG_EXEMPT_CAP * total
    for k in R.GPU_TOL:
        assert worst[k] <= R.GPU_TOL[k], (k, worst[k], R.GPU_TOL[k])
    assert lag_bad == 0


def test_a_row_alone_has_the_bits_of_the_row_in_a_batch(rows):
    import t2v_hip
    dev = torch.device('cuda:0')
    xs = [x for _, x, _ in rows]
    n = [len(x) for x in xs]
    S = max(n) + 300
    t_stride = S // 256 + 1 + 5                                            # t_stride larger than needed
    batch = _raw(_batch(xs, S, dev), n, t_stride).cpu()
    assert not torch.isnan(batch).any()
    for b, (name, x, want) in enumerate(rows):
        T = R.n_frames(len(x))
        alone = _raw(_batch([x], len(x), dev), [len(x)], T).cpu()         # the smallest strides the call takes
        assert alone[0].numpy().tobytes() == batch[b, :, :T].contiguous().numpy().tobytes(), name
        tail = batch[b, :, T:]
        assert tail.numel() and not tail.any() and not torch.signbit(tail).any(), name       # +0 up to t_stride
        silent = torch.from_numpy(want['level_db'] == R.SILENT_DB)
        assert (batch[b, 0, :T][silent] == R.SILENT_DB).all() and not batch[b, 1:, :T][:, silent].any(), name
        assert not torch.signbit(batch[b, 1:, :T][:, silent]).any(), name
    zero = [b for b, (name, _, _) in enumerate(rows) if name.startswith('zeros')]
    assert len(zero) == 1 and (batch[zero[0], 0, :R.n_frames(n[zero[0]])] == R.SILENT_DB).all()
    # a length is clamped to the row: a count past y_stride reads what y_stride holds, a negative one nothing
    x = xs[0][:2000]
    y = _batch([x, x], 2000, dev)
    got = _raw(y, [5000, -3], 2000 // 256 + 1).cpu()
    assert got[0].numpy().tobytes() == _raw(y[:1], [2000], 2000 // 256 + 1).cpu()[0].numpy().tobytes() and not got[1].any()


def test_bad_arguments_are_refused():
    import t2v_hip
    lib = t2v_hip.load_library()
    dev = torch.device('cuda:0')
    y = torch.zeros(2, 1000, device=dev)
    n = torch.tensor([1000, 500], dtype=torch.int32, device=dev)
    out = torch.zeros(2, 6, 8, device=dev)
    p, st = t2v_hip._p, t2v_hip._stream()
    ERR_ARG = t2v_hip._ABI.define('T2V_ERR_ARG')
    assert lib.t2v_voice_quality(p(y), p(n), 1000, 2, p(out), 4, st) == 0          # 1000 // 256 + 1 = 4 frames
    for args in ((None, p(n), 1000, 2, p(out), 4), (p(y), None, 1000, 2, p(out), 4), (p(y), p(n), 1000, 2, None, 4),
                 (p(y), p(n), 1000, 0, p(out), 4), (p(y), p(n), 0, 2, p(out), 4), (p(y), p(n), (1 << 30) + 1, 2, p(out), 1 << 23),
                 (p(y), p(n), 1000, 2, p(out), 3)):
        assert lib.t2v_voice_quality(*args, st) == ERR_ARG, args
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    with pytest.raises(ValueError, match="float32"):
        t2v_hip.voice_quality(y.double(), [1000, 500])
    with pytest.raises(ValueError, match="1..1000"):
        t2v_hip.voice_quality(y, [1000, 1001])
    with pytest.raises(ValueError, match="empty"):
        t2v_hip.voice_quality(y[:, :0], [0, 0])
    with pytest.raises(ValueError, match="2 integer"):
        t2v_hip.voice_quality(y, [1000])


# ---------------------------------------------------------------------- Synthesizer.evaluate(voice=True), Synthesizer.voice_quality
def _host_tracks(vq, b, frames):
    import evaluation as E
    return {k: getattr(vq, k)[b, :frames].cpu().double().tolist() for k in E.VOICE_TRACKS}


def test_evaluate_voice_equals_the_manual_composition(setup):
    import evaluation as E
    import t2v_hip
    from synthesizer import Synthesizer
    syn, rows = setup['syn'], setup['rows']
    dec = syn.model.decoder
    others = PLAIN_KEYS | set(E.PROSODY_KEYS) | set(E.ALIGNED_KEYS) | set(E.ENERGY_KEYS) | set(E.ENERGY_ALIGNED_KEYS)
    voice_keys = set(E.VOICE_KEYS) | set(E.VOICE_ALIGNED_KEYS)
    np.random.seed(7)
    recs = syn.evaluate(rows, 2, prosody=True, aligned=True, energy=True, voice=True)
    assert dec._calls == len(rows)
    assert [r['n_frames'] for r in recs] == setup['n_want'] and [r['hit_max'] for r in recs] == setup['hit_want']
    assert all(set(r) == others | voice_keys for r in recs)
    # the same seeds without the flag: every other key keeps its bits
    dec._calls = 0
    np.random.seed(7)
    without = syn.evaluate(rows, 2, prosody=True, aligned=True, energy=True)
    assert all(set(r) == others for r in without)
    assert [{k: v for k, v in r.items() if k not in voice_keys} for r in recs] == without
    # alone it draws what prosody=True draws, and adds exactly VOICE_KEYS
    dec._calls = 0
    np.random.seed(7)
    alone = syn.evaluate(rows, 2, voice=True)
    state_alone = np.random.get_state()
    assert all(set(r) == PLAIN_KEYS | set(E.VOICE_KEYS) for r in alone)
    assert [{k: r[k] for k in E.VOICE_KEYS} for r in alone] == [{k: r[k] for k in E.VOICE_KEYS} for r in recs]
    dec._calls = 0
    np.random.seed(7)
    syn.evaluate(rows, 2, prosody=True)
    assert np.array_equal(np.random.get_state()[1], state_alone[1]) and np.random.get_state()[2] == state_alone[2]
    dec._calls = 0
    assert all(set(r) == PLAIN_KEYS for r in syn.evaluate(rows, 2, voice=False))
    # by hand
    np.random.seed(7)
    seen = dict(both=0, none=0, path=0)
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
        ref = t2v_hip.voice_quality(y_ref, n_samples)
        r = t2v_hip.aligned_scores(t2v_hip.mel_cepstrum(mel_postnet, n), n, t2v_hip.mel_cepstrum(truth, n_ref), n_ref, return_path=True)
        K, path = r.n_points.cpu().tolist(), r.path.cpu().numpy()
        for b in range(len(g)):
            rec = recs[i0 + b]
            ref_tracks = _host_tracks(ref, b, n_ref[b])
            if b in can:
                w = wavs[can.index(b)]
                one = t2v_hip.voice_quality(w[None].contiguous(), [w.numel()])
                assert one.level_db.size(1) == n[b]                                   # one frame per mel frame
                syn_tracks = _host_tracks(one, 0, n[b])
                want = E.voice_fields(syn_tracks, ref_tracks)
                ka, kb = E.voice_counted(syn_tracks['level_db']), E.voice_counted(ref_tracks['level_db'])
                pairs = [(syn_tracks['alpha_db'][i], ref_tracks['alpha_db'][j]) for i, j in path[b, :K[b]] if ka[i] and kb[j]]
                along = E.voice_path_fields(pairs)
                seen['path'] += along['alpha_rmse_db'] is not None
            else:
                want = E.voice_fields(None, ref_tracks)
                along = dict.fromkeys(E.VOICE_ALIGNED_KEYS)
                assert rec['alpha_db'] is None and rec['cpp_db'] is None and rec['alpha_shift_db'] is None
            print("row %d: %d x %d frames, %s, %s" % (i0 + b, n[b], n_ref[b], {k: rec[k] for k in E.VOICE_KEYS}, along))
            for k in E.VOICE_KEYS:
                assert _same(rec[k], want[k]), (i0 + b, k, rec[k], want[k])
            for k in E.VOICE_ALIGNED_KEYS:
                assert _same(rec[k], along[k]), (i0 + b, k, rec[k], along[k])
            assert rec['alpha_ref_db'] is not None and rec['cpp_ref_db'] is not None
            seen['both'] += rec['alpha_shift_db'] is not None
            seen['none'] += rec['alpha_shift_db'] is None
    print(seen)
    assert seen['both'] > 0 and seen['path'] > 0, seen
    s = E.summarize(recs)
    counted = [r for r in recs if not r['hit_max'] and r['alpha_shift_db'] is not None]
    v = s['voice']['overall']
    assert v['n_voice'] == len(counted) and set(s['voice']['by_emotion']) == {'neu', 'sad', 'ang', 'hap'}
    assert {'alpha_rmse_db_mean', 'alpha_corr_mean', 'cpp_shift_db_mean', 'hammarberg_ref_db_mean'} <= set(v)
    assert 'voice' not in E.summarize(without) and E.summarize(without)['energy'] == s['energy']
    # a row decoded to fewer than the vocoder's 4 frames has no waveform: None on its synthesised side, the recording's stays
    dec._calls = 0
    dec.max_decoder_steps = 3
    short = syn.evaluate(rows[:3], 2, voice=True, aligned=True)
    assert [r['n_frames'] <= 3 for r in short] == [True] * 3
    for r, full in zip(short, recs):
        assert all(r[k] is None for k in ('alpha_db', 'hammarberg_db', 'slope_db_khz', 'cpp_db', 'alpha_shift_db', 'cpp_shift_db'))
        assert all(r[k] is None for k in E.VOICE_ALIGNED_KEYS) and r['mcd_db'] is not None
        assert all(r[k] == full[k] for k in ('alpha_ref_db', 'hammarberg_ref_db', 'slope_ref_db_khz', 'cpp_ref_db'))
    # no Griffin-Lim vocoder: the error of prosody=True
    bare = Synthesizer(setup['hp']).load_checkpoint(setup['ck'])
    with pytest.raises(RuntimeError, match="Griffin-Lim"):
        bare.evaluate(rows, 2, voice=True)


def test_synthesizer_voice_quality_equals_the_per_wav_call(tmp_path):
    import t2v_hip
    from scipy.io.wavfile import write
    from synthesizer import Synthesizer
    specs = [('a.wav', 16000, R.tone(150.0, 9000, 1, 20.0, seed=1)), ('b48.wav', 48000, R.noise(30000, seed=2)),
             ('c.wav', 16000, R.tone(300.0, 2049, 2, 30.0, seed=3)), ('d.wav', 16000, R.tone(90.0, 12345, 1, 10.0, seed=4))]
    paths = []
    for name, sr, x in specs:
        paths.append(str(tmp_path / name))
        write(paths[-1], sr, np.round(np.clip(x, -1.0, 1.0) * 32767 * 0.9).astype(np.int16))
    syn = Synthesizer(resample=True)
    got = syn.voice_quality(paths, batch_size=3)
    assert len(got) == 4
    for p, g in zip(paths, got):
        y, n = syn.load_wavs([p])
        one = t2v_hip.voice_quality(y, n)
        assert tuple(g) == t2v_hip.VOICE_FEATS
        for k in t2v_hip.VOICE_FEATS:
            assert g[k].is_cuda and g[k].dim() == 1 and g[k].numel() == n[0] // 256 + 1
            assert g[k].cpu().numpy().tobytes() == getattr(one, k)[0].cpu().numpy().tobytes(), (p, k)
    assert float(got[0]['cpp_lag'].median()) == pytest.approx(16000 / 150.0, abs=1.0)
    with pytest.raises(ValueError, match="SR doesn't match"):
        Synthesizer().voice_quality(paths)
    with pytest.raises(ValueError):
        syn.voice_quality([])
