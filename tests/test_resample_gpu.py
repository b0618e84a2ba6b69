"""csrc/resample.hip on the device against the fp64 definitions of resample_ref.py: the ragged polyphase resampler (bound
derived from the fp32 formats, not measured), the trim bounds (exact), the crop and 16-bit write-out (exact), and the two
routes that use them: Synthesizer(resample=True, trim_db=...) and prepare_corpus.main."""
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

RATES = (48000, 44100, 22050, 11025, 8000, 128000)   # 128 kHz: a window wider than one LDS pass, the kernel's other path
ROWS = (1, 777, 2049)
STRIDE = 2100                                   # wider than the longest row


def _bits(t):
    return t.cpu().numpy().tobytes()


def _rows(seed, lengths, stride, fill=np.nan):
    rng = np.random.RandomState(seed)
    x = np.full((len(lengths), stride), fill, dtype=np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.uniform(-1, 1, n).astype(np.float32)
    return x


@pytest.fixture(scope='module')
def batches():
    """per rate: (x (3, STRIDE) fp32 with NaN past each length, [(y, sum |t x|) per row in fp64 from the fp32 taps])"""
    import t2v_hip
    out = {}
    for sr in RATES:
        up, down, half, taps = t2v_hip.resample_taps(sr, 16000)
        x = _rows(sr, ROWS, STRIDE)
        out[sr] = (x, [R.resample(x[b, :n], up, down, half, taps)[:2] for b, n in enumerate(ROWS)])
    return out


@pytest.mark.parametrize('sr', RATES)
def test_batch_against_the_fp64_reference(batches, sr):
    """A K-term fp32 fma chain, in any order, errs by at most K u sum |t x| to first order (u = 2^-24); (K + 1) u sum |t x|
    covers the higher orders for K u << 1 and the rounding of nothing else: the taps are the reference's own fp32 taps and the
    samples are fp32 on both sides.  K is the tap count of the longest phase."""
    import t2v_hip
    x, ref = batches[sr]
    up, down, half, _ = t2v_hip.resample_taps(sr, 16000)
    y, n_out = t2v_hip.resample(torch.from_numpy(x).cuda(), list(ROWS), sr, 16000)
    assert n_out == [-((-n * up) // down) for n in ROWS] and tuple(y.shape) == (len(ROWS), max(n_out))
    y = y.cpu().numpy()
    K = R.taps_per_phase(up, half)
    for b, (want, mag) in enumerate(ref):
        err = np.abs(y[b, :n_out[b]].astype(np.float64) - want)
        bound = (K + 1) * 2.0 ** -24 * mag
        print("%d Hz row %d: n_out %d, K %d, worst error %.3g, worst error / bound %.3f"
              % (sr, b, n_out[b], K, err.max(), np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (sr, b)
        assert np.all(y[b, n_out[b]:] == 0) and not np.signbit(y[b, n_out[b]:]).any()


def test_pcm16_rows_give_the_bits_of_their_fp32_values():
    import t2v_hip
    rng = np.random.RandomState(5)
    s = np.zeros((3, 1300), dtype=np.int16)
    n = [1300, 1, 640]
    for b, k in enumerate(n):
        s[b, :k] = rng.randint(-32768, 32768, k)
    s[0, :2] = (-32768, 32767)
    f = s.astype(np.float32) / np.float32(32768.0)
    for sr in (44100, 8000, 16000):
        y16, n16 = t2v_hip.resample(torch.from_numpy(s).cuda(), n, sr, 16000)
        y32, n32 = t2v_hip.resample(torch.from_numpy(f).cuda(), n, sr, 16000)
        assert n16 == n32 and y16.dtype == torch.float32 and _bits(y16) == _bits(y32), sr


@pytest.mark.parametrize('sr', (48000, 44100, 8000, 128000))
def test_a_row_alone_in_the_batch_and_at_another_stride(batches, sr):
    import t2v_hip
    x, _ = batches[sr]
    y, n_out = t2v_hip.resample(torch.from_numpy(x).cuda(), list(ROWS), sr, 16000)
    for b, n in enumerate(ROWS):
        alone, k = t2v_hip.resample(torch.from_numpy(x[b:b + 1, :n].copy()).cuda(), [n], sr, 16000)
        assert k == [n_out[b]] and _bits(alone[0, :k[0]]) == _bits(y[b, :k[0]]), (sr, b)
        wide = np.full((2, n + 333), np.nan, dtype=np.float32)
        wide[1, :n] = x[b, :n]
        wide[0, :5] = 0.25
        other, k2 = t2v_hip.resample(torch.from_numpy(wide).cuda(), [5, n], sr, 16000)
        assert k2[1] == n_out[b] and _bits(other[1, :k2[1]]) == _bits(y[b, :k2[1]]), (sr, b)


@pytest.mark.parametrize('sr,lengths', [(48000, (768, 769, 1)), (44100, (705, 706, 1)), (48000, (3072, 3073, 1)), (44100, (5292, 5293, 1))])
def test_output_lengths_around_one_workgroup(sr, lengths):
    """256 outputs (one workgroup's lanes), 257 and 1; then a whole tile (1024 outputs at 48 kHz, 1920 at 44.1 kHz), one more and 1"""
    import t2v_hip
    up, down, half, taps = t2v_hip.resample_taps(sr, 16000)
    x = _rows(11, lengths, max(lengths) + 7)
    y, n_out = t2v_hip.resample(torch.from_numpy(x).cuda(), list(lengths), sr, 16000)
    assert n_out in ([256, 257, 1], [1024, 1025, 1], [1920, 1921, 1])
    y = y.cpu().numpy()
    K = R.taps_per_phase(up, half)
    for b, n in enumerate(lengths):
        want, mag, _ = R.resample(x[b, :n], up, down, half, taps)
        assert np.all(np.abs(y[b, :n_out[b]] - want) <= (K + 1) * 2.0 ** -24 * mag), (sr, b)
        assert np.all(y[b, n_out[b]:] == 0)


def _trim_batch():
    cases = R.trim_cases()
    lengths = [len(x) for _, x in cases]
    y = np.full((len(cases), max(lengths) + 300), np.nan, dtype=np.float32)
    for b, (_, x) in enumerate(cases):
        y[b, :len(x)] = x
    return cases, y, lengths


@pytest.mark.parametrize('top_db,pad_frames', [(40.0, 2), (40.0, 0), (70.0, 2), (20.0, 5)])
def test_trim_bounds_equal_the_reference(top_db, pad_frames):
    import t2v_hip
    cases, y, lengths = _trim_batch()
    want = []
    for name, x in cases:
        start, end, margin = R.trim_bounds(x, top_db, pad_frames)
        assert margin > 1e-3, (name, margin)       # an fp32 sum of 1024 squares is off by 6e-5 at most: no frame is a toss-up
        want.append([start, end])
    got = t2v_hip.trim_bounds(torch.from_numpy(y).cuda(), lengths, top_db, pad_frames)
    assert got.dtype == torch.int32 and got.is_cuda and got.cpu().tolist() == want
    for b, n in enumerate(lengths):                # and a row alone
        alone = t2v_hip.trim_bounds(torch.from_numpy(y[b:b + 1, :n].copy()).cuda(), [n], top_db, pad_frames)
        assert alone.cpu().tolist() == [want[b]]


def test_crop_equals_numpy():
    import t2v_hip
    rng = np.random.RandomState(3)
    y = rng.uniform(-0.9, 0.9, (4, 1000)).astype(np.float32)
    y[1, 100:110] = (1.0, -1.0, 1.3, -1.3, 32767.4 / 32768, 32767.6 / 32768, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 2.5 / 32768)
    y[1, 700] = 7.0                                                    # outside row 1's bounds: not counted
    bounds = [[0, 1000], [90, 600], [257, 258], [512, 512]]
    for bd in (bounds, torch.tensor(bounds, dtype=torch.int32).cuda()):
        out, counts = t2v_hip.crop(torch.from_numpy(y).cuda(), bd)
        assert counts == [1000, 510, 1, 0] and out.dtype == torch.float32 and tuple(out.shape) == (4, 1000)
        out = out.cpu().numpy()
        for b, (s, e) in enumerate(bounds):
            assert out[b, :e - s].tobytes() == y[b, s:e].tobytes() and np.all(out[b, e - s:] == 0)
    pcm, counts, stats = t2v_hip.crop(torch.from_numpy(y).cuda(), bounds, pcm16=True, return_stats=True)
    assert pcm.dtype == torch.int16 and counts == [1000, 510, 1, 0]
    pcm = pcm.cpu().numpy()
    for b, (s, e) in enumerate(bounds):
        want, clipped, peak = R.crop_pcm16(y[b], s, e)
        assert pcm[b, :e - s].tobytes() == want.tobytes() and np.all(pcm[b, e - s:] == 0), b
        assert stats[b] == (clipped, float(peak)), (b, stats[b], clipped, peak)
    assert stats[1][0] == 4 and stats[1][1] == float(np.float32(1.3)) and stats[3] == (0, 0.0)
    assert _bits(t2v_hip.crop(torch.from_numpy(y).cuda(), bounds, pcm16=True)[0]) == pcm.tobytes()


def _tone_wav(path, sr, seconds, head, tail, freq, seed):
    """int16 wav: noise 55 dB down for head / tail seconds around a tone"""
    from scipy.io.wavfile import write
    rng = np.random.RandomState(seed)
    n0, n1, n2 = int(head * sr), int(seconds * sr), int(tail * sr)
    x = np.concatenate([1e-3 * rng.uniform(-1, 1, n0), 0.5 * np.sin(2 * np.pi * freq * np.arange(n1) / sr),
                        1e-3 * rng.uniform(-1, 1, n2)])
    s = np.round(x * 32767).astype(np.int16)
    write(str(path), sr, s)
    return s


def test_synthesizer_end_to_end(tmp_path):
    import t2v_hip
    from synthesizer import Synthesizer
    p48, p16 = str(tmp_path / 'a48.wav'), str(tmp_path / 'b16.wav')
    s48 = _tone_wav(p48, 48000, 0.15, 0.08, 0.11, 330.0, 1)
    s16 = _tone_wav(p16, 16000, 0.2, 0.1, 0.05, 180.0, 2)
    syn = Synthesizer(resample=True, trim_db=40)
    mels, frames = syn.load_mels([p48, p16])
    # by hand
    y48, n48 = t2v_hip.resample(torch.from_numpy(s48[None]).cuda(), [len(s48)], 48000, 16000)
    y = torch.zeros(2, max(n48[0], len(s16)), device='cuda')
    y[0, :n48[0]] = y48[0]
    y[1, :len(s16)] = torch.from_numpy(s16.astype(np.float32) / np.float32(32768.0)).cuda()
    n = [n48[0], len(s16)]
    bounds = t2v_hip.trim_bounds(y, n, 40.0, 2)
    cut, counts = t2v_hip.crop(y, bounds)
    assert all(c < k for c, k in zip(counts, n)), (counts, n)           # something was trimmed from both
    want = syn.stft.mel_spectrogram(cut, torch.tensor(counts, dtype=torch.int64))
    assert frames == [c // 256 + 1 for c in counts]
    assert tuple(mels.shape) == tuple(want.shape) and _bits(mels) == _bits(want)
    yy, nn = syn.load_wavs([p48, p16])
    assert nn == counts and _bits(yy) == _bits(cut)
    one = syn.load_mel(p48)
    assert _bits(one[0]) == _bits(mels[0, :, :frames[0]])
    assert syn.wav_lengths([p48, p16]) == n
    # resample only: the counts are the resampled ones
    assert Synthesizer(resample=True).load_wavs([p16, p48])[1] == [n[1], n[0]]
    # the default is unchanged
    with pytest.raises(ValueError, match="48000 SR doesn't match target 16000 SR"):
        Synthesizer().load_wavs([p48, p16])
    with pytest.raises(ValueError, match="SR doesn't match"):
        Synthesizer(trim_db=40).load_mels([p16, p48])


def test_prepare_corpus_end_to_end(tmp_path):
    import prepare_corpus as PC
    import t2v_hip
    from scipy.io.wavfile import read
    src = tmp_path / 'src'
    (src / 's1').mkdir(parents=True)
    (src / 's2').mkdir()
    specs = [(str(src / 's1' / 'u.wav'), 48000, 3), (str(src / 's2' / 'u.wav'), 44100, 4), (str(src / 'v.wav'), 16000, 5)]
    samples = [_tone_wav(p, sr, 0.12, 0.07, 0.09, 200.0 + 50 * seed, seed) for p, sr, seed in specs]
    stereo = str(src / 'stereo.wav')
    from scipy.io.wavfile import write
    write(stereo, 16000, np.zeros((500, 2), dtype=np.int16))
    filelist = tmp_path / 'in.txt'
    filelist.write_text(''.join("%s|text %d|%d|%d\n" % (p, i, i, i % 4) for i, (p, _, _) in enumerate(specs))
                        + stereo + "|skipped|9|0\n", encoding='utf-8')
    out_dir, out_list, report_path = tmp_path / 'out', tmp_path / 'out.txt', tmp_path / 'rep.json'
    PC.main(['--filelist_path', str(filelist), '--out_dir', str(out_dir), '--out_filelist', str(out_list), '--report',
             str(report_path), '--batch_size', '2'])
    names = ['s1_u.wav', 's2_u.wav', 'v.wav']
    lines = out_list.read_text(encoding='utf-8').splitlines()
    assert lines == ["%s|text %d|%d|%d" % (os.path.join(str(out_dir), names[i]), i, i, i % 4) for i in range(3)]
    report = json.loads(report_path.read_text(encoding='utf-8'))
    assert report['n_rows'] == 4 and report['n_written'] == 3 and report['n_skipped'] == 1
    assert 'channels' in report['rows'][3]['skipped']
    assert set(report['by_source_rate']) == {'48000', '44100', '16000'}
    for i, (p, sr, _) in enumerate(specs):
        y, n = t2v_hip.resample(torch.from_numpy(samples[i][None]).cuda(), [len(samples[i])], sr, 16000)
        bounds = t2v_hip.trim_bounds(y, n, 40.0, 2)
        pcm, counts, stats = t2v_hip.crop(y, bounds, pcm16=True, return_stats=True)
        rate, got = read(os.path.join(str(out_dir), names[i]))
        assert rate == 16000 and got.dtype == np.int16 and got.tobytes() == pcm[0, :counts[0]].cpu().numpy().tobytes(), i
        rec = report['rows'][i]
        start, end = bounds.cpu().tolist()[0]
        assert rec['source_rate'] == sr and rec['samples_in'] == len(samples[i]) and rec['samples_out'] == counts[0] < n[0]
        assert rec['trimmed_head_s'] == start / 16000.0 and rec['trimmed_tail_s'] == (n[0] - end) / 16000.0
        assert rec['peak'] == stats[0][1] and rec['clipped_samples'] == stats[0][0] and rec['all_silent'] is False
        assert rec['trimmed_head_s'] > 0 and rec['trimmed_tail_s'] > 0
        tot = report['by_source_rate'][str(sr)]
        assert tot['rows'] == 1 and tot['seconds_in'] == pytest.approx(len(samples[i]) / float(sr))


def test_bad_arguments_raise_and_the_library_stays_usable():
    import t2v_hip
    x = torch.zeros(2, 600, device='cuda')
    good = lambda: t2v_hip.resample(x, [600, 300], 48000, 16000)
    for call, exc in ((lambda: t2v_hip.resample(x.cpu(), [600, 300], 48000, 16000), t2v_hip.T2VHipError),
                      (lambda: t2v_hip.resample(x.double(), [600, 300], 48000, 16000), ValueError),
                      (lambda: t2v_hip.resample(x[0], [600], 48000, 16000), ValueError),
                      (lambda: t2v_hip.resample(x, [600, 601], 48000, 16000), ValueError),
                      (lambda: t2v_hip.resample(x, [600, 0], 48000, 16000), ValueError),
                      (lambda: t2v_hip.resample(x, [600], 48000, 16000), ValueError),
                      (lambda: t2v_hip.resample(x, [600, 300], 44056, 16000), ValueError),
                      (lambda: t2v_hip.resample(x, [600, 300], 0, 16000), ValueError),
                      (lambda: t2v_hip.trim_bounds(x.cpu(), [600, 300]), t2v_hip.T2VHipError),
                      (lambda: t2v_hip.trim_bounds(x, [600, 300], top_db=0.0), ValueError),
                      (lambda: t2v_hip.trim_bounds(x, [600, 300], pad_frames=-1), ValueError),
                      (lambda: t2v_hip.trim_bounds(x, [600, 700]), ValueError),
                      (lambda: t2v_hip.trim_bounds(x.short(), [600, 300]), ValueError),
                      (lambda: t2v_hip.crop(x.cpu(), [[0, 1], [0, 1]]), t2v_hip.T2VHipError),
                      (lambda: t2v_hip.crop(x, [[0, 601], [0, 1]]), ValueError),
                      (lambda: t2v_hip.crop(x, [[5, 4], [0, 1]]), ValueError),
                      (lambda: t2v_hip.crop(x, [[0, 1]]), ValueError),
                      (lambda: t2v_hip.crop(x, [[0.0, 1.0], [0.0, 1.0]]), ValueError),
                      (lambda: t2v_hip.crop(x, [[0, 1], [0, 1]], return_stats=True), ValueError)):
        with pytest.raises(exc):
            call()
        y, n = good()
        assert n == [200, 100] and float(y.abs().max()) == 0.0
    # the C ABI's own refusals: a short output stride, a table above the limit
    lib = t2v_hip.load_library()
    n = torch.tensor([600, 300], dtype=torch.int32, device='cuda')
    taps = torch.zeros(97, device='cuda')
    y = torch.zeros(2, 200, device='cuda')
    args = lambda stride, half: (t2v_hip._p(x), 0, 1.0, t2v_hip._p(n), 600, 2, t2v_hip._p(taps), 1, 3, half, t2v_hip._p(y), stride,
                                 t2v_hip._stream())
    assert lib.t2v_resample(*args(199, 48)) == -2                       # T2V_ERR_ARG
    assert lib.t2v_resample(*args(200, 16384)) == -1                    # T2V_ERR_DIMS: 32 769 taps
    assert lib.t2v_resample(*args(200, 48)) == 0
    torch.cuda.synchronize()
    assert good()[1] == [200, 100]
    assert t2v_hip.trim_bounds(x, [600, 300]).cpu().tolist() == [[0, 600], [0, 300]]
