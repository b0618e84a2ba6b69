"""The resampler's definition, taps and trim in fp64 on the CPU (resample_ref.py), the host side of t2v_hip.resample_taps, and
prepare_corpus.py's argument handling, filelist rewriting and output names.  The kernels are checked against the same
reference in test_resample_gpu.py."""
import math
import os

import numpy as np
import pytest

import resample_ref as R


@pytest.mark.parametrize('sr', R.RATES)
def test_ref_is_scipy_resample_poly(sr):
    from scipy.signal import resample_poly
    up, down, half, g = R.window(sr, 16000)
    rng = np.random.RandomState(sr)
    for n in R.LENGTHS:
        x = rng.randn(n)
        y, mag, cnt = R.resample(x, up, down, half, up * g)
        want = resample_poly(x, up, down, window=g)
        assert len(y) == len(want) == -((-n * up) // down)
        assert np.max(np.abs(y - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), (sr, n)
        assert np.all(mag >= np.abs(y) - 1e-15) and cnt.max() <= R.taps_per_phase(up, half)


@pytest.mark.parametrize('sr', R.RATES)
def test_taps_of_t2v_hip_are_the_windowed_sinc(sr):
    import t2v_hip
    up, down, half, taps = t2v_hip.resample_taps(sr, 16000)
    rup, rdown, rhalf, g = R.window(sr, 16000)
    assert (up, down, half) == (rup, rdown, rhalf) and math.gcd(up, down) == 1 and up * sr == down * 16000
    assert taps.dtype == np.float32 and len(taps) == 2 * half + 1 and not taps.flags.writeable
    assert taps.tobytes() == (up * g).astype(np.float32).tobytes()
    assert abs(g.sum() - 1.0) < 1e-12 and np.array_equal(taps, taps[::-1])
    assert abs(float(taps.astype(np.float64).sum()) / up - 1.0) < 1e-6
    assert t2v_hip.resample_taps(sr, 16000)[3] is taps                  # cached per argument tuple
    assert t2v_hip.resample_taps(sr * 3, 48000)[:3] == (up, down, half)  # the ratio is reduced


@pytest.mark.parametrize('sr', R.RATES)
def test_tones_through_the_fp32_taps(sr):
    """a 1 kHz tone comes through to 1e-4 (3.7e-5 at the worst rate); 9 kHz in a 48 kHz input is down 90 dB (96.8 measured)"""
    import t2v_hip
    up, down, half, taps = t2v_hip.resample_taps(sr, 16000)
    n = sr // 4
    y, _, _ = R.resample(np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr), up, down, half, taps)
    edge = half // down + 2                                             # outputs whose taps reach past the ends
    m = np.arange(len(y))[edge:-edge]
    err = np.max(np.abs(y[edge:-edge] - np.sin(2 * np.pi * 1000.0 * m / 16000.0)))
    print("%d Hz: 1 kHz tone error %.3g" % (sr, err))
    assert err <= 1e-4
    if sr == 48000:
        y, _, _ = R.resample(np.sin(2 * np.pi * 9000.0 * np.arange(n) / sr), up, down, half, taps)
        db = 20 * np.log10(np.max(np.abs(y[edge:-edge])))
        print("9 kHz in 48 kHz: %.1f dB" % db)
        assert db <= -90.0


def test_table_limit_and_bad_rates():
    import t2v_hip
    with pytest.raises(ValueError, match="2000/5507"):
        t2v_hip.resample_taps(44056, 16000)
    for a, b in ((0, 16000), (16000, -1), (44100.5, 16000), (True, 16000)):
        with pytest.raises(ValueError):
            t2v_hip.resample_taps(a, b)
    with pytest.raises(ValueError):
        t2v_hip.resample_taps(48000, 16000, zeros=0)
    assert t2v_hip.resample_taps(96000, 22050)[2] == 10240              # the largest table among the common rates: 20 481
    assert t2v_hip.resample_taps(16000, 16000)[:2] == (1, 1)
    assert [t2v_hip.resample_length(n, 160, 441) for n in (1, 441, 442, 705, 706)] == [1, 160, 161, 256, 257]


def test_trim_ref_on_the_constructed_signals():
    got = {name: R.trim_bounds(x) for name, x in R.trim_cases()}
    for name, (start, end, margin) in got.items():
        print(name, start, end, margin)
        assert margin > 1e-3, name
    # tone on [1500, 4500) of 5777: frames 4..19 overlap it (frame t covers [256 t - 512, 256 t + 512)) -> 256 (4 - 2), 256 (19 + 3)
    assert got['silence_tone_silence'][:2] == (512, 5632)
    # tone on [1300, 2801): frames 4..10 overlap it, 10 = n // 256 is the last frame
    assert got['sound_to_the_last_sample'][:2] == (512, 2801)
    assert got['all_zero'][:2] == (0, 1500)
    assert got['one_sample'][:2] == (0, 1)
    x = dict(R.trim_cases())['silence_tone_silence']
    assert R.trim_bounds(x, pad_frames=0)[:2] == (1024, 5120)
    assert R.trim_bounds(x, top_db=70.0)[:2] == (0, 5777)               # the noise sounds at 70 dB: nothing to cut


def test_crop_ref_rounds_to_even_and_clamps():
    y = np.array([0.0, 0.5 / 32768, 1.5 / 32768, -1.0, 1.0, -1.2, 0.99999], dtype=np.float32)
    pcm, clipped, peak = R.crop_pcm16(y, 1, 7)
    assert pcm.tolist() == [0, 2, -32768, 32767, -32768, 32767] and clipped == 3 and peak == np.float32(1.2)


# ---------------------------------------------------------------------- prepare_corpus.py, host side
def test_prepare_corpus_parser():
    import prepare_corpus as PC
    a = PC.parse_args(['--filelist_path', 'f.txt', '--out_dir', 'd', '--out_filelist', 'g.txt'])
    assert (a.sampling_rate, a.trim_db, a.no_trim, a.pad_frames, a.batch_size) == (16000, 40.0, False, 2, 64)
    assert a.report == os.path.join('d', 'report.json')
    a = PC.parse_args(['--filelist_path', 'f.txt', '--out_dir', 'd', '--out_filelist', 'g.txt', '--no_trim', '--sampling_rate',
                       '22050', '--report', 'r.json', '--batch_size', '3', '--pad_frames', '0'])
    assert (a.sampling_rate, a.no_trim, a.report, a.batch_size, a.pad_frames) == (22050, True, 'r.json', 3, 0)
    base = ['--filelist_path', 'f.txt', '--out_dir', 'd', '--out_filelist', 'g.txt']
    for bad in (['--trim_db', '30', '--no_trim'], ['--batch_size', '0'], ['--trim_db', '-3'], ['--pad_frames', '-1'],
                ['--sampling_rate', '0'], []):
        with pytest.raises(SystemExit):
            PC.parse_args((base if bad else []) + bad)
    assert callable(PC.main)


def test_prepare_corpus_rewrites_the_filelist(tmp_path):
    import prepare_corpus as PC
    f = tmp_path / 'list.txt'
    f.write_text("a/x.wav|안녕|3|1\n\nb/y.wav|two|words|0|extra\nc/z.wav\n", encoding='utf-8')
    rows = PC.read_rows(str(f))
    assert rows == [['a/x.wav', '안녕', '3', '1'], ['b/y.wav', 'two', 'words', '0', 'extra'], ['c/z.wav']]
    lines = PC.rewrite_rows(rows, ['out/x.wav', None, 'out/z.wav'])
    assert lines == ['out/x.wav|안녕|3|1', 'out/z.wav']


def test_prepare_corpus_output_names_are_unique():
    import prepare_corpus as PC
    names = PC.output_names(['a/x.wav', 'b/x.wav', 'c/y.wav', 'q/a/x.wav', 'z.wav', 'z.wav', 'x.flac.wav'])
    assert names == ['a_x.wav', 'b_x.wav', 'y.wav', 'q_a_x.wav', 'z.wav', 'z_1.wav', 'x.flac.wav']
    assert PC.output_names(['s1/a.wav', 's2/a.wav']) == ['s1_a.wav', 's2_a.wav']
    many = ['d%d/u.wav' % (i % 3) for i in range(7)] + ['u_1.wav']
    assert len(set(PC.output_names(many))) == len(many)


def test_wav_switches_on_the_three_command_lines():
    import evaluate
    import extract_latents
    import synthesizer
    from wavio import wav_options
    cases = ((synthesizer, ['--load_path', 'c']), (evaluate, ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']),
             (extract_latents, ['--load_path', 'c', '--filelist_path', 'f', '--out', 'o']))
    for mod, base in cases:
        a = mod.build_arg_parser().parse_args(base)
        assert wav_options(a) == dict(resample=False, trim_db=None), mod.__name__
        a = mod.build_arg_parser().parse_args(base + ['--resample', '--trim_db', '35'])
        assert wav_options(a) == dict(resample=True, trim_db=35.0), mod.__name__
        with pytest.raises(SystemExit):
            wav_options(mod.build_arg_parser().parse_args(base + ['--trim_db', '0']))


def test_default_synthesizer_still_refuses_another_rate(tmp_path):
    """the default stays the reference's: a 22 050 Hz wav is a ValueError before anything reaches the device"""
    from scipy.io.wavfile import write
    from synthesizer import Synthesizer
    p = str(tmp_path / 'sr22k.wav')
    write(p, 22050, np.zeros(3000, dtype=np.int16))
    syn = Synthesizer()
    assert syn.resample is False and syn.trim_db is None
    for call in (syn.load_mel, lambda q: syn.load_wavs([q]), lambda q: syn.load_mels([q])):
        with pytest.raises(ValueError, match="22050 SR doesn't match target 16000 SR"):
            call(p)
    assert Synthesizer(resample=True).wav_lengths([p]) == [-((-3000 * 320) // 441)]
    assert syn.wav_lengths([p]) == [3000]
    for bad in (0, -5.0, float('inf')):
        with pytest.raises(ValueError):
            Synthesizer(trim_db=bad)


def test_read_wav_formats(tmp_path):
    from scipy.io.wavfile import write
    from wavio import read_wav, wav_header
    s16 = np.array([0, 1, -32768, 32767], dtype=np.int16)
    write(str(tmp_path / 'a.wav'), 44100, s16)
    rate, data = read_wav(str(tmp_path / 'a.wav'))
    assert rate == 44100 and data.dtype == np.int16 and data.tolist() == s16.tolist()
    assert wav_header(str(tmp_path / 'a.wav')) == (44100, 4, 1)
    write(str(tmp_path / 'b.wav'), 48000, np.array([0, 1 << 30, -(1 << 31)], dtype=np.int32))
    rate, data = read_wav(str(tmp_path / 'b.wav'))
    assert rate == 48000 and data.dtype == np.float32 and data.tolist() == [0.0, 0.5, -1.0]
    write(str(tmp_path / 'c.wav'), 8000, np.array([0.25, -0.5], dtype=np.float32))
    assert read_wav(str(tmp_path / 'c.wav'))[1].tolist() == [0.25, -0.5]
    write(str(tmp_path / 'd.wav'), 16000, np.zeros((10, 2), dtype=np.int16))
    assert wav_header(str(tmp_path / 'd.wav')) == (16000, 10, 2)
    with pytest.raises(ValueError, match="2 channels"):
        read_wav(str(tmp_path / 'd.wav'))
