"""CPU side of the ragged reference encoder: the length grouping of Synthesizer.latents and the latent-export command line."""
import os

import numpy as np
import pytest


def test_length_groups_cover_every_index_once_longest_first():
    from synthesizer import length_groups
    rng = np.random.RandomState(3)
    lengths = [int(x) for x in rng.randint(1, 50, size=37)]
    for bs in (1, 4, 16, 37, 64):
        groups = length_groups(lengths, bs)
        flat = [i for g in groups for i in g]
        assert sorted(flat) == list(range(len(lengths)))
        assert all(1 <= len(g) <= bs for g in groups) and len(groups) == -(-len(lengths) // bs)
        assert [lengths[i] for i in flat] == sorted(lengths, reverse=True)
        # results laid out group after group go back to input order through the inverse permutation
        values = np.array([10 * lengths[i] + i for i in flat])
        inv = np.empty(len(flat), dtype=np.int64)
        inv[flat] = np.arange(len(flat))
        assert values[inv].tolist() == [10 * lengths[i] + i for i in range(len(lengths))]


def test_length_groups_ties_keep_input_order_and_bad_batch_size_raises():
    from synthesizer import length_groups
    assert length_groups([5, 3, 5, 3, 5], 2) == [[0, 2], [4, 1], [3]]
    assert length_groups([], 4) == []
    with pytest.raises(ValueError):
        length_groups([1, 2], 0)


def test_extract_latents_arguments():
    import extract_latents as X
    a = X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz'])
    assert (a.load_path, a.filelist_path, a.out, a.batch_size, a.hparams) == ('ck', 'f.txt', 'o.npz', 64, '')
    a = X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz', '--batch_size', '8',
                      '--hparams', 'z_latent_dim=16'])
    assert a.batch_size == 8 and a.hparams == 'z_latent_dim=16'
    with pytest.raises(SystemExit):
        X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz', '--batch_size', '0'])
    with pytest.raises(SystemExit):
        X.parse_args(['--load_path', 'ck', '--filelist_path', 'f.txt'])          # --out is required


def test_extract_latents_reads_the_filelist_rows(tmp_path):
    import extract_latents as X
    fl = tmp_path / 'list.txt'
    fl.write_text("a.wav|안녕|0|2\n\nb.wav|네|1|0\n", encoding='utf-8')
    paths, emotions = X.read_filelist(str(fl))
    assert paths == ['a.wav', 'b.wav'] and emotions.tolist() == [2, 0] and emotions.dtype == np.int64


def test_wav_num_samples_reads_the_header(tmp_path):
    from scipy.io.wavfile import write
    from synthesizer import wav_num_samples
    p = str(tmp_path / 'x.wav')
    write(p, 16000, np.zeros(12345, dtype=np.int16))
    assert wav_num_samples(p) == 12345 and os.path.exists(p)
