"""The host side of the resident corpus (corpus.py): the tables against TextMelLoader, the checks of outside input, the
collate's host plan against DeviceFrontendCollate, the views under the bucketed sampler, and the switch in train.py.  No GPU:
nothing here touches the device store."""
import os
import struct

import numpy as np
import pytest
import torch

import resident_ref as R
from corpus import ResidentCollate, ResidentCorpus
from data_utils import BucketBatchSampler, DeviceFrontendCollate, TextMelLoader


@pytest.fixture(scope='module')
def made(tmp_path_factory):
    root = tmp_path_factory.mktemp('resident')
    train_list, val_list, rows = R.write_corpus(root)
    hp = R.hparams(train_list, val_list)
    corpus = ResidentCorpus([train_list, val_list], hp, build=False)
    return dict(root=str(root), train=train_list, val=val_list, rows=rows, hp=hp, corpus=corpus)


def test_the_test_corpus_has_the_ties_and_spread_the_tests_rely_on(made):
    c = made['corpus']
    by_path = {p: i for i, p in enumerate(c.paths)}
    n_ids = [int(c.n_ids[by_path[r[0]]]) for r in made['rows']]
    n_frames = [int(c.n_frames[by_path[r[0]]]) for r in made['rows']]
    assert n_frames == [3, 3, 4, 4, 5, 9, 11, 16, 17]
    assert n_ids[1] == n_ids[2] and n_ids[3] == n_ids[4] and n_ids[1] != n_ids[3]
    assert max(n_ids) == n_ids[5] and n_ids.count(n_ids[5]) == 1 and n_frames[5] != max(n_frames)
    assert min(n_ids) == n_ids[0]


@pytest.mark.parametrize('k', [0, 1], ids=['training', 'validation'])
def test_tables_equal_textmelloader_item_by_item(made, k):
    c, hp = made['corpus'], made['hp']
    loader = TextMelLoader(made['train'] if k == 0 else made['val'], hp, stft=object())
    view = c.view(k)
    assert len(view) == len(loader) == (R.N_TRAIN, 9 - R.N_TRAIN)[k]
    assert c.bounds == [0, R.N_TRAIN, 9] and len(c) == 9
    for i in range(len(loader)):
        path, text, speaker, emotion = loader.audiopaths_and_text[i][:4]
        u = view[i]
        assert type(u) is int and u == c.bounds[k] + i
        assert c.paths[u] == path                                       # the order after the seed-1234 shuffle
        ids = loader.get_text(text)
        assert c.ids[u].dtype == np.int32 and c.ids[u].tolist() == ids.tolist() and int(c.n_ids[u]) == ids.numel()
        assert loader.get_speaker(speaker).tolist() == [float(j == c.speaker[u]) for j in range(hp.n_speakers)]
        assert loader.get_emotion(emotion).tolist() == [float(j == c.emotion[u]) for j in range(hp.n_emotions)]
        assert int(c.n_samples[u]) == dict((r[0], n) for r, n in zip(made['rows'], R.SAMPLES))[path]
        assert int(c.n_frames[u]) == int(c.n_samples[u]) // hp.hop_length + 1
    assert view.lengths() == loader.lengths() and all(type(n) is int for n in view.lengths())
    assert view.text_lengths() == loader.text_lengths() and all(type(n) is int for n in view.text_lengths())
    with pytest.raises(IndexError):
        view[len(view)]


def _list_of(tmp_path, line):
    fl = tmp_path / 'bad.txt'
    good = tmp_path / 'good.wav'
    R.write_wav(str(good), 1000, 1)
    fl.write_text("%s|가|0|0\n%s\n" % (good, line), encoding='utf-8')
    return str(fl)


def _float_wav(path, n):
    """a RIFF file with format tag 3 (IEEE float), which is not PCM"""
    data = np.zeros(n, dtype='<f4').tobytes()
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(data)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 3, 1, 16000, 64000, 4, 32))
        f.write(b'data' + struct.pack('<I', len(data)) + data)


def test_rejected_input_raises_the_named_error_and_names_the_row(made, tmp_path):
    from scipy.io.wavfile import write
    hp = made['hp']
    wav = lambda name: str(tmp_path / name)
    write(wav('rate.wav'), 22050, np.zeros(4000, dtype=np.int16))
    write(wav('wide.wav'), 16000, np.zeros(4000, dtype=np.int32))
    write(wav('byte.wav'), 16000, np.zeros(4000, dtype=np.uint8))
    _float_wav(wav('float.wav'), 4000)
    write(wav('short.wav'), 16000, np.zeros(512, dtype=np.int16))
    write(wav('ok.wav'), 16000, np.zeros(513, dtype=np.int16))
    cases = [
        ("%s|가|0|0" % wav('rate.wav'), ValueError, "SR doesn't match target"),
        ("%s|가|0|0" % wav('wide.wav'), ValueError, "16-bit PCM"),
        ("%s|가|0|0" % wav('byte.wav'), ValueError, "16-bit PCM"),
        ("%s|가|0|0" % wav('float.wav'), ValueError, "16-bit PCM"),
        ("%s|가|0|0" % wav('short.wav'), ValueError, "512"),
        ("%s|가|1|0" % wav('ok.wav'), ValueError, "speaker index 1 outside the one-hot width 1"),
        ("%s|가|0|4" % wav('ok.wav'), ValueError, "emotion index 4 outside the one-hot width 4"),
        ("%s|가|0|-1" % wav('ok.wav'), ValueError, "emotion index -1"),
        ("%s|가|0" % wav('ok.wav'), ValueError, "path|text|speaker|emotion"),
    ]
    for line, error, match in cases:
        fl = _list_of(tmp_path, line)
        with pytest.raises(error, match=match) as ei:
            ResidentCorpus([fl], hp, build=False)
        assert "%s row 2" % fl in str(ei.value), (line, str(ei.value))          # the filelist and the row, from 1
        if line.count('|') == 3:
            assert line.split('|')[0] in str(ei.value)                          # and the wav
    # a symbol id outside the embedding: the IndexError of BatchLayout.check_ids, with the row
    import hparams as HP
    small = HP.create_hparams("n_symbols=3")
    fl = _list_of(tmp_path, "%s|가|0|0" % wav('ok.wav'))
    with pytest.raises(IndexError, match="symbol id out of range") as ei:
        ResidentCorpus([fl], small, build=False)
    assert "%s row 1" % fl in str(ei.value) and "embedding has 3 rows" in str(ei.value)
    # the same lists are taken when nothing is wrong with them
    assert len(ResidentCorpus([_list_of(tmp_path, "%s|가|0|3" % wav('ok.wav'))], hp, build=False)) == 2


def test_another_mel_width_is_refused_by_name(made):
    hp = R.hparams(made['train'], made['val'], "n_mel_channels=64")
    corpus = ResidentCorpus([made['val']], hp, build=False)
    with pytest.raises(ValueError, match="80 mel channels, hparams.n_mel_channels is 64"):
        corpus.build_store()


class _ZeroFrontend(object):
    """stands in for TacotronSTFT in DeviceFrontendCollate: the plan under test does not depend on the mel values"""

    def mel_spectrogram(self, wav, lengths=None, scale=1.0):
        return torch.zeros(wav.size(0), 80, int(lengths.max()) // 256 + 1)


INDEX_LISTS = ([0], [1, 2], [2, 1], [3, 4, 1, 2], [4, 3, 5, 0, 2, 1], [5, 5, 0], [8, 6, 7], [0, 8], [6, 1, 2, 7, 3, 4, 5], [1, 2, 1])


@pytest.mark.parametrize('r', [1, 2], ids=['r1', 'r2'])
def test_host_plan_equals_device_frontend_collate(made, monkeypatch, r):
    """DeviceFrontendCollate itself, run on the host: its device is swapped for the CPU and its front end for zeros.  Index lists
    are positions in the nine file-order rows and hold the tied pairs (1, 2) and (3, 4) in both orders, a repeated row, the
    first and the last utterance of the store and rows of both lists."""
    import hparams as HP
    c = made['corpus']
    hp = HP.create_hparams("n_frames_per_step=%d" % r)
    by_path = {p: i for i, p in enumerate(c.paths)}
    loaders = [TextMelLoader(made[k], hp, stft=object(), return_audio=True) for k in ('train', 'val')]
    items = {}
    for k, loader in enumerate(loaders):
        for i in range(len(loader)):
            items[c.bounds[k] + i] = loader[i]
    # data_utils calls `torch.device('cuda')` through the torch module, so the name can only be swapped there.  A lambda in its
    # place would break an `isinstance(x, torch.device)`; between here and the end of the test only DeviceFrontendCollate's
    # .to(dev) / arange(device=dev), ResidentCollate.plan and tensor comparisons run, which hand the real device object on and
    # never test for the type, the items were made above, and monkeypatch puts the class back when the test ends
    real = torch.device
    monkeypatch.setattr(torch, 'device', lambda *a, **kw: real('cpu'))
    reference = DeviceFrontendCollate(hp, stft=_ZeroFrontend())
    collate = ResidentCollate(c, hp)
    lists = [[by_path[made['rows'][j][0]] for j in rows] for rows in INDEX_LISTS] + [[0, len(c) - 1], list(range(len(c)))]
    for batch in lists:
        text, input_lengths, mel, gate, output_lengths, speakers, emotions = reference([items[u] for u in batch])
        got_lengths, rows, T_in, T_out = collate.plan(batch)
        assert got_lengths.dtype == torch.int64 and not got_lengths.is_cuda and torch.equal(got_lengths, input_lengths)
        assert T_in == text.size(1) and T_out == mel.size(2) == gate.size(1) and T_out % r == 0
        assert [int(c.n_frames[u]) for u in rows] == output_lengths.tolist()
        for row, u in enumerate(rows):              # the order, ties included: tied rows hold different ids
            assert text[row, :int(c.n_ids[u])].tolist() == c.ids[u].tolist()
            assert emotions[row].tolist() == [int(j == c.emotion[u]) for j in range(hp.n_emotions)]
    for bad in ([], [-1], [len(c)], [0, 99]):
        with pytest.raises(ValueError):
            collate.plan(bad)


@pytest.mark.parametrize('world,rank', [(1, 0), (2, 1)])
def test_bucket_sampler_from_a_view_equals_the_one_from_textmelloader(made, world, rank):
    loader = TextMelLoader(made['train'], made['hp'], stft=object())
    view = made['corpus'].view(0)
    make = lambda ds: BucketBatchSampler(ds.lengths(), 2 // world, world_size=world, rank=rank, seed=7, window=2,
                                         text_lengths=ds.text_lengths(), text_cap=8)
    a, b = make(view), make(loader)
    for epoch in range(3):
        a.set_epoch(epoch)
        b.set_epoch(epoch)
        assert list(a) == list(b) and len(list(a)) == 3
        assert a.persistent_hit_rate() == b.persistent_hit_rate()


def test_train_parser_knows_the_switch():
    import inspect
    import train as TR
    ap = TR.cli_parser()
    assert ap.parse_args([]).resident_corpus is False
    assert ap.parse_args(['--resident_corpus']).resident_corpus is True
    assert inspect.signature(TR.train).parameters['resident_corpus'].default is False
    assert inspect.signature(TR.prepare_dataloaders).parameters['resident_corpus'].default is False
    import hparams as HP
    assert not hasattr(HP.create_hparams(), 'resident_corpus')          # a switch of the run, not a hyper-parameter


def test_resident_corpus_refuses_mels_from_disk_before_anything_else(monkeypatch):
    import hparams as HP
    import train as TR
    touched = []
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: touched.append('is_available') or False)
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a: touched.append('mem_get_info') or (0, 0))
    hp = HP.create_hparams("load_mel_from_disk=True,training_files=/nonexistent/train.txt,validation_files=/nonexistent/val.txt")
    with pytest.raises(ValueError, match="resident_corpus=True .* load_mel_from_disk=True"):
        TR.prepare_dataloaders(hp, resident_corpus=True)
    assert not touched
