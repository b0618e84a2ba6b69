"""The resident corpus on the GPU: batches of corpus.ResidentCollate (ONE t2v_collate_batch launch over the device store) against
DeviceFrontendCollate on TextMelLoader(return_audio=True) items, through the kernel, the loaders, the engine and train()."""
import ctypes as C
import os
import re

import pytest
import torch

import resident_ref as R

pytestmark = pytest.mark.gpu

NAMES = ('text_padded', 'input_lengths', 'mel_padded', 'gate_padded', 'output_lengths', 'speakers', 'emotions')
# positions in the nine file-order rows of tests/resident_ref.py (rows 0..5 training, 6..8 validation; (1, 2) and (3, 4) tie)
INDEX_LISTS = ([0], [8], [5], [1, 2], [2, 1], [6, 3], [3, 4, 7], [5, 5, 0], [4, 3, 5, 0, 2, 1], [1, 2, 1, 8, 6, 7],
               [6, 1, 2, 7, 3, 4, 5], [0, 1, 2, 3, 4, 5, 8])


@pytest.fixture(scope='module')
def made(tmp_path_factory):
    from corpus import ResidentCorpus
    from data_utils import TextMelLoader
    root = tmp_path_factory.mktemp('resident_gpu')
    train_list, val_list, rows = R.write_corpus(root)
    hp = R.hparams(train_list, val_list)
    corpus = ResidentCorpus([train_list, val_list], hp)
    items = {}
    for k, fl in enumerate((train_list, val_list)):
        loader = TextMelLoader(fl, hp, return_audio=True)
        for i in range(len(loader)):
            items[corpus.bounds[k] + i] = loader[i]
    by_path = {p: i for i, p in enumerate(corpus.paths)}
    return dict(root=str(root), train=train_list, val=val_list, rows=rows, hp=hp, corpus=corpus, items=items,
                globals=[by_path[r[0]] for r in rows])


def _same(got, want, what=''):
    assert len(got) == len(want) == 7
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g.cuda(), w.cuda()), (what, name)


@pytest.mark.parametrize('r', [1, 2], ids=['r1', 'r2'])
def test_batches_equal_device_frontend_collate(made, r):
    """every tensor with torch.equal, the mel bit for bit: both sides are the same front-end kernel on the same samples.  r2
    (n_frames_per_step=2): the frames that round T_out up are 0.0 with gate 1.0."""
    import hparams as HP
    from corpus import ResidentCollate
    from data_utils import DeviceFrontendCollate
    c = made['corpus']
    hp = HP.create_hparams("n_frames_per_step=%d" % r)
    reference, collate = DeviceFrontendCollate(hp), ResidentCollate(c, hp)
    lists = [[made['globals'][j] for j in rows] for rows in INDEX_LISTS] + [[0, len(c) - 1], [len(c) - 1, 0, len(c) - 1]]
    assert sorted(set(len(b) for b in lists)) == [1, 2, 3, 6, 7]
    odd = 0
    for batch in lists:
        want = reference([made['items'][u] for u in batch])
        got = collate(batch)
        assert not got[1].is_cuda and all(t.is_cuda for i, t in enumerate(got) if i != 1)
        _same(got, want, batch)
        T = int(want[4].max())
        if got[2].size(2) > T:
            odd += 1
            assert (got[2][:, :, T:] == 0).all() and (got[3][:, T:] == 1).all()
    assert odd > 0 if r == 2 else odd == 0
    # the store keeps no audio: mels, ids and six small arrays
    assert c.store.nbytes() == c.store_bytes() and c.store.mel.numel() == 80 * int(c.n_frames.sum())


def test_every_element_is_written_and_nothing_else(made):
    import t2v_hip
    c = made['corpus']
    g = made['globals']
    batch = [g[5], g[0], g[8], g[1]]                 # 13..3 symbols, 3..17 frames, unsorted: the kernel takes the order as given
    T_in, T_out = int(c.n_ids[batch].max()) + 3, int(c.n_frames[batch].max()) + 5
    B, guard = len(batch), 64
    shapes = ((B, T_in), (B, 80, T_out), (B, T_out), (B,), (B, c.n_speakers), (B, c.n_emotions))
    bufs, views = [], []
    for shape, (name, dt) in zip(shapes, t2v_hip.COLLATE_OUT):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * guard,), float('nan') if dt.is_floating_point else -1, dtype=dt, device='cuda')
        bufs.append(buf)
        views.append(buf[guard:guard + n].view(shape))
    out = t2v_hip.collate_batch(c.store, batch, T_in, T_out, out=views)
    torch.cuda.synchronize()
    for buf, view, o, (name, dt) in zip(bufs, views, out, t2v_hip.COLLATE_OUT):
        assert o.data_ptr() == view.data_ptr()
        edge = torch.cat([buf[:guard], buf[-guard:]])
        if dt.is_floating_point:
            assert torch.isnan(edge).all(), name
            assert not torch.isnan(view).any(), name
        else:
            assert (edge == -1).all(), name
            assert not (view == -1).any(), name
    text, mel, gate, lengths, speakers, emotions = out
    for row, u in enumerate(batch):
        L, T = int(c.n_ids[u]), int(c.n_frames[u])
        assert text[row, :L].tolist() == c.ids[u].tolist() and (text[row, L:] == 0).all()
        assert (mel[row, :, T:] == 0).all() and (gate[row, :T - 1] == 0).all() and (gate[row, T - 1:] == 1).all()
        off = int(c.store.mel_off[u])
        assert torch.equal(mel[row, :, :T], c.store.mel[off:off + 80 * T].view(80, T))
        assert int(lengths[row]) == T and speakers[row].tolist() == [1]
        assert emotions[row].tolist() == [int(j == c.emotion[u]) for j in range(4)]
    # a second launch into the same memory gives the same bits (no atomics, no dependence on what was there)
    again = t2v_hip.collate_batch(c.store, batch, T_in, T_out)
    for a, b in zip(again, out):
        assert torch.equal(a, b)


def test_argument_checks_through_the_c_abi(made):
    import t2v_abi
    import t2v_hip
    from corpus import ResidentCollate
    lib = t2v_hip.load_library()
    err = t2v_abi.load().define('T2V_ERR_ARG')
    c = made['corpus']
    s = c.store
    B, T_in, T_out = 2, int(c.n_ids.max()), int(c.n_frames.max())
    idx = torch.tensor([0, 1], dtype=torch.int32, device='cuda')
    out = [torch.empty(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(
        ((B, T_in), (B, 80, T_out), (B, T_out), (B,), (B, 1), (B, 4)), t2v_hip.COLLATE_OUT)]
    ptrs = [t.data_ptr() for t in (s.mel, s.mel_off, s.n_frames, s.ids, s.id_off, s.n_ids, s.speaker, s.emotion, idx)]
    ints = [B, s.n_utts, T_in, T_out, 1, 4]
    outs = [t.data_ptr() for t in out]

    def call(ptrs=ptrs, ints=ints, outs=outs):
        return lib.t2v_collate_batch(*([C.c_void_p(p) for p in ptrs] + list(ints) + [C.c_void_p(p) for p in outs] + [None]))

    assert call() == 0
    for i in range(len(ptrs)):
        assert call(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) == err, i
    for i in range(len(outs)):
        assert call(outs=outs[:i] + [None] + outs[i + 1:]) == err, i
    for i in range(len(ints)):                       # B, n_utts, T_in, T_out and both one-hot widths: 0 and negative
        for bad in (0, -1):
            assert call(ints=ints[:i] + [bad] + ints[i + 1:]) == err, (i, bad)
    torch.cuda.synchronize()
    # an index outside the store, or a width that does not cover the batch, is the host's ValueError: nothing is launched
    before = [t.clone() for t in out]
    for bad in ([0, len(c)], [-1, 0], []):
        with pytest.raises(ValueError):
            t2v_hip.collate_batch(s, bad, T_in, T_out, out=out)
        with pytest.raises(ValueError):
            ResidentCollate(c, made['hp'])(bad)
    g = made['globals']
    with pytest.raises(ValueError, match="do not cover"):
        t2v_hip.collate_batch(s, [g[5]], int(c.n_ids[g[5]]) - 1, T_out)
    with pytest.raises(ValueError, match="do not cover"):
        t2v_hip.collate_batch(s, [g[8]], T_in, int(c.n_frames[g[8]]) - 1)
    with pytest.raises(ValueError, match="out="):
        t2v_hip.collate_batch(s, [0, 1], T_in, T_out, out=out[:5] + [out[5].float()])
    torch.cuda.synchronize()
    for a, b in zip(before, out):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_store_that_does_not_fit_names_the_alternative(made, monkeypatch):
    from corpus import ResidentCorpus
    monkeypatch.setattr(ResidentCorpus, 'MAX_FREE_FRACTION', 1e-12)
    with pytest.raises(ValueError, match="device_frontend=True"):
        ResidentCorpus([made['train'], made['val']], made['hp'])
    assert ResidentCorpus([made['train']], made['hp'], build=False).store is None


@pytest.mark.parametrize('bucket', [False, True], ids=['plain', 'bucket_batches'])
def test_loaders_give_equal_batches_over_one_epoch(made, bucket, capsys):
    import train as TR
    extra = "batch_size=2,bucket_batches=%s" % bucket
    want_loader, want_val, want_fn = TR.prepare_dataloaders(R.hparams(made['train'], made['val'], extra + ",device_frontend=True"))
    got_loader, got_val, got_fn = TR.prepare_dataloaders(R.hparams(made['train'], made['val'], extra), resident_corpus=True)
    assert re.search(r"Resident corpus: 9 utterances, 72 frames, \d+\.\d MB on the device, built in \d+\.\d\d s", capsys.readouterr().out)
    assert type(got_loader.batch_sampler).__name__ == type(want_loader.batch_sampler).__name__
    want, got = list(want_loader), list(got_loader)
    assert len(want) == len(got) == 3
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, i)
    # validate() builds its loader from valset and the same collate_fn
    assert len(got_val) == len(want_val) == 3
    _same(got_fn([got_val[i] for i in range(3)]), want_fn([want_val[i] for i in range(3)]), 'validation')


def test_two_engine_steps_leave_identical_arenas(made):
    import train as TR
    arenas = []
    for resident in (False, True):
        hp = R.hparams(made['train'], made['val'], "batch_size=2" + ("" if resident else ",device_frontend=True"))
        torch.manual_seed(hp.seed)
        torch.cuda.manual_seed(hp.seed)
        eng = TR.TrainEngine(hp, graph=False)
        eng.model.vae_gst.eps_override = torch.full((2, 32), 0.125, device='cuda')
        loader, _, _ = TR.prepare_dataloaders(hp, resident_corpus=resident)
        batches = iter(loader)
        losses = [float(eng.step(next(batches), it)[0]) for it in range(2)]
        torch.cuda.synchronize()
        arenas.append((losses, eng.optimizer.params.clone()))
        eng.close()
    assert arenas[0][0] == arenas[1][0]
    assert torch.equal(arenas[0][1], arenas[1][1])


def test_train_loop_prints_the_same_losses_and_writes_a_checkpoint(made, tmp_path, capsys):
    import train as TR
    printed = {}
    for resident in (False, True):
        hp = R.hparams(made['train'], made['val'], "batch_size=2,epochs=1" + ("" if resident else ",device_frontend=True"))
        out = str(tmp_path / ('resident' if resident else 'frontend'))
        TR.train(out, 'logs', None, False, 1, 0, 'group_name', hp, resident_corpus=resident)
        printed[resident] = capsys.readouterr().out
        assert os.path.isfile(os.path.join(out, 'checkpoint_0'))
    assert "Resident corpus: 9 utterances, 72 frames" in printed[True] and "Resident corpus" not in printed[False]
    assert "Validation loss 0:" in printed[True]
    # `Train loss <iteration> <loss> Grad Norm <norm>`: everything but the seconds per iteration
    lines = {k: re.findall(r"^(Train loss \d+ \S+ Grad Norm \S+) ", v, flags=re.M) for k, v in printed.items()}
    assert len(lines[True]) == 3 and lines[True] == lines[False]
