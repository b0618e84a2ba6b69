"""Batched synthesis: a ragged batch of texts comes out item by item as the same texts decoded one at a time — encoder and
Postnet masked to each item's length, per-item stop frames and Prenet dropout seeds in both decode loops."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tacotron2-vae_amd')


@pytest.fixture()
def no_dropout():
    import model as M
    old = M.drop_rate
    M.drop_rate = 0.0
    yield
    M.drop_rate = old


def _model(steps=24):
    import hparams as HP
    import model as M
    hp = HP.create_hparams("max_decoder_steps=%d" % steps)
    torch.manual_seed(hp.seed)
    return M.Tacotron2(hp).cuda().eval()


def _memory(lens, seed, T=None):
    g = torch.Generator().manual_seed(seed)
    T = T or max(lens)
    mem = torch.randn(len(lens), T, 512, generator=g) * 0.5
    for b, L in enumerate(lens):
        mem[b, L:] = 7.0            # garbage past each length: must never be read
    return mem.cuda()


def _gate_logits(dec, mem):
    """gate logits of all max_decoder_steps frames of each item alone (never stopping)"""
    old = dec.gate_threshold
    dec.gate_threshold = 1.0
    try:
        return [dec.inference(m)[1][0, :, 0].cpu() for m in mem]
    finally:
        dec.gate_threshold = old


def _pick_gate_bias(dec, mems):
    """A gate bias under which the items stop on different frames, every logit far from the threshold (the gate row does
    not feed back into the recurrence, so a bias shift moves each item's logits by the same amount)."""
    logits = _gate_logits(dec, mems)
    vals = torch.sort(torch.cat(logits)).values
    best = None
    for i in range(len(vals) - 1):
        c = float(vals[i] + vals[i + 1]) / 2
        stops = []
        for lg in logits:
            f = (lg > c).nonzero()
            stops.append(int(f[0]) if len(f) else len(lg))
        margin = float(vals[i + 1] - vals[i]) / 2
        if len(set(stops)) >= 2 and min(stops) >= 2 and (best is None or margin > best[0]):
            best = (margin, c)
    assert best is not None and best[0] > 1e-4, "no gate bias separates the items"
    with torch.no_grad():
        dec.gate_layer.linear_layer.bias -= best[1]


def _check_items(dec, mem, lens, out, single_kw=None, tol=(2e-5, 2e-5, 2e-6)):
    mel, gate, al, n = out
    B, T_in = mem.size(0), mem.size(1)
    N = int(n.max())
    assert mel.shape == (B, 80, N) and gate.shape == (B, N, 1) and al.shape == (B, N, T_in)
    for b, L in enumerate(lens):
        m1, g1, a1 = dec.inference(mem[b:b + 1, :L], **(single_kw or {}))
        nb = m1.size(2)
        assert int(n[b]) == nb, (b, int(n[b]), nb)
        assert (mel[b, :, :nb] - m1[0]).abs().max().item() < tol[0], b
        assert (gate[b, :nb] - g1[0]).abs().max().item() < tol[1], b
        assert (al[b, :nb, :L] - a1[0]).abs().max().item() < tol[2], b
        # padding convention: mel 0, gate logit 1e3, alignment 0
        assert (mel[b, :, nb:] == 0).all() and (gate[b, nb:] == 1e3).all()
        assert (al[b, nb:] == 0).all() and (al[b, :, L:] == 0).all()


def test_encoder_ragged_batch_matches_each_text_alone(no_dropout):
    m = _model()
    lens = [1, 5, 37, 84, 200]
    g = torch.Generator().manual_seed(3)
    ids = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, L in enumerate(lens):
        ids[b, :L] = torch.randint(1, m.transcript_embedding.weight.size(0), (L,), generator=g)
    ids = ids.cuda()
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    with torch.no_grad():
        out = m.encoder.inference(m.transcript_embedding(ids).transpose(1, 2), lengths)
        assert out.shape == (len(lens), max(lens), 512)
        for b, L in enumerate(lens):
            one = m.encoder.inference(m.transcript_embedding(ids[b:b + 1, :L]).transpose(1, 2))
            assert (out[b, :L] - one[0]).abs().max().item() < 2e-5, b
            assert (out[b, L:] == 0).all(), b
        # the pad symbol's embedding is never read
        m.transcript_embedding.weight[0] += 3.0
        out2 = m.encoder.inference(m.transcript_embedding(ids).transpose(1, 2), lengths)
        assert torch.equal(out, out2)
        # control: the unmasked encoder does read it
        plain = m.encoder.inference(m.transcript_embedding(ids).transpose(1, 2))
        assert (plain[0, :1] - out[0, :1]).abs().max().item() > 1e-3


def test_postnet_ragged_batch_matches_each_mel_alone(no_dropout):
    m = _model()
    lens = [60, 41, 17, 5]
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(len(lens), 80, max(lens), generator=g) * 2 - 4).cuda()
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    with torch.no_grad():
        y = m.postnet(x, lengths)
        xz = x.clone()
        for b, L in enumerate(lens):
            xz[b, :, L:] = 0                     # the decoder's padding convention
        plain = m.postnet(xz)
        leak = 0.0
        for b, L in enumerate(lens):
            one = m.postnet(x[b:b + 1, :, :L])
            assert (y[b, :, :L] - one[0]).abs().max().item() < 2e-5, b
            assert (y[b, :, L:] == 0).all()
            leak = max(leak, (plain[b, :, :L] - one[0]).abs().max().item())
        assert leak > 1e-3          # unmasked, the frames past a short item's end leak into its last frames


@pytest.mark.parametrize("lens,persistent", [((150, 37, 96), None), ((60, 12, 33, 90, 7, 45), False),
                                             ((30, 70, 5, 18, 64, 41, 9, 80, 22, 55, 13), None)],
                         ids=['persistent_B3', 'per_stage_B6', 'groups_B11'])
def test_decoder_batch_matches_each_text_alone(no_dropout, lens, persistent):
    import t2v_hip
    import t2v_oracle as O
    m = _model()
    dec = m.decoder
    mem = _memory(lens, 10 + len(lens))
    if persistent is None and len(lens) <= 4:
        assert t2v_hip.load_library().t2v_decoder_persist_supported(len(lens), max(lens))
    with torch.no_grad():
        _pick_gate_bias(dec, [mem[b:b + 1, :L] for b, L in enumerate(lens)])
        out = dec.inference_batch(mem, lens, persistent=persistent)
        n = out[3]
        assert len(set(n.tolist())) >= 2 and int(n.min()) < dec.max_decoder_steps
        _check_items(dec, mem, lens, out, {'persistent': persistent})
    # one item against the CPU oracle
    b = int(np.argmin([abs(L - 40) for L in lens]))
    L, nb = lens[b], int(n[b])
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    o_mel, o_gate, o_al = O.decoder_inference(sd, mem[b:b + 1, :L].cpu(), max_steps=dec.max_decoder_steps, stop_on_gate=False)
    assert (out[0][b, :, :nb].cpu() - o_mel[0, :, :nb]).abs().max().item() < 2e-4
    assert (out[2][b, :nb, :L].cpu() - o_al[0, :nb]).abs().max().item() < 2e-5


@pytest.mark.parametrize("lens,persistent", [((150, 37, 96), None), ((60, 12, 33, 90, 7), False)],
                         ids=['persistent', 'per_stage'])
def test_decoder_batch_dropout_seeds_are_per_item(lens, persistent):
    """Prenet dropout on: item b with seed s_b is the B = 1 decode with seed s_b, i.e. the inference() call that would have
    drawn s_b; a batch with seeds=None reserves the seeds of B consecutive inference() calls."""
    import model as M
    assert M.drop_rate > 0
    m = _model()
    dec = m.decoder
    dec.gate_threshold = 1.0                     # all frames: the masks of every frame are compared
    mem = _memory(lens, 20)
    with torch.no_grad():
        c0 = dec._calls
        out = dec.inference_batch(mem, lens, persistent=persistent)
        assert dec._calls == c0 + len(lens)
        for b, L in enumerate(lens):
            dec._calls = c0 + b                  # the b-th of the sequential calls draws seed call_seed(c0 + b + 1)
            m1, g1, a1 = dec.inference(mem[b:b + 1, :L], persistent=persistent)
            assert (out[0][b] - m1[0]).abs().max().item() < 2e-5, b
            assert (out[2][b, :, :L] - a1[0]).abs().max().item() < 2e-6, b
        # explicit seeds, in another order: item b still follows its own seed
        seeds = [dec.call_seed(c0 + 1 + b) for b in range(len(lens))]
        perm = list(reversed(range(len(lens))))
        out2 = dec.inference_batch(mem[perm], [lens[p] for p in perm], seeds=[seeds[p] for p in perm], persistent=persistent)
        for i, p in enumerate(perm):
            assert (out2[0][i] - out[0][p]).abs().max().item() < 2e-5
        # a different seed gives different masks
        out3 = dec.inference_batch(mem[:1], lens[:1], seeds=[seeds[0] + 1], persistent=persistent)
        assert (out3[0][0] - out[0][0]).abs().max().item() > 1e-3


def _synth(tmp_path, hp_string, gate_bias=None, vocoder=None, name='ck'):
    import hparams as HP
    import train as TR
    from synthesizer import Synthesizer
    hp = HP.create_hparams(hp_string)
    torch.manual_seed(hp.seed)
    model = TR.load_model(hp)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if gate_bias is not None:
        sd['decoder.gate_layer.linear_layer.bias'].fill_(gate_bias)
    ck = str(tmp_path / name)
    torch.save({'iteration': 1, 'state_dict': sd, 'optimizer': {}, 'learning_rate': 1e-3}, ck)
    fl = str(tmp_path / 'refs_test.txt')
    g = torch.Generator().manual_seed(5)
    zs = (torch.randn(8, hp.z_latent_dim, generator=g) * 0.3).numpy()
    np.savez(Synthesizer.centroid_cache_path(ck, fl), zs=zs, emotions=np.arange(8) % 4)
    return hp, ck, fl


OTHER_TEXTS = ("안녕하세요.", "오늘은 날씨가 참 좋네요. 산책하러 갈까요?", "네.")


@pytest.mark.parametrize("case", ['ratios', 'ref_audio'])
def test_synthesize_batch_item_matches_the_reference(tmp_path, golden_dir, no_dropout, case):
    import hparams as HP
    import train as TR
    from scipy.io.wavfile import write
    from synthesizer import Synthesizer
    g = np.load(os.path.join(golden_dir, 'synthesize.npz'))
    text = bytes(g['text_utf8']).decode('utf-8')
    hp = HP.create_hparams("max_decoder_steps=24")
    torch.manual_seed(hp.seed)
    model = TR.load_model(hp)
    ck = str(tmp_path / 'ckpt_5')
    torch.save({'iteration': 5, 'state_dict': {k: v.detach().clone() for k, v in model.state_dict().items()},
                'optimizer': {}, 'learning_rate': 1e-3}, ck)
    fl = str(tmp_path / 'refs_test.txt')
    np.savez(Synthesizer.centroid_cache_path(ck, fl), zs=g['zs'], emotions=g['emotions'])
    syn = Synthesizer(hp).load(ck, filelist_path=fl)
    with torch.no_grad():
        syn.model.decoder.gate_layer.bias.fill_(float(g[case + '_gate_bias'][0]))
    ref = str(tmp_path / 'ref.wav')
    write(ref, 16000, g['ref_wav'])
    texts = [OTHER_TEXTS[0], text, OTHER_TEXTS[1], OTHER_TEXTS[2]]
    outs = syn.synthesize_batch(texts, None, case == 'ref_audio', [ref] * 4 if case == 'ref_audio' else None,
                                tuple(float(r) for r in g['ratios']))
    assert len(outs) == 4
    post, align = outs[1]
    want_post, want_align = torch.from_numpy(g[case + '_post']), torch.from_numpy(g[case + '_align'])
    assert post.shape == want_post.shape and align.shape == want_align.shape, (post.shape, want_post.shape)
    assert (post.cpu() - want_post).abs().mean() < 1e-4 and (post.cpu() - want_post).abs().max() < 5e-4
    assert (align.cpu() - want_align).abs().max() < 2e-5


def test_synthesize_batch_equals_the_sequence_of_synthesize_calls(tmp_path):
    """Dropout on, two synthesizers loaded from one checkpoint: the batch equals the sequential calls item by item, and with
    the Griffin-Lim vocoder and the same np.random seed so do the waveforms."""
    import model as M
    from scipy.io.wavfile import read
    from synthesizer import Synthesizer
    assert M.drop_rate > 0
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=30", gate_bias=-1e3)
    texts = [OTHER_TEXTS[1], OTHER_TEXTS[2], "한국어 음성 합성", OTHER_TEXTS[0], "가나다라마바사"]
    ratios = [(1, 0, 0, 0), (0, 1, 0, 0), (0.5, 0, 0.5, 0), (0, 0, 0, 1), (0.25, 0.25, 0.25, 0.25)]
    seq, bat = Synthesizer(hp).load(ck, vocoder='griffin_lim', filelist_path=fl), \
        Synthesizer(hp).load(ck, vocoder='griffin_lim', filelist_path=fl)
    np.random.seed(7)
    a = [seq.synthesize(t, str(tmp_path / ('s%d.wav' % i)), False, None, r) for i, (t, r) in enumerate(zip(texts, ratios))]
    np.random.seed(7)
    b = bat.synthesize_batch(texts, [str(tmp_path / ('b%d.wav' % i)) for i in range(len(texts))], False, None, ratios)
    assert seq.model.decoder._calls == bat.model.decoder._calls == len(texts)
    for i, ((pa, aa), (pb, ab)) in enumerate(zip(a, b)):
        assert pa.shape == pb.shape and aa.shape == ab.shape, i
        assert (pa - pb).abs().max().item() < 1e-4, i
        assert (aa - ab).abs().max().item() < 2e-5, i
        _, wa = read(str(tmp_path / ('s%d.wav' % i)))
        _, wb = read(str(tmp_path / ('b%d.wav' % i)))
        assert wa.shape == wb.shape == ((pa.size(2) - 1) * 256,)
        assert np.abs(wa - wb).max() < 1e-3 * max(1.0, np.abs(wa).max()), i
    # a second batch continues the call sequence
    c = seq.synthesize(texts[2], None, False, None, ratios[2])
    d = bat.synthesize_batch(texts[2:3], None, False, None, [ratios[2]])
    assert (c[0] - d[0][0]).abs().max().item() < 1e-4


def test_synthesizer_cli_writes_one_wav_per_text(tmp_path):
    from scipy.io.wavfile import read
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=20", gate_bias=-1e3)
    out = tmp_path / 'samples'
    cmd = [sys.executable, os.path.join(PKG, 'synthesizer.py'), '--load_path', ck, '--sample_path', str(out),
           '--text', OTHER_TEXTS[0], '--text', OTHER_TEXTS[1], '--text', OTHER_TEXTS[2], '--vocoder', 'griffin_lim',
           '--batch_size', '2', '--ratios', '0.5,0,0.5,0', '--filelist_path', fl, '--hparams', 'max_decoder_steps=20']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    for i in range(3):
        sr, data = read(str(out / ('%d.wav' % i)))
        assert sr == 16000 and data.shape == (19 * 256,) and np.all(np.isfinite(data))
