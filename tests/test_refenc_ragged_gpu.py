"""vae_gst over a ragged batch of reference mels: every row is what the utterance alone gives, in the model, the
centroid pass of Synthesizer.load, batched reference styles and the latent-export command."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tacotron2-vae_amd')
EDGE_LENS = [3, 64, 65, 127, 128, 129, 600, 1100]        # 1100 frames: 18 GRU steps


def _perturb_bns(module, seed):
    """BatchNorm running statistics and affine parameters away from the identity"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                m.weight.copy_(1 + 0.3 * torch.randn(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))


def _vae(seed=5):
    import hparams as HP
    import modules as MD
    torch.manual_seed(seed)
    vae = MD.VAE_GST(HP.create_hparams())
    _perturb_bns(vae, seed + 1)
    return vae.cuda().eval()


def _mels(lens, seed, T=None):
    g = torch.Generator().manual_seed(seed)
    T = T or max(lens)
    mel = torch.randn(len(lens), 80, T, generator=g) * 2 - 4
    for b, L in enumerate(lens):
        mel[b, :, L:] = float('nan')             # never read
    return mel.cuda()


def _check_rows(vae, mels, lens, oracle=True):
    import t2v_oracle as O
    sd = {'vae_gst.' + k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in vae.state_dict().items()}
    out = vae(mels, lens)
    assert all(not o.requires_grad for o in out)
    assert out[0].shape == (len(lens), 512) and all(o.shape == (len(lens), 32) for o in out[1:])
    with torch.no_grad():
        for b, L in enumerate(lens):
            alone = vae(mels[b:b + 1, :, :L])
            ref = O.vae_gst_forward(sd, mels[b:b + 1, :, :L].cpu().double(), False) if oracle else None
            for k, name in enumerate(('prosody', 'mu', 'logvar', 'z')):
                row, one = out[k][b].cpu(), alone[k][0].cpu()
                assert torch.isfinite(row).all(), (b, L, name)
                assert (row - one).abs().max().item() < 1e-4, (b, L, name)
                if oracle:
                    d_one = (one.double() - ref[k][0]).abs().max().item()
                    d_row = (row.double() - ref[k][0]).abs().max().item()
                    assert d_row <= 2 * d_one + 1e-7, (b, L, name, d_row, d_one)


@pytest.mark.parametrize("gemm_form", [True, False])
def test_ragged_rows_equal_each_utterance_alone(monkeypatch, gemm_form):
    import t2v_hip
    monkeypatch.setattr(t2v_hip, 'CONV2D_GEMM', gemm_form)
    vae = _vae()
    mels = _mels(EDGE_LENS, 11)
    _check_rows(vae, mels, EDGE_LENS)
    # lengths as a device int tensor and as a CPU tensor: the same answer
    a = vae(mels, torch.tensor(EDGE_LENS, dtype=torch.int32).cuda())
    b = vae(mels, torch.tensor(EDGE_LENS))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("gemm_form", [True, False])
def test_ragged_batch_above_16_items(monkeypatch, gemm_form):
    """B = 20 crosses the GRU's 16-sequence chunk of one cooperative launch"""
    import t2v_hip
    monkeypatch.setattr(t2v_hip, 'CONV2D_GEMM', gemm_form)
    vae = _vae(7)
    rng = np.random.RandomState(4)
    lens = [2, 700] + [int(x) for x in rng.randint(3, 700, size=18)]
    _check_rows(vae, _mels(lens, 12), lens)


def test_ragged_guards_and_full_lengths():
    vae = _vae()
    mels = _mels([50, 40], 13)
    with pytest.raises(ValueError):
        vae(mels, [1, 40])                       # CoordConv needs >= 2 rows
    with pytest.raises(ValueError):
        vae(mels, [51, 40])                      # past the padded length
    with pytest.raises(ValueError):
        vae(mels, [50])                          # one length per item
    vae.train()
    with pytest.raises(RuntimeError):
        vae(mels, [50, 40])
    vae.eval()
    full = _mels([90, 90, 90], 14)
    with torch.no_grad():
        want = vae(full)
    got = vae(full, [90, 90, 90])
    for x, y in zip(got, want):
        assert (x - y).abs().max().item() < 1e-5


def test_ragged_entry_points_reject_bad_arguments():
    import t2v_hip
    lib = t2v_hip.load_library()
    x = torch.zeros(2, 80, 40, device='cuda')
    w = torch.zeros(32, 4, 3, 3, device='cuda')
    y = torch.empty(2, 32, 20, 40, device='cuda')
    hlen = torch.tensor([40, 30], dtype=torch.int32, device='cuda')
    p = t2v_hip._p
    s = t2v_hip._stream()
    assert lib.t2v_conv2d_s2_fwd_ragged(p(x), p(w), None, p(y), None, 2, 1, 40, 80, 32, 1, 40, s) == -2        # no hlen
    assert lib.t2v_conv2d_s2_fwd_ragged(p(x), p(w), None, p(y), p(hlen), 2, 1, 40, 80, 32, 1, 39, s) == -2    # stride < H
    assert lib.t2v_conv2d_s2_fwd_ragged(p(x), p(w), None, p(y), p(hlen), 2, 2, 40, 80, 32, 1, 40, s) == -2    # gather needs Cx 1
    scr = torch.empty(lib.t2v_conv2d_s2_gemm_ragged_scratch_floats(2, 1, 40, 80, 32, 1), device='cuda')
    assert lib.t2v_conv2d_s2_fwd_gemm_ragged(p(x), p(w), None, p(y), p(scr), None, 2, 1, 40, 80, 32, 1, 40, s) == -2
    gi = torch.zeros(2, 3, 768, device='cuda')
    assert lib.t2v_gru_fwd_len(p(gi), p(w), p(w), p(y), None, p(y), p(hlen), None, p(y), 2, 3, s) == -2          # no steps
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- synthesizer
def _write_wavs(dirpath, n, seed, sr=16000, lo=3000, hi=40000):
    from scipy.io.wavfile import write
    rng = np.random.RandomState(seed)
    paths = []
    for i in range(n):
        N = int(rng.randint(lo, hi))
        t = np.arange(N) / sr
        x = 4000 * np.sin(2 * np.pi * rng.uniform(80, 400) * t) + 1500 * rng.randn(N)
        p = os.path.join(str(dirpath), 'w%02d_%d.wav' % (i, seed))
        write(p, sr, np.clip(x, -32768, 32767).astype(np.int16))
        paths.append(p)
    return paths


def _checkpoint(dirpath, hp_string="", gate_bias=None, name='ckpt'):
    import hparams as HP
    import train as TR
    hp = HP.create_hparams(hp_string)
    torch.manual_seed(hp.seed)
    model = TR.load_model(hp)
    _perturb_bns(model.vae_gst, 21)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if gate_bias is not None:
        sd['decoder.gate_layer.linear_layer.bias'].fill_(gate_bias)
    ck = os.path.join(str(dirpath), name)
    torch.save({'iteration': 1, 'state_dict': sd, 'optimizer': {}, 'learning_rate': 1e-3}, ck)
    return hp, ck


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp('refs')
    hp, ck = _checkpoint(d)
    wavs = _write_wavs(d, 40, 1)
    emotions = [int(e) for e in np.random.RandomState(2).randint(0, 4, size=len(wavs))]
    fl = os.path.join(str(d), 'koemo_spk_emo_all_test.txt')
    with open(fl, 'w', encoding='utf-8') as f:
        for p, e in zip(wavs, emotions):
            f.write('%s|텍스트|0|%d\n' % (p, e))
    from synthesizer import Synthesizer
    syn = Synthesizer(hp).load_checkpoint(ck)
    with torch.no_grad():
        seq = torch.cat([syn.model.vae_gst(syn.load_mel(p))[3] for p in wavs]).cpu().numpy()     # what load() did before
    return dict(dir=d, hp=hp, ck=ck, wavs=wavs, emotions=emotions, filelist=fl, z_seq=seq)


def test_load_mels_items_equal_load_mel(refs):
    from synthesizer import Synthesizer
    syn = Synthesizer(refs['hp'])
    paths = refs['wavs'][:6]
    mels, n = syn.load_mels(paths)
    assert mels.shape == (6, 80, max(n))
    for b, p in enumerate(paths):
        one = syn.load_mel(p)
        assert one.shape == (1, 80, n[b])
        assert (mels[b, :, :n[b]] - one[0]).abs().max().item() < 1e-5, b


def test_centroid_pass_runs_in_ragged_groups(refs, monkeypatch):
    import modules as MD
    from synthesizer import EMOTIONS, Synthesizer
    calls = []
    orig = MD.VAE_GST.forward

    def spy(self, inputs, lengths=None):
        calls.append((inputs.size(0), lengths is not None))
        return orig(self, inputs, lengths)
    monkeypatch.setattr(MD.VAE_GST, 'forward', spy)
    syn = Synthesizer(refs['hp']).load(refs['ck'], filelist_path=refs['filelist'], batch_size=16)
    assert calls == [(16, True), (16, True), (8, True)]
    cache = np.load(Synthesizer.centroid_cache_path(refs['ck'], refs['filelist']))
    assert cache['zs'].shape == refs['z_seq'].shape and cache['zs'].dtype == np.float32
    assert np.abs(cache['zs'] - refs['z_seq']).max() < 1e-4
    assert cache['emotions'].tolist() == refs['emotions']
    emo = np.array(refs['emotions'])
    for i, name in enumerate(EMOTIONS):
        want = refs['z_seq'][emo == i].mean(0)
        assert np.abs(getattr(syn, name) - want).max() < 1e-4, name
    # the cache is read back (no vae_gst call) on the next load
    del calls[:]
    Synthesizer(refs['hp']).load(refs['ck'], filelist_path=refs['filelist'])
    assert calls == []


def test_centroid_pass_rejects_a_wrong_sample_rate(refs, tmp_path):
    from synthesizer import Synthesizer
    bad = _write_wavs(tmp_path, 1, 9, sr=22050)[0]
    fl = str(tmp_path / 'list_bad.txt')
    with open(fl, 'w', encoding='utf-8') as f:
        f.write('%s|텍스트|0|1\n%s|텍스트|0|2\n' % (refs['wavs'][0], bad))
    with pytest.raises(ValueError, match="22050 SR doesn't match target 16000 SR"):
        Synthesizer(refs['hp']).load(refs['ck'], filelist_path=fl, batch_size=4)


def test_extract_latents_command(refs):
    out = os.path.join(str(refs['dir']), 'latents.npz')
    cmd = [sys.executable, os.path.join(PKG, 'extract_latents.py'), '--load_path', refs['ck'], '--filelist_path',
           refs['filelist'], '--out', out, '--batch_size', '12']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    N = len(refs['wavs'])
    assert sorted(d.files) == ['emotions', 'logvars', 'mus', 'paths', 'prosody', 'zs']
    assert d['prosody'].shape == (N, 512) and d['mus'].shape == d['logvars'].shape == d['zs'].shape == (N, 32)
    assert d['emotions'].shape == d['paths'].shape == (N,)
    assert d['emotions'].tolist() == refs['emotions'] and d['paths'].tolist() == refs['wavs']
    assert np.abs(d['zs'] - refs['z_seq']).max() < 1e-4
    assert np.array_equal(d['mus'], d['zs'])          # eval: z = mu


def test_latents_rows_in_input_order(refs):
    from synthesizer import Synthesizer
    syn = Synthesizer(refs['hp']).load_checkpoint(refs['ck'])
    paths = refs['wavs'][::-3]
    prosody, mu, logvar, z = syn.latents(paths, batch_size=5)
    idx = [refs['wavs'].index(p) for p in paths]
    assert np.abs(z.cpu().numpy() - refs['z_seq'][idx]).max() < 1e-4
    with torch.no_grad():
        for i in (0, len(paths) - 1):
            one = syn.model.vae_gst(syn.load_mel(paths[i]))
            for k in range(4):
                assert (one[k][0] - (prosody, mu, logvar, z)[k][i]).abs().max().item() < 1e-4


@pytest.fixture()
def no_dropout():
    import model as M
    old = M.drop_rate
    M.drop_rate = 0.0
    yield
    M.drop_rate = old


TEXTS = ("안녕하세요.", "오늘은 날씨가 참 좋네요. 산책하러 갈까요?", "네.", "한국어 음성 합성")


def test_synthesize_batch_reference_styles_in_one_vae_gst_call(tmp_path, monkeypatch):
    """dropout on, two synthesizers from one checkpoint: the batch with four reference wavs equals the sequential
    synthesize() calls, and vae_gst runs once for the whole batch (each distinct wav once)."""
    import model as M
    from synthesizer import Synthesizer
    monkeypatch.setattr(M, 'drop_rate', 0.5)       # the module default (another test may have left it at 0)
    hp, ck = _checkpoint(tmp_path, "max_decoder_steps=30", gate_bias=-1e3)
    fl = str(tmp_path / 'refs_test.txt')
    g = torch.Generator().manual_seed(5)
    np.savez(Synthesizer.centroid_cache_path(ck, fl), zs=(torch.randn(8, hp.z_latent_dim, generator=g) * 0.3).numpy(),
             emotions=np.arange(8) % 4)
    wavs = _write_wavs(tmp_path, 4, 3)
    seq, bat = Synthesizer(hp).load(ck, filelist_path=fl), Synthesizer(hp).load(ck, filelist_path=fl)
    a = [seq.synthesize(t, None, True, w) for t, w in zip(TEXTS, wavs)]
    calls = []
    orig = bat.model.vae_gst.forward

    def spy(inputs, lengths=None):
        calls.append((tuple(inputs.shape), None if lengths is None else list(lengths)))
        return orig(inputs, lengths)
    bat.model.vae_gst.forward = spy
    b = bat.synthesize_batch(list(TEXTS), None, True, wavs)
    assert len(calls) == 1 and calls[0][0][0] == 4 and calls[0][1] is not None
    for i, ((pa, aa), (pb, ab)) in enumerate(zip(a, b)):
        assert pa.shape == pb.shape and aa.shape == ab.shape, i
        assert (pa - pb).abs().max().item() < 1e-4, i
        assert (aa - ab).abs().max().item() < 2e-5, i
    # a repeated wav is encoded once; the items stay those of the sequential calls
    del calls[:]
    c = [seq.synthesize(t, None, True, w) for t, w in zip(TEXTS[:3], [wavs[2], wavs[0], wavs[2]])]
    d = bat.synthesize_batch(list(TEXTS[:3]), None, True, [wavs[2], wavs[0], wavs[2]])
    assert len(calls) == 1 and calls[0][0][0] == 2
    for (pa, _), (pb, _) in zip(c, d):
        assert pa.shape == pb.shape and (pa - pb).abs().max().item() < 1e-4


def test_synthesize_batch_golden_reference_wav_among_others(tmp_path, golden_dir, no_dropout):
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
        syn.model.decoder.gate_layer.bias.fill_(float(g['ref_audio_gate_bias'][0]))
    ref = str(tmp_path / 'ref.wav')
    write(ref, 16000, g['ref_wav'])
    others = _write_wavs(tmp_path, 3, 8, lo=5000, hi=60000)
    texts = [TEXTS[0], text, TEXTS[1], TEXTS[2]]
    outs = syn.synthesize_batch(texts, None, True, [others[0], ref, others[1], others[2]])
    post, align = outs[1]
    want_post, want_align = torch.from_numpy(g['ref_audio_post']), torch.from_numpy(g['ref_audio_align'])
    assert post.shape == want_post.shape and align.shape == want_align.shape, (post.shape, want_post.shape)
    assert (post.cpu() - want_post).abs().mean() < 1e-4 and (post.cpu() - want_post).abs().max() < 5e-4
    assert (align.cpu() - want_align).abs().max() < 2e-5
