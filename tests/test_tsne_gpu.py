"""t2v_hip.tsne / tsne_affinities / tsne_gradient (csrc/tsne.hip) against tests/tsne_ref.py in fp64, with the same formulas
run in fp32 numpy as the yardstick of what single precision costs; the scikit-learn numbers of tests/golden/tsne.npz for the
quality of a full run; determinism, sizes, refusals, and the commands that draw the map.

Error rule of the value tests: kernel error <= 4 x max(error of the fp32 restatement, one fp32 rounding of the reference).
The factor covers summation order and the device's exp / log / reciprocal; the floor is there because the kernel's result
is stored in fp32, so half an ulp is what a perfect kernel shows when the restatement happens to land closer than that."""
import os

import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
ULP = 2.0 ** -24


@pytest.fixture(scope='module')
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, 'tsne.npz')) as f:
        return {k: f[k] for k in f.files}


def _with_duplicates():
    """601 points in 32 dimensions, rows 100..119 exact copies of row 3"""
    rs = np.random.RandomState(77)
    X = (rs.standard_normal((4, 32))[np.arange(601) % 4] + rs.standard_normal((601, 32))).astype(np.float32)
    X[100:120] = X[3]
    return X


def _rel(a, ref, mask):
    return float((np.abs(a.astype(np.float64) - ref)[mask] / ref[mask]).max())


@pytest.mark.parametrize("name", ['fixture', 'duplicates'])
def test_affinities_against_fp64(gold, name):
    import t2v_hip
    X = gold['X'] if name == 'fixture' else _with_duplicates()
    n = len(X)
    ref = R.affinities(X, 30.0)
    yard = R.affinities(X, 30.0, np.float32)
    Pd = t2v_hip.tsne_affinities(torch.from_numpy(X).cuda(), 30.0)
    assert Pd.shape == (n, n) and Pd.dtype == torch.float32
    assert torch.equal(Pd, Pd.t()) and bool((Pd.diagonal() == 0).all())           # symmetric to the bit
    P = Pd.cpu().numpy()
    assert np.isfinite(P).all() and (P >= 0).all()
    big = ref > 1e-12
    e_k, e_y = _rel(P, ref, big), _rel(yard, ref, big)
    rows = ref.sum(axis=1)
    r_k = float(np.abs(P.astype(np.float64).sum(axis=1) - rows).max() / rows.max())
    r_y = float(np.abs(yard.astype(np.float64).sum(axis=1) - rows).max() / rows.max())
    print("affinities %s: max relative error kernel %.3g, fp32 numpy %.3g, ratio %.3g; row sums kernel %.3g, fp32 numpy %.3g; "
          "sum P %.9g" % (name, e_k, e_y, e_k / e_y, r_k, r_y, P.astype(np.float64).sum()))
    assert e_k <= MARGIN * max(e_y, ULP)
    assert r_k <= MARGIN * max(r_y, ULP)
    if name == 'duplicates':
        rest = np.setdiff1d(np.arange(n), np.r_[3, 100:120])
        assert (P[100:120, 3] > 0).all() and np.array_equal(P[100, rest], P[3, rest])     # a copy has the row of its original


@pytest.mark.parametrize("where", ['init', 'spread'])
@pytest.mark.parametrize("ex", [1.0, 12.0])
def test_gradient_against_fp64(gold, where, ex):
    import t2v_hip
    Pd = t2v_hip.tsne_affinities(torch.from_numpy(gold['X']).cuda(), 30.0)
    P = Pd.cpu().numpy()                                # the kernel's own fp32 P is the input of all three
    y = gold[where]
    kl_ref, g_ref = R.kl_and_grad(P, y, ex)
    kl_y, g_y = R.kl_and_grad(P, y, ex, np.float32)
    g, kl = t2v_hip.tsne_gradient(Pd, torch.from_numpy(y).cuda(), ex)
    assert g.shape == (len(y), 2) and kl.shape == ()
    g, kl = g.cpu().numpy().astype(np.float64), float(kl)
    scale = np.abs(g_ref).max()
    e_k, e_y = np.abs(g - g_ref).max() / scale, np.abs(g_y.astype(np.float64) - g_ref).max() / scale
    k_k, k_y = abs(kl - kl_ref) / abs(kl_ref), abs(float(kl_y) - kl_ref) / abs(kl_ref)
    print("gradient at %s, exaggeration %g: max |err| / max |grad| kernel %.3g, fp32 numpy %.3g, ratio %.3g; kl %.9g (fp64 %.9g) "
          "relative error kernel %.3g, fp32 numpy %.3g" % (where, ex, e_k, e_y, e_k / e_y, kl, kl_ref, k_k, k_y))
    assert e_k <= MARGIN * max(e_y, ULP)
    assert k_k <= MARGIN * max(k_y, ULP)


def test_twenty_iterations_against_fp64(gold):
    """The map is chaotic later; the first 20 iterations are compared, end to end (affinities and descent), with the fp32
    restatement's own drift from fp64 over the same 20 steps as the yardstick."""
    import t2v_hip
    X, y0 = gold['X'], gold['init']
    y_ref, t_ref = R.descend(R.affinities(X, 30.0), y0, 20)
    y_yard, t_yard = R.descend(R.affinities(X, 30.0, np.float32), y0, 20, dtype=np.float32)
    y, trace = t2v_hip.tsne(torch.from_numpy(X).cuda(), 30.0, n_iter=20, init=torch.from_numpy(y0), return_trace=True)
    y, trace = y.cpu().numpy().astype(np.float64), trace.cpu().numpy()
    scale = np.abs(y_ref).max()
    e_k, e_y = np.abs(y - y_ref).max() / scale, np.abs(y_yard.astype(np.float64) - y_ref).max() / scale
    print("20 iterations: max |dy| / max |y| kernel %.3g, fp32 numpy %.3g, ratio %.3g; kl %.7g (fp64 %.7g)"
          % (e_k, e_y, e_k / e_y, trace[-1], t_ref[-1]))
    assert trace.shape == (1,) and e_k <= MARGIN * max(e_y, ULP)
    k_k, k_y = abs(trace[0] - t_ref[0]) / t_ref[0], abs(t_yard[0] - t_ref[0]) / t_ref[0]
    print("   kl relative error kernel %.3g, fp32 numpy %.3g" % (k_k, k_y))
    assert k_k <= MARGIN * max(k_y, ULP)                # the one trace slot holds the objective after the 20th update


@pytest.fixture(scope='module')
def full_run(gold):
    import t2v_hip
    y, trace = t2v_hip.tsne(torch.from_numpy(gold['X']).cuda(), 30.0, n_iter=1000, seed=0, return_trace=True)
    return y.cpu(), trace.cpu()


def test_full_run_quality(gold, full_run):
    y, trace = (t.numpy() for t in full_run)
    bound = float(gold['final_kl'].max()) * 1.02
    in_x, in_map = R.knn_label_agreement(gold['X'], gold['labels']), R.knn_label_agreement(y, gold['labels'])
    print("1000 iterations: KL %.5f (scikit-learn exact, 5 seeds: %.5f..%.5f; bound %.5f); 5-NN label agreement %.4f in X, "
          "%.4f in the map; trace %s" % (trace[-1], gold['final_kl'].min(), gold['final_kl'].max(), bound, in_x, in_map,
                                         np.array2string(trace, precision=4)))
    assert trace.shape == (20,) and np.isfinite(trace).all() and np.isfinite(y).all()
    assert trace[-1] <= bound
    assert (np.diff(trace[5:]) <= 0).all()              # slots 5.. are iterations 300, 350, ..., 1000
    assert in_map >= in_x


def test_runs_repeat_to_the_bit(gold, full_run):
    import t2v_hip
    X = torch.from_numpy(gold['X']).cuda()
    y, trace = t2v_hip.tsne(X, 30.0, n_iter=1000, seed=0, return_trace=True)
    assert torch.equal(y.cpu(), full_run[0]) and torch.equal(trace.cpu(), full_run[1])
    # the same rows at the head of a larger buffer whose tail is NaN: nothing past N is read
    big = torch.full((len(X) + 37, X.size(1)), float('nan'), device='cuda')
    big[:len(X)] = X
    y2 = t2v_hip.tsne(big[:len(X)], 30.0, n_iter=1000, seed=0)
    assert torch.equal(y2.cpu(), full_run[0])
    assert torch.equal(t2v_hip.tsne_affinities(big[:len(X)], 30.0), t2v_hip.tsne_affinities(X, 30.0))
    assert not torch.equal(t2v_hip.tsne(X, 30.0, n_iter=1000, seed=1).cpu(), full_run[0])


@pytest.mark.parametrize("n", [97, 1232, 6496])
def test_sizes_finish_finite(n):
    import t2v_hip
    x = torch.from_numpy(np.random.RandomState(n).standard_normal((n, 32)).astype(np.float32)).cuda()
    y, trace = t2v_hip.tsne(x, 30.0, n_iter=1000, return_trace=True)
    assert y.shape == (n, 2) and y.dtype == torch.float32 and y.is_cuda
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(trace).all()) and float(y.abs().max()) > 1.0
    print("N = %d: KL %.4f" % (n, float(trace[-1])))


def test_wide_inputs_and_other_perplexities():
    import t2v_hip
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((300, 64)).astype(np.float32))
    for d, perplexity in ((2, 5.0), (33, 50.0), (64, 99.0)):
        ref = R.affinities(x[:, :d].numpy(), perplexity)
        P = t2v_hip.tsne_affinities(x[:, :d].contiguous().cuda(), perplexity).cpu().numpy()
        yard = R.affinities(x[:, :d].numpy(), perplexity, np.float32)
        big = ref > 1e-12
        assert _rel(P, ref, big) <= MARGIN * max(_rel(yard, ref, big), ULP), (d, perplexity)


def test_refusals_name_the_numbers():
    import t2v_hip
    with pytest.raises(ValueError, match="16385"):
        t2v_hip.tsne(torch.empty(16385, 32, device='cuda'))
    with pytest.raises(ValueError, match="65"):
        t2v_hip.tsne(torch.zeros(600, 65, device='cuda'))
    with pytest.raises(ValueError, match="perplexity 40 with 100 points"):
        t2v_hip.tsne(torch.zeros(100, 32, device='cuda'), perplexity=40)
    with pytest.raises(ValueError, match="perplexity"):
        t2v_hip.tsne_affinities(torch.zeros(100, 32, device='cuda'), 40.0)
    with pytest.raises(ValueError):
        t2v_hip.tsne(torch.zeros(600, 32, device='cuda'), n_iter=0)
    with pytest.raises(ValueError):
        t2v_hip.tsne(torch.zeros(600, 32, device='cuda'), init=torch.zeros(599, 2))
    with pytest.raises(ValueError):
        t2v_hip.tsne(torch.zeros(600, 32, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError):
        t2v_hip.tsne_gradient(torch.zeros(600, 600, device='cuda'), torch.zeros(600, 3, device='cuda'))
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()


# ---------------------------------------------------------------------------------------------- from wavs to the figure
def _perturb_bns(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                k = m.num_features
                m.running_mean.copy_(torch.randn(k, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(k, generator=g) + 0.5)
                m.weight.copy_(1 + 0.3 * torch.randn(k, generator=g))
                m.bias.copy_(0.2 * torch.randn(k, generator=g))


def _write_wavs(dirpath, n, seed, sr=16000, lo=3000, hi=16000):
    from scipy.io.wavfile import write
    rng = np.random.RandomState(seed)
    paths = []
    for i in range(n):
        N = int(rng.randint(lo, hi))
        t = np.arange(N) / sr
        x = 4000 * np.sin(2 * np.pi * rng.uniform(80, 400) * t) + 1500 * rng.randn(N)
        p = os.path.join(str(dirpath), 'w%03d_%d.wav' % (i, seed))
        write(p, sr, np.clip(x, -32768, 32767).astype(np.int16))
        paths.append(p)
    return paths


@pytest.fixture(scope='module')
def wavset(tmp_path_factory):
    import hparams as HP
    import train as TR
    d = tmp_path_factory.mktemp('latent_map')
    hp = HP.create_hparams("")
    torch.manual_seed(hp.seed)
    model = TR.load_model(hp)
    _perturb_bns(model.vae_gst, 21)
    ck = os.path.join(str(d), 'ckpt')
    torch.save({'iteration': 1, 'state_dict': {k: v.detach().clone() for k, v in model.state_dict().items()}, 'optimizer': {},
                'learning_rate': 1e-3}, ck)
    wavs = _write_wavs(d, 100, 1)
    emotions = [int(e) for e in np.random.RandomState(2).randint(0, 4, size=len(wavs))]
    fl = os.path.join(str(d), 'list_test.txt')
    with open(fl, 'w', encoding='utf-8') as f:
        for p, e in zip(wavs, emotions):
            f.write('%s|텍스트|0|%d\n' % (p, e))
    return dict(dir=str(d), hp=hp, ck=ck, wavs=wavs, emotions=emotions, filelist=fl)


def test_synthesizer_latent_map(wavset):
    import t2v_hip
    from synthesizer import Synthesizer
    syn = Synthesizer(wavset['hp']).load_checkpoint(wavset['ck'])
    y = syn.latent_map(wavset['wavs'], perplexity=20.0, n_iter=300)
    assert y.shape == (100, 2) and y.is_cuda and bool(torch.isfinite(y).all())
    mu = syn.latents(wavset['wavs'])[1]
    assert torch.equal(y, t2v_hip.tsne(mu, perplexity=20.0, n_iter=300))
    y2, trace = syn.latent_map(wavset['wavs'][:60], key='zs', batch_size=7, perplexity=10.0, n_iter=100, seed=3, return_trace=True)
    assert y2.shape == (60, 2) and trace.shape == (2,)
    with pytest.raises(ValueError, match="key"):
        syn.latent_map(wavset['wavs'], key='mu')
    with pytest.raises(ValueError, match="512"):
        syn.latent_map(wavset['wavs'], key='prosody')          # E = 512 is wider than the kernel's 64 dimensions


def test_commands_write_the_map(wavset):
    import extract_latents
    import latent_map
    plain = os.path.join(wavset['dir'], 'latents.npz')
    extract_latents.main(['--load_path', wavset['ck'], '--filelist_path', wavset['filelist'], '--out', plain])
    with np.load(plain) as f:
        assert sorted(f.files) == ['emotions', 'logvars', 'mus', 'paths', 'prosody', 'zs']       # what it wrote before --tsne
        mus = f['mus']
    out, png = os.path.join(wavset['dir'], 'map.npz'), os.path.join(wavset['dir'], 'map.png')
    latent_map.main(['--latents', plain, '--out', out, '--png', png, '--n_iter', '300'])
    with np.load(out) as f:
        assert sorted(f.files) == ['emotions', 'kl', 'kl_trace', 'map', 'paths']
        assert f['map'].shape == (100, 2) and f['map'].dtype == np.float32 and np.isfinite(f['map']).all()
        assert f['kl_trace'].shape == (6,) and float(f['kl']) == float(f['kl_trace'][-1]) and np.isfinite(f['kl'])
        assert f['emotions'].tolist() == wavset['emotions'] and f['paths'].tolist() == wavset['wavs']
        want, _ = latent_map.compute_map(mus, n_iter=300)
        assert np.array_equal(f['map'], want)
    try:
        import matplotlib  # noqa: F401
        has_plots = True
    except ImportError:
        has_plots = False
    assert os.path.isfile(png) == has_plots
    if has_plots:
        with open(png, 'rb') as f:
            assert f.read(8) == b'\x89PNG\r\n\x1a\n'
    both = os.path.join(wavset['dir'], 'latents_tsne.npz')
    extract_latents.main(['--load_path', wavset['ck'], '--filelist_path', wavset['filelist'], '--out', both, '--tsne'])
    with np.load(both) as f:
        assert sorted(f.files) == ['emotions', 'logvars', 'mus', 'paths', 'prosody', 'tsne', 'tsne_kl', 'zs']
        assert np.array_equal(f['mus'], mus)
        want, trace = latent_map.compute_map(mus)
        assert np.array_equal(f['tsne'], want) and float(f['tsne_kl']) == float(trace[-1])
