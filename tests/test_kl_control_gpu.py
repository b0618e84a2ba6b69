"""KL control on the device (csrc/kl_control.hip behind loss_function.Tacotron2Loss_VAE): free bits, the capacity target and the
collapse monitor against the fp64 references of tests/klc_ref.py.

Bounds: those of tests/test_refenc_gpu.py::test_fused_loss_matches_oracle, the project's own for this kernel's arithmetic —
values within 1e-5 * |ref| + 1e-6, gradients within 1e-5 * max |ref grad| + 1e-9.  tests/test_klc_ref.py asserts what lets them
hold case by case: no k[d] within 1 % of the floor, the fp32 and fp64 references floor the same dimensions, |K'/B - C| >= 10 % of C.
The monitor's mean and M2 are fp64 sums of fp32 inputs, so only the order differs from the reference: 1e-9 relative plus absolute.
Every case prints its figures before it asserts (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

import klc_ref as R

pytestmark = pytest.mark.gpu

STEP = 20000        # logistic KL weight ~ 1


def _criterion(free_bits=0.0, capacity=-1.0, monitor=None):
    import hparams as HP
    from loss_function import Tacotron2Loss_VAE
    spec = "anneal_function=logistic"
    if free_bits:
        spec += ",kl_free_bits=%r" % free_bits
    if capacity >= 0:
        spec += ",kl_capacity=%r" % capacity
    crit = Tacotron2Loss_VAE(HP.create_hparams(spec))
    crit.monitor = monitor
    return crit


def _run(crit, tensors):
    """(total, recon, kl, w) of the criterion on the device and the five leaves with their gradients"""
    dev = [t.clone().cuda().requires_grad_(True) for t in tensors[:5]]
    out = crit([dev[0], dev[1], dev[2], None, dev[3], dev[4]], (tensors[5].cuda(), tensors[6].cuda()), STEP)
    out[0].backward()
    torch.cuda.synchronize()
    return out, dev


@pytest.fixture()
def klc_calls(monkeypatch):
    """counts the calls of the new export"""
    import t2v_hip
    lib = t2v_hip.load_library()
    n = {'klc': 0, 'plain': 0}
    for key, name in (('klc', 't2v_loss_fwd_bwd_klc'), ('plain', 't2v_loss_fwd_bwd')):
        def counted(*a, _f=getattr(lib, name), _k=key):
            n[_k] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    return n


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("mode", R.MODES, ids=[m[0] for m in R.MODES])
@pytest.mark.parametrize("shape", R.SHAPES, ids=["B%d_T%d" % s for s in R.SHAPES])
def test_objective_matches_the_fp64_reference(shape, mode, klc_calls):
    _, free_bits, capacity = mode
    tensors = R.inputs(*shape)
    crit = _criterion(free_bits, capacity)
    out, dev = _run(crit, tensors)
    assert klc_calls == {'klc': 1, 'plain': 0}
    ref = R.objective(tensors, out[3], free_bits, capacity)
    got = {'total': out[0].detach(), 'recon': out[1], 'kl': out[2], 'kp': crit.kl_floored_sum, 'T': crit.kl_objective}
    failed = []
    for name, v in got.items():
        err, bound = abs(float(v) - float(ref[name])), 1e-5 * abs(float(ref[name])) + 1e-6
        print("%s %s %-5s got %.9g ref %.9g err %.3g bound %.3g" % (shape, mode[0], name, float(v), float(ref[name]), err, bound))
        if not err < bound:
            failed.append((name, err, bound))
    for name, d, g in zip(('dmel', 'dpost', 'dgate', 'dmu', 'dlogvar'), dev, ref['grads']):
        err, bound = float((d.grad.cpu().double() - g).abs().max()), 1e-5 * float(g.abs().max()) + 1e-9
        print("%s %s %-7s err %.3g bound %.3g" % (shape, mode[0], name, err, bound))
        if not err < bound:
            failed.append((name, err, bound))
    print("%s %s floored %d (ref %d) s %+.0f" % (shape, mode[0], int(crit.kl_floored_dims), ref['n_floored'], ref['s']))
    assert not failed, failed
    # exactness: the floored dimensions, their count, and zeros that are zeros
    fl = ref['floored']
    assert int(crit.kl_floored_dims) == ref['n_floored'] and (ref['n_floored'] > 0) == (free_bits > 0)
    for d in dev[3:]:
        assert (d.grad.cpu()[:, fl] == 0.0).all()
        assert (d.grad.cpu()[:, ~fl] != 0.0).any()
    assert out[3] == crit.kl_weight(STEP)


def test_validation_loss_stays_the_reference(klc_calls):
    """under no_grad the criterion launches the plain kernel: the loss of a free-bits + capacity run is the loss of a plain run"""
    tensors = R.inputs(6)
    crit, plain = _criterion(R.LAMBDA, R.CAPACITIES[0]), _criterion()
    dev = [t.cuda() for t in tensors]
    with torch.no_grad():
        a = crit([dev[0], dev[1], dev[2], None, dev[3], dev[4]], (dev[5], dev[6]), STEP)
        b = plain([dev[0], dev[1], dev[2], None, dev[3], dev[4]], (dev[5], dev[6]), STEP)
    assert klc_calls == {'klc': 0, 'plain': 2}
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------ off path
@pytest.mark.parametrize("shape", [(6, 400), (3, 5)], ids=["B6_T400", "B3_T5"])
def test_off_path_is_the_plain_launch_with_the_same_bits(shape, klc_calls):
    import t2v_hip
    tensors = R.inputs(*shape)
    out, dev = _run(_criterion(), tensors)
    assert klc_calls == {'klc': 0, 'plain': 1}
    leaves = [t.clone().cuda().requires_grad_(True) for t in tensors[:5]]
    total, out4 = t2v_hip.VAELoss.apply(*leaves, tensors[5].cuda(), tensors[6].cuda(), out[3])
    total.backward()
    torch.cuda.synchronize()
    assert klc_calls == {'klc': 0, 'plain': 2}
    assert torch.equal(out[0], total) and torch.equal(out[1], out4[1]) and torch.equal(out[2], out4[2])
    for a, b in zip(dev, leaves):
        assert torch.equal(a.grad, b.grad)


def test_monitor_alone_keeps_the_plain_objective():
    """with both switches off and a monitor installed the launch is the new one and the objective is the plain one: K' = T = KL,
    gradients the bits of the plain kernel's (the same products)"""
    import t2v_hip
    tensors = R.inputs(6, 400)
    crit = _criterion(monitor=t2v_hip.KLMonitor(R.D))
    out, dev = _run(crit, tensors)
    plain, pdev = _run(_criterion(), tensors)
    assert float(crit.kl_floored_sum) == float(crit.kl_objective) == float(out[2]) and int(crit.kl_floored_dims) == 0
    assert torch.equal(out[1], plain[1])                                    # recon: the same partials in the same order
    assert abs(float(out[2]) - float(plain[2])) < 1e-5 * float(plain[2])    # raw KL: fp64 column sums here, fp32 partials there
    for a, b in zip(dev, pdev):
        assert torch.equal(a.grad, b.grad)
    assert crit.monitor.read()['n'] == 6


# ------------------------------------------------------------------------------------------------ determinism, odd shapes
@pytest.mark.parametrize("B,dims", [(1, 1), (5, 1), (3, 7), (7, 33), (2, 256), (64, 32), (300, 32)])
def test_same_bits_twice_and_odd_latent_shapes(B, dims):
    """D = 1, B * D no multiple of 64, D = 256 (one row in flight), more rows than threads per column: against the fp64 reference,
    and two calls on the same inputs give the same bits"""
    import t2v_hip
    tensors = R.inputs(B, 3, dims)
    # a floor between the columns' batch means: the median of k, nudged off any k[d]; D = 1: under the only k (B = 1), above it (B = 5)
    k = R.objective(tensors, 1.0)['k']
    free_bits = float(k.median()) * 1.05 if dims > 1 else float(k[0]) * (0.5 if B == 1 else 2.0)
    assert R.floor_margin(k, free_bits) >= 0.01
    capacity = 0.5 * float(R.objective(tensors, 1.0, free_bits)['kp']) / B
    runs = []
    for _ in range(2):
        mon = t2v_hip.KLMonitor(dims)
        crit = _criterion(free_bits, capacity, monitor=mon)
        out, dev = _run(crit, tensors)
        runs.append([out[0], out[1], out[2], crit.kl_floored_sum, crit.kl_objective, crit.kl_floored_dims, mon.buf.clone()]
                    + [d.grad for d in dev])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ref = R.objective(tensors, out[3], free_bits, capacity)
    for name, v in (('total', out[0].detach()), ('kl', out[2]), ('kp', crit.kl_floored_sum), ('T', crit.kl_objective)):
        err, bound = abs(float(v) - float(ref[name])), 1e-5 * abs(float(ref[name])) + 1e-6
        print("B %d D %d %-5s got %.9g ref %.9g err %.3g bound %.3g" % (B, dims, name, float(v), float(ref[name]), err, bound))
        assert err < bound, name
    assert int(crit.kl_floored_dims) == ref['n_floored']
    for d, g in zip(dev[3:], ref['grads'][3:]):
        assert float((d.grad.cpu().double() - g).abs().max()) < 1e-5 * float(g.abs().max()) + 1e-9
        assert (d.grad.cpu()[:, ref['floored']] == 0.0).all()


# ------------------------------------------------------------------------------------------------ monitor
def test_monitor_follows_five_batches_of_different_sizes():
    import latent_scores
    import t2v_hip
    dims = 12
    rng = np.random.RandomState(11)
    # standard deviations of mu well on either side of sqrt(ACTIVE_THRESHOLD) = 0.1, and a mean that dwarfs the small ones
    std = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.3, 0.5, 0.8, 1.0, 1.5, 2.0, 3.0])
    batches = []
    for b in (3, 1, 16, 7, 64):
        mu = (rng.randn(b, dims) * std + 0.7).astype(np.float32)
        batches.append((mu, (0.3 * rng.randn(b, dims)).astype(np.float32)))
    mon = t2v_hip.KLMonitor(dims)
    crit = _criterion(monitor=mon)
    for mu, lv in batches:
        b = len(mu)
        t = R.inputs(b, 2, dims)
        _run(crit, (t[0], t[1], t[2], torch.from_numpy(mu), torch.from_numpy(lv), t[5], t[6]))
    ref = R.monitor_reference(batches)
    got = mon.read()
    buf = mon.buf.cpu().numpy()
    assert got['n'] == ref['n'] == 91 and got['launches'] == ref['launches'] == 5
    assert buf[0] == 91.0 and buf[1] == 5.0
    for name, g, r in (('mean', got['mean'], ref['mean']), ('m2', got['m2'], ref['m2'])):
        err = np.abs(g - r)
        print("monitor %-4s max err %.3g (rel %.3g)" % (name, err.max(), (err / np.abs(r)).max()))
        assert (err <= 1e-9 * np.abs(r) + 1e-9).all(), name
    skl = buf[2 + 2 * dims:]
    err = np.abs(skl - ref['sum_kl'])
    print("monitor sum kl max rel err %.3g" % (err / ref['sum_kl']).max())
    assert (err < 1e-5 * np.abs(ref['sum_kl']) + 1e-6).all()
    assert np.array_equal(got['kl_per_dim'], skl / 91)
    rows = np.concatenate([m for m, _ in batches])
    var = rows.astype(np.float64).var(axis=0)
    assert (np.abs(var - latent_scores.ACTIVE_THRESHOLD) > 0.5 * latent_scores.ACTIVE_THRESHOLD).all()   # no dimension near the rule
    assert got['active_units'] == latent_scores.active_units(rows) == 7
    mon.reset()
    torch.cuda.synchronize()
    assert not mon.buf.any() and mon.read()['n'] == 0 and mon.read()['active_units'] == 0
    _run(crit, (t[0], t[1], t[2], torch.from_numpy(batches[-1][0]), torch.from_numpy(batches[-1][1]), t[5], t[6]))
    again = mon.read()
    assert again['n'] == 64 and again['launches'] == 1
    one = R.monitor_reference(batches[-1:])
    assert (np.abs(again['m2'] - one['m2']) <= 1e-9 * one['m2'] + 1e-9).all()


# ------------------------------------------------------------------------------------------------ the training loop
def test_train_loop_prints_and_logs_the_monitor(tmp_path, capsys):
    """train() on four synthetic wavs with the switches on: the step lines carry the KL objective, the validation at iteration 0
    reads the monitor (2 utterances seen), and the event file holds the three new tags beside the old ones"""
    from scipy.io.wavfile import write
    import hparams as HP
    import logger as L
    import train as TR
    wavs = [str(tmp_path / ('%d.wav' % i)) for i in range(4)]
    for i, (p, n) in enumerate(zip(wavs, (24000, 16000, 20000, 18000))):
        write(p, 16000, (np.clip(0.1 * np.random.RandomState(i).randn(n), -1, 1) * 32767).astype(np.int16))
    texts = ["감정있는 한국어 목소리 생성", "안녕하세요 반갑습니다", "오늘 날씨가 좋네요", "테스트 문장입니다"]
    fl = tmp_path / 'list.txt'
    fl.write_text("\n".join("%s|%s|0|%d" % (w, t, i % 4) for i, (w, t) in enumerate(zip(wavs, texts))) + "\n", encoding='utf-8')
    out = str(tmp_path / 'out')
    hp = HP.create_hparams("batch_size=2,anneal_function=cyclical,anneal_cycle=4,kl_free_bits=0.05,kl_capacity=20,epochs=1,"
                           "iters_per_checkpoint=2,training_files=%s,validation_files=%s" % (fl, fl))
    TR.train(out, 'logs', None, False, 1, 0, 'group_name', hp)
    printed = capsys.readouterr().out
    assert "Train loss 0 " in printed and "Train loss 1 " in printed and "Validation loss 0:" in printed
    assert "KL monitor 0: active units " in printed and " of 32 over 2 utterances" in printed
    assert printed.count(" KL objective ") == 2 and " floored dims " in printed
    logdir = os.path.join(out, 'logs')
    ev = L.read_events(os.path.join(logdir, os.listdir(logdir)[0]))
    scalars = [(s, t, v) for s, t, k, v in ev if k == 'scalar']
    tags = {t for _, t, _ in scalars}
    assert {'training.kl_active_units', 'training.kl_floored_dims', 'training.kl_objective', 'kl_div', 'validation.loss'} <= tags
    assert [s for s, t, _ in scalars if t == 'training.kl_objective'] == [0, 1]
    assert [s for s, t, _ in scalars if t == 'training.kl_active_units'] == [0]
    T = [v for _, t, v in scalars if t == 'training.kl_objective']
    assert all(v > 0 for v in T)


# ------------------------------------------------------------------------------------------------ engine: graph equals eager
def test_graph_replay_follows_the_cycle_and_equals_eager_training():
    """test_graph_replay_equals_eager_training's configuration with kl_free_bits=0.05, kl_capacity=20 and the cyclical weight at
    anneal_cycle=4: steps 2..6 are replays of ONE graph, cross a cycle boundary (w = 0.2, 0.2, 0, 0.1, 0.2 through the device
    record, no re-capture) and are the eager steps bit for bit; the monitor saw steps x B rows"""
    import hparams as HP
    import train as TR
    import t2v_hip
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from bench import synthetic_batch
    batches = [synthetic_batch(3, 30, 48, 5, lens_in=[30, 22, 17], lens_out=[48, 40, 31]),
               synthetic_batch(3, 30, 48, 6, lens_in=[30, 25, 11], lens_out=[48, 37, 20])]
    runs = {}
    steps = 7
    for mode in ('eager', 'graph'):
        hp = HP.create_hparams("batch_size=3,graph_step=%s,kl_free_bits=0.05,kl_capacity=20,anneal_function=cyclical,anneal_cycle=4"
                               % (mode == 'graph'))
        torch.manual_seed(hp.seed)
        torch.cuda.manual_seed(hp.seed)
        eng = TR.TrainEngine(hp)
        assert eng.kl_monitor is not None and eng.criterion.monitor is eng.kl_monitor
        eng.model.overlap_branches = False
        eng.model.vae_gst.eps_override = torch.full((3, 32), 0.25, device='cuda')
        vals = []
        for it in range(steps):
            loss, recon, kl, w, gn = eng.step(batches[it % 2], it)
            c = eng.criterion
            vals.append((float(loss), float(recon), float(kl), float(w), float(gn), float(c.kl_floored_sum), float(c.kl_objective),
                         float(c.kl_floored_dims)))
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
        assert (mode == 'graph') == (len(eng._graphs) == 1)
        seen = eng.kl_monitor.read()
        assert seen['n'] == steps * 3 and seen['launches'] == steps
        runs[mode] = (vals, eng.optimizer.params.clone(), eng.optimizer.step_count, eng.kl_monitor.buf.clone())
    assert runs['eager'][2] == runs['graph'][2] == steps
    assert runs['eager'][0] == runs['graph'][0], (runs['eager'][0], runs['graph'][0])
    assert torch.equal(runs['eager'][1], runs['graph'][1]) and torch.equal(runs['eager'][3], runs['graph'][3])
    vals = runs['graph'][0]
    assert [v[3] for v in vals] == [0.0, 0.1, 0.2, 0.2, 0.0, 0.1, 0.2]
    for loss, recon, kl, w, gn, kp, T, nfl in vals:
        assert abs(loss - (recon + w * T)) <= 1e-6 * abs(loss)             # the replayed total carries that step's weight
        assert abs(T - abs(kp - 3 * 20.0)) <= 1e-6 * max(T, kp) + 1e-6 and kp >= kl and 0 <= nfl <= 32     # (fp32 copies of fp64 K', T)
    assert vals[4][0] == vals[4][1]                                         # w = 0 at the cycle's first step: total = recon
    assert len(set(v[0] for v in vals)) == steps
