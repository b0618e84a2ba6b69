"""The weight average through the training engine and its consumers: TrainEngine with hparams.ema_decay (eager and captured
steps), the checkpoint keys and a resume, Synthesizer.load_checkpoint(weights='ema').  One module-wide set of runs at B = 2,
the smallest batch of tests/test_train_plumbing_gpu.py; every test reads what those runs left."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 6
HP = "batch_size=2,anneal_function=constant,graph_step=%s,ema_decay=%s"


def _engine(graph, decay):
    import hparams
    import train as TR
    hp = hparams.create_hparams(HP % (graph, decay))
    torch.manual_seed(hp.seed)
    torch.cuda.manual_seed(hp.seed)
    eng = TR.TrainEngine(hp)
    eng.graph_watchdog = False          # (its eager comparison step would take the place of the fourth replay)
    eng.model.vae_gst.eps_override = torch.full((2, 32), 0.125, device='cuda')
    return hp, eng


def _steps(eng, batch, first, last):
    with eng.stream_context():
        for it in range(first, last):
            eng.step(batch, it)
    torch.cuda.synchronize()
    import t2v_hip
    t2v_hip.check_async_errors()


def _state(eng):
    opt = eng.optimizer
    return dict(params=opt.params.clone(), ema=None if opt.ema is None else opt.ema.clone(), m=opt.exp_avg.clone(),
                step_count=opt.step_count)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    import t2v_hip
    import train as TR
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synthetic_batch
    batch = synthetic_batch(2, 17, 24, 3)
    tmp = tmp_path_factory.mktemp('ema')
    out = {}
    # 6 steps of one shape on the graph engine: two eager warm-ups, the capture, then replays
    _, eng = _engine(True, 0.999)
    _steps(eng, batch, 0, STEPS)
    out['graph'] = _state(eng)
    out['graph_replays'] = len(eng._graphs)
    eng.close()
    # the same on the eager engine; a checkpoint after 6 steps, then the seventh
    hp, eng = _engine(False, 0.999)
    _steps(eng, batch, 0, STEPS)
    out['eager'] = _state(eng)
    out['ckpt'] = str(tmp / 'checkpoint_ema')
    TR.save_checkpoint(eng.model, eng.optimizer, hp.learning_rate, STEPS - 1, out['ckpt'])
    out['ema_state_dict'] = eng.optimizer.ema_state_dict(eng.model)
    out['state_dict'] = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    _steps(eng, batch, STEPS, STEPS + 1)
    out['seven'] = _state(eng)
    eng.close()
    # a fresh engine resumes from the checkpoint and makes the seventh step
    hp, eng = _engine(False, 0.999)
    eng.optimizer.ema.fill_(3.0)
    _, _, _, iteration = TR.load_checkpoint(out['ckpt'], eng.model, eng.optimizer)
    out['resumed_at'] = (iteration, _state(eng))
    _steps(eng, batch, iteration + 1, iteration + 2)
    out['resumed'] = _state(eng)
    eng.close()
    # the feature off: one step, a checkpoint; resumed by a run that has it on
    hp, eng = _engine(False, 0.0)
    _steps(eng, batch, 0, 1)
    out['off_has_ema'] = eng.optimizer.ema is not None
    out['ckpt_off'] = str(tmp / 'checkpoint_plain')
    TR.save_checkpoint(eng.model, eng.optimizer, hp.learning_rate, 0, out['ckpt_off'])
    eng.close()
    t2v_hip.register_grad_slots({})
    return out


def test_graph_and_eager_engines_keep_the_same_shadow(runs):
    g, e = runs['graph'], runs['eager']
    assert runs['graph_replays'] == 1 and g['step_count'] == e['step_count'] == STEPS
    assert torch.equal(g['params'].view(torch.int32), e['params'].view(torch.int32))
    assert torch.equal(g['ema'].view(torch.int32), e['ema'].view(torch.int32))
    assert not torch.equal(e['ema'], e['params']) and bool(torch.isfinite(e['ema']).all())


def test_checkpoint_round_trip_continues_the_uninterrupted_run(runs):
    iteration, at = runs['resumed_at']
    assert iteration == STEPS - 1 and at['step_count'] == STEPS
    assert torch.equal(at['ema'].view(torch.int32), runs['eager']['ema'].view(torch.int32))
    assert torch.equal(at['params'].view(torch.int32), runs['eager']['params'].view(torch.int32))
    for k in ('params', 'ema', 'm'):
        assert torch.equal(runs['resumed'][k].view(torch.int32), runs['seven'][k].view(torch.int32)), k
    assert runs['resumed']['step_count'] == STEPS + 1
    assert not torch.equal(runs['seven']['ema'], runs['eager']['ema'])


def test_checkpoint_keys_with_and_without_the_average(runs, golden_dir, capsys):
    import train as TR
    with open(os.path.join(golden_dir, 'checkpoint_schema.json')) as f:
        top = json.load(f)['top_keys']
    off = torch.load(runs['ckpt_off'], map_location='cpu', weights_only=False)
    assert not runs['off_has_ema'] and list(off.keys()) == top and len(top) == 4          # the reference's four keys, nothing else
    on = torch.load(runs['ckpt'], map_location='cpu', weights_only=False)
    assert list(on.keys()) == top + ['ema_state_dict', 'ema'] and on['ema'] == {'decay': 0.999, 'warmup': True}
    assert list(on['ema_state_dict']) == list(on['state_dict']) and len(on['ema_state_dict']) == 142
    import optim
    differ = [k for k in on['state_dict'] if not torch.equal(on['state_dict'][k], on['ema_state_dict'][k])]
    # only live parameters are averaged: dead ones and the buffers (BatchNorm statistics) are the model's
    assert not [k for k in differ if optim.is_dead_param(k) or 'running_' in k or k.endswith('num_batches_tracked')]
    assert len(differ) > len(on['optimizer']['state']) // 2
    # a checkpoint without the average, resumed with the feature on: the shadow starts from the loaded weights, and says so
    _, eng = _engine(False, 0.999)
    try:
        eng.optimizer.ema.fill_(3.0)
        capsys.readouterr()
        TR.load_checkpoint(runs['ckpt_off'], eng.model, eng.optimizer)
        assert "holds no 'ema_state_dict'" in capsys.readouterr().out
        assert torch.equal(eng.optimizer.ema, eng.optimizer.params)
        eng.optimizer.ema.fill_(3.0)
        TR.warm_start_model(runs['ckpt'], eng.model, eng.optimizer)               # a warm start seeds it from the RAW weights
        assert torch.equal(eng.optimizer.ema, eng.optimizer.params)
        assert torch.equal(eng.optimizer.params.view(torch.int32), runs['eager']['params'].view(torch.int32))
    finally:
        eng.close()


def test_synthesizer_loads_the_averaged_weights(runs):
    import hparams
    from synthesizer import Synthesizer
    hp = hparams.create_hparams()
    syn = Synthesizer(hp).load_checkpoint(runs['ckpt'], weights='ema')
    got = syn.model.state_dict()
    assert syn.weights == 'ema' and not syn.model.training
    assert list(got) == list(runs['ema_state_dict']) and all(torch.equal(got[k].cpu(), runs['ema_state_dict'][k].cpu()) for k in got)
    for w in (None, 'raw'):
        raw = Synthesizer(hp).load_checkpoint(runs['ckpt'], weights=w)
        assert raw.weights == 'raw' and all(torch.equal(v.cpu(), runs['state_dict'][k].cpu()) for k, v in raw.model.state_dict().items())
    moved = [k for k in got if not torch.equal(got[k].cpu(), runs['state_dict'][k].cpu())]
    assert moved
    with pytest.raises(ValueError, match='ema_state_dict'):
        Synthesizer(hp).load_checkpoint(runs['ckpt_off'], weights='ema')
    with pytest.raises(ValueError, match='weights'):
        Synthesizer(hp).load_checkpoint(runs['ckpt'], weights='best')
    assert Synthesizer(hp).load_checkpoint(runs['ckpt_off']).weights == 'raw'
    a = Synthesizer.centroid_cache_path(runs['ckpt'], 'lists/koemo_spk_emo_all_test.txt')
    b = Synthesizer.centroid_cache_path(runs['ckpt'], 'lists/koemo_spk_emo_all_test.txt', 'ema')
    assert a == runs['ckpt'] + '_test.npz' and b == runs['ckpt'] + '_ema_test.npz'
    assert Synthesizer.centroid_cache_path(runs['ckpt'], 'lists/koemo_spk_emo_all_test.txt', 'raw') == a


def test_train_validates_and_saves_both_weight_sets(tmp_path, capsys):
    """train() with ema_decay on (graph engine, the default): every checkpoint iteration validates the raw and then the averaged
    weights, logs both losses, leaves the raw weights in the model, and the checkpoint it writes loads through --weights ema"""
    import numpy as np
    from scipy.io.wavfile import write
    import hparams
    import train as TR
    from logger import read_events
    from synthesizer import Synthesizer
    wavs = [str(tmp_path / 'a.wav'), str(tmp_path / 'b.wav')]
    for i, (p, n) in enumerate(zip(wavs, (16000, 12000))):
        write(p, 16000, (np.clip(0.1 * np.random.RandomState(i).randn(n), -1, 1) * 32767).astype(np.int16))
    fl = tmp_path / 'list.txt'
    fl.write_text("%s|안녕하세요 반갑습니다|0|0\n%s|오늘 날씨가 좋네요|0|1\n" % tuple(wavs), encoding='utf-8')
    out = str(tmp_path / 'out')
    hp = hparams.create_hparams("batch_size=2,anneal_function=constant,epochs=2,iters_per_checkpoint=1,ema_decay=0.999,"
                                "training_files=%s,validation_files=%s" % (fl, fl))
    TR.train(out, 'logs', None, False, 1, 0, 'group_name', hp)
    printed = capsys.readouterr().out
    for it in (0, 1):
        assert printed.index("Validation loss %d:" % it) < printed.index("Validation loss (ema) %d:" % it)
    ck = torch.load(os.path.join(out, 'checkpoint_1'), map_location='cpu', weights_only=False)
    assert ck['ema'] == {'decay': 0.999, 'warmup': True} and list(ck['ema_state_dict']) == list(ck['state_dict'])
    moved = [k for k in ck['state_dict'] if not torch.equal(ck['state_dict'][k], ck['ema_state_dict'][k])]
    assert moved and all(bool(torch.isfinite(v).all()) for v in ck['ema_state_dict'].values() if v.dtype.is_floating_point)
    logdir = os.path.join(out, 'logs')
    events = [e for f in os.listdir(logdir) for e in read_events(os.path.join(logdir, f))]
    raw = {s: v for s, tag, kind, v in events if tag == 'validation.loss'}
    ema = {s: v for s, tag, kind, v in events if tag == 'validation.loss.ema'}
    assert sorted(raw) == sorted(ema) == [0, 1] and all(np.isfinite(v) for v in ema.values()) and ema != raw
    syn = Synthesizer(hparams.create_hparams()).load_checkpoint(os.path.join(out, 'checkpoint_1'), weights='ema')
    assert all(torch.equal(v.cpu(), ck['ema_state_dict'][k]) for k, v in syn.model.state_dict().items())
