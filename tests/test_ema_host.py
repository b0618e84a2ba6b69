"""Host side of the weight average (no GPU): the hparams group, --weights on the three command lines, the checkpoint dict with
and without an average (stub optimiser), the logger's tag and the derived binding of the new entry point."""
import ctypes as C

import pytest
import torch


def test_recipe_group_parses_and_stays_out_of_values_and_extensions():
    import hparams as HP
    hp = HP.create_hparams()
    assert hp.recipe() == {'ema_decay': 0.0, 'ema_warmup': True} and hp.ema_decay == 0.0 and hp.ema_warmup is True
    assert not set(hp.recipe()) & set(hp.values()) and not set(hp.recipe()) & set(hp.extensions())
    assert set(hp.values()) | set(hp.extensions()) | set(hp.recipe()) == set(hp._store)
    hp = HP.create_hparams("ema_decay=0.9999,ema_warmup=False,batch_size=4")
    assert hp.recipe() == {'ema_decay': 0.9999, 'ema_warmup': False} and hp.values()['batch_size'] == 4
    assert 'ema_decay' not in hp.values() and 'ema_decay' not in hp.extensions()
    assert HP.create_hparams().values() == HP.create_hparams("ema_decay=0.5").values()
    with pytest.raises(ValueError):
        HP.create_hparams("ema_decay=often")


def test_weights_flag_on_the_three_command_lines():
    import evaluate
    import extract_latents
    import synthesizer
    lines = ((synthesizer, ['--load_path', 'ck', '--text', 'x']),
             (evaluate, ['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.json']),
             (extract_latents, ['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz']))
    for mod, base in lines:
        assert mod.parse_args(base).weights is None
        assert synthesizer.weights_option(mod.parse_args(base)) == {}                # the call it always was
        for w in ('raw', 'ema'):
            args = mod.parse_args(base + ['--weights', w])
            assert args.weights == w and synthesizer.weights_option(args) == {'weights': w}
        with pytest.raises(SystemExit):
            mod.parse_args(base + ['--weights', 'best'])
    assert synthesizer.WEIGHTS == {'raw': 'state_dict', 'ema': 'ema_state_dict'}
    assert synthesizer.check_weights(None) == 'raw' and synthesizer.check_weights('ema') == 'ema'
    with pytest.raises(ValueError, match='weights'):
        synthesizer.check_weights('best')
    path = synthesizer.Synthesizer.centroid_cache_path
    assert path('out/checkpoint_500', 'lists/koemo_spk_emo_all_test.txt') == 'out/checkpoint_500_test.npz'
    assert path('out/checkpoint_500', 'lists/koemo_spk_emo_all_test.txt', 'ema') == 'out/checkpoint_500_ema_test.npz'
    assert path('out/checkpoint_500', 'refs.txt', 'ema') == 'out/checkpoint_500_ema_refs.npz'


class _StubAdam(object):
    """what save_checkpoint / load_checkpoint / warm_start_model ask of an optimiser"""

    def __init__(self, ema):
        self.ema = torch.zeros(3) if ema else None
        self.ema_decay, self.ema_warmup = (0.9999, True) if ema else (0.0, True)
        self.calls = []

    def state_dict(self):
        return {'state': {}, 'param_groups': [{'lr': 1e-3}]}

    def load_state_dict(self, sd):
        self.calls.append('load_state_dict')

    def ema_state_dict(self, model):
        return {k: v.detach().clone() + 1.0 for k, v in model.state_dict().items()}

    def load_ema_state_dict(self, sd):
        self.calls.append(('load_ema_state_dict', sorted(sd)))

    def reset_ema(self):
        self.calls.append('reset_ema')


def test_checkpoint_dict_with_and_without_an_average(tmp_path, capsys):
    import train as TR
    model = torch.nn.Linear(3, 2)
    plain, ema = str(tmp_path / 'plain'), str(tmp_path / 'ema')
    TR.save_checkpoint(model, _StubAdam(False), 1e-3, 7, plain)
    TR.save_checkpoint(model, _StubAdam(True), 1e-3, 7, ema)
    a = torch.load(plain, map_location='cpu', weights_only=False)
    b = torch.load(ema, map_location='cpu', weights_only=False)
    assert list(a) == ['iteration', 'state_dict', 'optimizer', 'learning_rate']          # the reference's dict, nothing else
    assert list(b) == list(a) + ['ema_state_dict', 'ema'] and b['ema'] == {'decay': 0.9999, 'warmup': True}
    assert list(b['ema_state_dict']) == list(b['state_dict']) == ['weight', 'bias']
    assert torch.equal(b['ema_state_dict']['weight'], model.weight.detach() + 1.0)
    assert all(torch.equal(a[k2][k], b[k2][k]) for k2 in ('state_dict',) for k in a[k2]) and a['iteration'] == b['iteration'] == 7
    capsys.readouterr()
    # load: the average is restored when the checkpoint has one and the optimiser keeps one
    opt = _StubAdam(True)
    assert TR.load_checkpoint(ema, model, opt)[3] == 7
    assert opt.calls == ['load_state_dict', ('load_ema_state_dict', ['bias', 'weight'])]
    assert 'ema_state_dict' not in capsys.readouterr().out
    opt = _StubAdam(True)
    TR.load_checkpoint(plain, model, opt)
    assert opt.calls == ['load_state_dict']
    assert capsys.readouterr().out.count("holds no 'ema_state_dict'") == 1            # one line says where the average starts
    for path in (plain, ema):                       # an optimiser without an average reads either file as it always did
        opt = _StubAdam(False)
        TR.load_checkpoint(path, model, opt)
        assert opt.calls == ['load_state_dict'] and 'ema_state_dict' not in capsys.readouterr().out
    opt = _StubAdam(True)
    TR.warm_start_model(ema, model, opt)
    assert opt.calls == ['reset_ema']
    TR.warm_start_model(ema, model)                 # the reference's two-argument call still works


def test_logger_writes_the_ema_validation_tag(tmp_path):
    from logger import Tacotron2Logger, read_events
    lg = Tacotron2Logger(str(tmp_path / 'logs'))
    lg.log_validation_ema(0.25, 500)
    lg.close()
    assert read_events(lg.path) == [(500, 'validation.loss.ema', 'scalar', 0.25)]


def test_new_entry_point_is_declared_and_bound_from_the_header():
    import t2v_abi
    import t2v_hip
    i, f, vp, u64 = C.c_int, C.c_float, C.c_void_p, C.c_uint64
    name = 't2v_clip_adam_ema_step_guarded'
    restype, argtypes = t2v_abi.load().prototypes[name]
    assert restype is i and argtypes == [vp, vp, vp, vp, u64] + [f] * 9 + [vp, vp, vp, i] + [vp, f, i, u64] + [vp]
    old = t2v_abi.load().prototypes['t2v_clip_adam_step_guarded'][1]
    assert argtypes[:len(old) - 1] == old[:-1] and argtypes[-1] is old[-1]                # the guarded step's arguments + four
    assert name in t2v_hip.EXPORTS
    fn = getattr(t2v_hip.load_library(), name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    # turned away on the host, before anything is launched: the pointers are host dummies
    buf = C.create_string_buffer(256)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    head = [p, p, p, p, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0.1, 0.001, p, p, None, 0]
    err = t2v_abi.load().define('T2V_ERR_ARG')
    assert fn(*(head + [None, 1e-4, 1, 0, None])) == err
    assert fn(*(head + [C.c_void_p(p.value + 4), 1e-4, 1, 0, None])) == err
    for rate in (0.0, -0.5, 1.5, float('nan')):
        assert fn(*(head + [p, rate, 1, 0, None])) == err
