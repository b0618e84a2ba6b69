"""Host side of the guided attention switch (no GPU): the two recipe hparams, the criterion's argument check, the logger's tag and
the derived binding of the new entry points."""
import ctypes as C
import os

import pytest
import torch


def test_recipe_switches_default_off_and_parse():
    import hparams as HP
    hp = HP.create_hparams()
    assert hp.guided_attention_weight == 0.0 and hp.guided_attention_sigma == 0.4
    assert set(HP._RECIPE) == {'ema_decay', 'ema_warmup', 'guided_attention_weight', 'guided_attention_sigma'}
    on = HP.create_hparams("guided_attention_weight=1.0,guided_attention_sigma=0.3")
    assert on.guided_attention_weight == 1.0 and on.guided_attention_sigma == 0.3
    assert on.recipe()['guided_attention_weight'] == 1.0 and on.recipe()['guided_attention_sigma'] == 0.3
    assert on.values() == hp.values() and on.extensions() == hp.extensions()         # values() stays the reference's set
    with pytest.raises(ValueError):
        HP.create_hparams("guided_attention_weight=much")
    with pytest.raises(ValueError):
        HP.create_hparams("guided_attention=1.0")


def test_criterion_needs_lengths_when_the_term_is_on():
    import hparams as HP
    import loss_function as LF
    g = torch.Generator().manual_seed(0)
    out = [torch.randn(2, 80, 5, generator=g), torch.randn(2, 80, 5, generator=g), torch.randn(2, 5, generator=g),
           torch.softmax(torch.randn(2, 5, 9, generator=g), -1), torch.randn(2, 32, generator=g), torch.randn(2, 32, generator=g)]
    targets = (torch.randn(2, 80, 5, generator=g), torch.rand(2, 5, generator=g).round())
    off = LF.Tacotron2Loss_VAE(HP.create_hparams("anneal_function=constant"))
    on = LF.Tacotron2Loss_VAE(HP.create_hparams("anneal_function=constant,guided_attention_weight=0.5"))
    assert off.guided_weight == 0.0 and on.guided_weight == 0.5 and on.guided_sigma == 0.4
    base = off(out, targets, 0)
    assert len(base) == 4 and off.guided is None
    with pytest.raises(ValueError, match='lengths'):
        on(out, targets, 0)
    with torch.no_grad():           # validation: the term is left out, the loss is the reference's
        val = on(out, targets, 0, lengths=(torch.tensor([9, 4]), torch.tensor([5, 3])))
    assert torch.equal(val[0], base[0]) and on.guided is None


def test_training_tag_appears_only_when_given(tmp_path):
    import logger as L
    tags = {}
    for name, kw in (('off', {}), ('on', {'guided_attention': 0.125})):
        d = str(tmp_path / name)
        lg = L.Tacotron2Logger(d)
        lg.log_training(1.5, 0.25, 1e-3, 0.03, 1.4, 12.0, 0.001, 7, **kw)
        lg.close()
        ev = L.read_events(os.path.join(d, os.listdir(d)[0]))
        tags[name] = {t: v for s, t, k, v in ev if k == 'scalar'}
    assert 'training.guided_attention' not in tags['off']
    assert tags['on']['training.guided_attention'] == 0.125
    assert set(tags['on']) - set(tags['off']) == {'training.guided_attention'}


def test_new_entry_points_are_bound_from_the_header():
    import t2v_abi
    protos = t2v_abi.load().prototypes
    i, l, f, vp, u64 = C.c_int, C.c_long, C.c_float, C.c_void_p, C.c_uint64
    assert protos['t2v_guided_attention'] == (i, [vp, l, l, l, vp, vp, vp, vp, vp, i, i, i, f, vp])
    assert protos['t2v_guided_attention_part_doubles'] == (l, [i, i])
    for old, at in (('t2v_decoder_train_bwd', 3), ('t2v_decoder_bwd_achain', 4), ('t2v_decoder_bwd_achain_prepared', 4),
                    ('t2v_decoder_bwd_persistent16', 3), ('t2v_decoder_bwd_persistent16_prepared', 3)):
        res, args = protos[old]
        res2, args2 = protos[old + '_align']
        assert res2 is res and args2 == args[:at] + [vp] + args[at:], old           # the same call with dAL behind dHC / the buffers
