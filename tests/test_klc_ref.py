"""The fp64 reference of the KL control (tests/klc_ref.py) against the oracle and against its own definition, the conditions its
inputs keep so that round-off decides no case, the cyclical KL weight at hand-computed steps, and the host side of the new
hyper-parameters.  No GPU."""
import numpy as np
import pytest
import torch

import klc_ref as R

W = 0.001           # the oracle's 'constant' KL weight


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("B", R.BATCHES)
def test_reference_with_both_switches_off_is_the_oracle(B):
    import t2v_oracle as O
    t = R.inputs(B)
    leaves = [x.double().clone().requires_grad_(True) for x in t[:5]]
    total, recon, kl, w = O.loss_forward([leaves[0], leaves[1], leaves[2], None, leaves[3], leaves[4]], t[5].double(),
                                         t[6].double(), 0, 'constant')
    assert w == W
    total.backward()
    ref = R.objective(t, W)
    for name, want in (('total', total), ('recon', recon), ('kl', kl), ('kp', kl), ('T', kl)):
        assert abs(float(ref[name]) - float(want.detach())) <= 1e-12 * abs(float(want.detach())), name
    assert ref['s'] == 1.0 and ref['n_floored'] == 0
    for g, leaf in zip(ref['grads'], leaves):
        assert (g - leaf.grad).abs().max() <= 1e-12 * leaf.grad.abs().max()


@pytest.mark.parametrize("B", R.BATCHES)
def test_floored_dimensions_have_zero_gradient_and_the_others_the_reference_gradient(B):
    t = R.inputs(B)
    off, on = R.objective(t, W), R.objective(t, W, free_bits=R.LAMBDA)
    fl = on['floored']
    assert 12 <= int(fl.sum()) <= 15 and on['n_floored'] == int(fl.sum())
    for i in (3, 4):            # dmu, dlogvar
        assert (on['grads'][i][:, fl] == 0.0).all()
        a, b = on['grads'][i][:, ~fl], off['grads'][i][:, ~fl]
        assert ((a - b).abs() <= 4e-16 * b.abs()).all()         # (B * (1 / B) in the mean's gradient: an ulp at most)
    for i in (0, 1, 2):
        assert torch.equal(on['grads'][i], off['grads'][i])
    want = B * (torch.where(fl, torch.full_like(on['k'], R.LAMBDA), on['k'])).sum()
    assert float(on['kp']) == float(want) and float(on['kp']) > float(on['kl']) and float(on['kl']) == float(off['kl'])
    assert abs(float(on['total']) - (float(on['recon']) + W * float(on['kp']))) <= 1e-12 * abs(float(on['total']))


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("free_bits", (0.0, R.LAMBDA))
def test_the_sign_flips_the_latent_gradients_and_nothing_else(B, free_bits):
    t = R.inputs(B)
    plain = R.objective(t, W, free_bits=free_bits)
    below, above = (R.objective(t, W, free_bits=free_bits, capacity=c) for c in R.CAPACITIES)
    assert below['s'] == 1.0 and above['s'] == -1.0
    for o in (below, above):
        assert float(o['kp']) == float(plain['kp']) and torch.equal(o['floored'], plain['floored'])
        for i in (0, 1, 2):
            assert torch.equal(o['grads'][i], plain['grads'][i])
    for i in (3, 4):
        assert torch.equal(below['grads'][i], plain['grads'][i])
        assert torch.equal(above['grads'][i], -plain['grads'][i])
    for o, c in zip((below, above), R.CAPACITIES):
        assert abs(float(o['T']) - abs(float(o['kp']) - B * c)) <= 1e-12 * float(o['T'])
    # at equality the sign, and with it every latent gradient, is 0
    eq = R.objective(t, W, free_bits=free_bits, capacity=float(plain['kp']) / B)
    if float(eq['T']) == 0.0:
        assert eq['s'] == 0.0 and all(float(eq['grads'][i].abs().max()) == 0.0 for i in (3, 4))


@pytest.mark.parametrize("B", R.BATCHES)
def test_input_conditions_keep_round_off_from_deciding_a_case(B):
    t = R.inputs(B)
    f64 = R.objective(t, W, free_bits=R.LAMBDA)
    f32 = R.objective(t, W, free_bits=R.LAMBDA, dtype=torch.float32)
    margin = R.floor_margin(f64['k'], R.LAMBDA)
    print("B %d seed %d: floor margin %.4f, floored %d, K'/B %.2f" % (B, R.seed_of(B), margin, f64['n_floored'], float(f64['kp']) / B))
    assert margin >= 0.01
    assert torch.equal(f64['floored'], f32['floored'])
    for free_bits in (0.0, R.LAMBDA):
        per_item = float(R.objective(t, W, free_bits=free_bits)['kp']) / B
        assert 60.0 <= per_item <= 155.0
        for c in R.CAPACITIES:
            assert abs(per_item - c) >= 0.1 * c
    assert R.CAPACITIES[0] < float(f64['kp']) / B < R.CAPACITIES[1]
    assert torch.equal(R.inputs(B, 400)[3], t[3]) and torch.equal(R.inputs(B, 400)[4], t[4])     # latents depend on B alone


def test_monitor_reference_is_the_statistics_of_all_rows():
    rng = np.random.RandomState(5)
    batches = [(rng.randn(b, 4).astype(np.float32), (0.3 * rng.randn(b, 4)).astype(np.float32)) for b in (3, 1, 7)]
    ref = R.monitor_reference(batches)
    rows = np.concatenate([m for m, _ in batches]).astype(np.float64)
    assert ref['n'] == 11 and ref['launches'] == 3
    assert np.allclose(ref['mean'], rows.mean(0), rtol=1e-14) and np.allclose(ref['m2'], rows.var(0) * 11, rtol=1e-13)
    import latent_scores
    lvs = np.concatenate([v for _, v in batches])
    assert np.allclose(ref['sum_kl'] / 11, latent_scores.kl_per_dim(rows, lvs), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ cyclical annealing
def test_cyclical_weight_at_hand_computed_steps():
    from loss_function import kl_anneal_weight as kw
    args = dict(lag=50000, k=0.0025, x0=10000, upper=0.2, cycle=1000, ratio=0.5)
    assert kw('cyclical', 0, **args) == 0.0                       # cycle start
    assert kw('cyclical', 250, **args) == pytest.approx(0.1, rel=1e-15)     # mid-ramp: 0.2 * (0.25 / 0.5)
    assert kw('cyclical', 500, **args) == 0.2                     # end of the ramp
    assert kw('cyclical', 999, **args) == 0.2                     # last step of the cycle: held
    assert kw('cyclical', 1000, **args) == 0.0                    # first step of the next
    assert kw('cyclical', 1001, **args) == pytest.approx(0.2 * 0.001 / 0.5, rel=1e-15)
    assert kw('cyclical', 1250, **args) == kw('cyclical', 250, **args)
    args.update(cycle=4, ratio=0.25)
    assert [kw('cyclical', s, **args) for s in range(6)] == [0.0, 0.2, 0.2, 0.2, 0.0, 0.2]
    # the three reference names and the None of an unknown one stay what they were
    old = dict(lag=50000, k=0.0025, x0=10000, upper=0.2)
    assert kw('constant', 7, **old) == 0.001 and kw('linear', 100, **old) == 0 and kw('linear', 60000, **old) == 0.2
    assert kw('logistic', 10000, **old) == pytest.approx(0.2 / 1.2, rel=1e-15)
    assert kw('cosine', 3, **old) is None and kw('cosine', 3, **args) is None


def test_criterion_follows_the_cycle_of_its_hparams():
    import hparams as HP
    from loss_function import Tacotron2Loss_VAE
    crit = Tacotron2Loss_VAE(HP.create_hparams("anneal_function=cyclical,anneal_cycle=4"))
    assert [crit.kl_weight(s) for s in range(6)] == [0.0, 0.1, 0.2, 0.2, 0.0, 0.1]
    assert crit.kl_anneal_function('cyclical', 50000, 5, 0.0025, 10000, 0.2) == 0.1
    default = Tacotron2Loss_VAE(HP.create_hparams())
    assert default.kl_weight(12345) == default.kl_anneal_function('logistic', 50000, 12345, 0.0025, 10000, 0.2)
    assert not default.kl_control and default.monitor is None


# ------------------------------------------------------------------------------------------------ hyper-parameters
NEW = {'kl_free_bits': 0.0, 'kl_capacity': -1.0, 'anneal_cycle': 10000, 'anneal_ratio': 0.5, 'kl_monitor': False}


def test_new_hparams_parse_and_unset_ones_appear_in_no_listing():
    import hparams as HP
    hp = HP.create_hparams()
    for k, v in NEW.items():
        assert getattr(hp, k) == v and type(getattr(hp, k)) is type(v)
        assert k not in hp and k not in hp.values() and k not in hp.recipe() and k not in hp.extensions()
    assert hp.recipe() == {'ema_decay': 0.0, 'ema_warmup': True}
    hp = HP.create_hparams("kl_free_bits=0.05,kl_capacity=20,anneal_function=cyclical,anneal_cycle=4,anneal_ratio=0.25,kl_monitor=True")
    assert (hp.kl_free_bits, hp.kl_capacity, hp.anneal_cycle, hp.anneal_ratio, hp.kl_monitor) == (0.05, 20.0, 4, 0.25, True)
    assert type(hp.kl_capacity) is float and type(hp.anneal_cycle) is int
    assert set(NEW) <= set(hp.recipe()) and not set(NEW) & set(hp.values())
    assert hp.values() == dict(HP.create_hparams().values(), anneal_function='cyclical')
    with pytest.raises(ValueError, match='unknown hparam'):
        HP.create_hparams("kl_freebits=0.05")


def test_criterion_refuses_a_negative_floor_and_an_empty_cycle():
    import hparams as HP
    from loss_function import Tacotron2Loss_VAE
    with pytest.raises(ValueError, match='kl_free_bits'):
        Tacotron2Loss_VAE(HP.create_hparams("kl_free_bits=-0.1"))
    with pytest.raises(ValueError, match='anneal_cycle'):
        Tacotron2Loss_VAE(HP.create_hparams("anneal_cycle=0"))
    crit = Tacotron2Loss_VAE(HP.create_hparams("kl_free_bits=0.05"))
    assert crit.kl_control and crit.free_bits == 0.05 and crit.capacity == -1.0
    assert Tacotron2Loss_VAE(HP.create_hparams("kl_capacity=0")).kl_control


# ------------------------------------------------------------------------------------------------ logger, binding
def test_kl_tags_appear_only_when_given(tmp_path):
    import os
    import logger as L
    tags = {}
    for name, kw in (('off', {}), ('on', {'kl_objective': 45.5, 'kl_floored_dims': 13})):
        d = str(tmp_path / name)
        lg = L.Tacotron2Logger(d)
        lg.log_training(1.5, 0.25, 1e-3, 0.03, 1.4, 12.0, 0.001, 7, **kw)
        lg.close()
        ev = L.read_events(os.path.join(d, os.listdir(d)[0]))
        tags[name] = {t: v for s, t, k, v in ev if k == 'scalar'}
    assert set(tags['on']) - set(tags['off']) == {'training.kl_objective', 'training.kl_floored_dims'}
    assert tags['on']['training.kl_objective'] == 45.5 and tags['on']['training.kl_floored_dims'] == 13.0
    assert set(tags['off']) == {'training.loss', 'grad.norm', 'learning.rate', 'duration', 'kl_div', 'kl_weight', 'recon_loss'}
    import inspect
    assert inspect.signature(L.Tacotron2Logger.log_validation).parameters['kl_active_units'].default is None


def test_new_entry_point_is_bound_from_the_header():
    import ctypes as C
    import t2v_abi
    abi = t2v_abi.load()
    i, f, vp = C.c_int, C.c_float, C.c_void_p
    assert abi.prototypes['t2v_loss_fwd_bwd_klc'] == (i, [vp] * 16 + [C.c_uint64, i, i, i, f, f, f, vp])
    assert len(abi.layouts) == 12 and C.sizeof(abi.classes['t2v_step_params']) == 32       # no new struct, the record as it was
    res, args = abi.prototypes['t2v_loss_fwd_bwd']
    assert args == [vp] * 15 + [C.c_uint64, i, i, f, vp]
