"""The fp64 BatchNorm oracle of tests/bn_ref.py against torch (CPU, no GPU): equal to F.batch_norm in fp64 with autograd through
tanh / ReLU / identity and a multiplied keep-mask, in training and in eval, running statistics and the eval-mode bias gradient
included; its bounds are positive and scale with the inputs; an honest fp32 evaluation stays inside them and every mutation that a
case can see leaves them; the case table reaches every path with the slice count worked out by hand; and the number of ReLU
decisions the GPU test may excuse is (next to) none for the seeds it uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

SHAPES = ((2, 3, 5), (1, 4, 17), (3, 2, 1))


def _small(shape, seed):
    g = np.random.default_rng(seed)
    B, M, T = shape
    y = (g.standard_normal(shape) * 2 + 0.5).astype(np.float32)
    gamma, beta = g.uniform(0.5, 1.5, M).astype(np.float32), (0.1 * g.standard_normal(M)).astype(np.float32)
    rm, rv = g.standard_normal(M).astype(np.float32), g.uniform(0.5, 2, M).astype(np.float32)
    dout = g.standard_normal(shape).astype(np.float32)
    keep = (g.uniform(size=shape) >= 0.25) / 0.75
    return y, gamma, beta, rm, rv, dout, keep


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('act', (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU))
@pytest.mark.parametrize('training', (1, 0))
def test_oracle_equals_torch_fp64(shape, act, training):
    y, gamma, beta, rm, rv, dout, keep = _small(shape, 11 * sum(shape) + act)
    B, M, T = shape
    x, bias = _t(y).requires_grad_(True), torch.zeros(M, dtype=torch.float64, requires_grad=True)
    tg, tb = _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
    trm, trv = _t(rm), _t(rv)
    z = F.batch_norm(x + bias[None, :, None], trm, trv, tg, tb, bool(training), 0.1, R.EPS)
    a = torch.tanh(z) if act == R.ACT_TANH else torch.relu(z) if act == R.ACT_RELU else z
    out = a * _t(keep)
    out.backward(_t(dout))
    if training:
        st = R.stats(y, running_mean=rm, running_var=rv)
        assert np.abs(st.run_mean - trm.numpy()).max() < 1e-12 and np.abs(st.run_var - trv.numpy()).max() < 1e-12
        mean, rstd = st.mean, st.rstd
        # from block partials the same numbers (fp64 partials here: the oracle only adds what it is given)
        sp = R.stats(y, partials=R.block_partials(y, 3).astype(np.float64), running_mean=rm, running_var=rv)
        assert np.abs(sp.mean - mean).max() < 1e-6 and np.abs(sp.rstd - rstd).max() < 1e-5
    else:
        mean, (rstd, _) = rm.astype(np.float64), R.eval_rstd(rv)
    f = R.forward(y, mean, rstd, gamma, beta, act, keep_scale=keep)
    assert np.abs(f.out - out.detach().numpy()).max() < 1e-12
    b = R.backward(y, dout, mean, rstd, gamma, beta, act, not training, keep_scale=keep)
    assert np.abs(b.dy - x.grad.numpy()).max() < 1e-12
    assert np.abs(b.dgamma - tg.grad.numpy()).max() < 1e-12 and np.abs(b.dbeta - tb.grad.numpy()).max() < 1e-12
    assert np.abs(b.dbias - bias.grad.numpy()).max() < 1e-12            # exactly 0 in training, g S1 in eval
    if training:
        assert not b.dbias.any() and not b.e_dbias.any()
    assert (f.e_z > 0).all()
    live = np.abs(b.dz).sum(1) > 0              # (a channel whose every dz is exactly 0, ReLU on a tiny shape, has exact zero sums)
    assert (b.e_dgamma[live] > 0).all() and (b.e_dbeta[live] > 0).all() and not b.e_dbeta[~live].any()
    assert (f.e_out[keep != 0] > 0).all() and not f.e_out[keep == 0].any()           # a dropped element is exactly 0
    assert (b.e_dy >= 0).all() and (b.e_dy[b.dy != 0] > 0).all()


def test_fwd_len_contract():
    y, gamma, beta, rm, rv, _, _ = _small((3, 2, 6), 5)
    rstd, rel = R.eval_rstd(rv)
    f = R.forward(y, rm, rstd, gamma, beta, R.ACT_TANH, lengths=[0, 4, 9], rstd_rel=rel)
    full = R.forward(y, rm, rstd, gamma, beta, R.ACT_TANH, rstd_rel=rel)
    assert not f.out[0].any() and not f.out[1, :, 4:].any() and not f.e_out[1, :, 4:].any()
    assert np.array_equal(f.out[1, :, :4], full.out[1, :, :4]) and np.array_equal(f.out[2], full.out[2])
    m = R.forward(y, rm, rstd, gamma, beta, R.ACT_TANH, lengths=[0, 4, 9], mutate='pad_beta')
    assert np.array_equal(m.out[0], np.broadcast_to(beta.astype(np.float64)[:, None], (2, 6)))


def test_bounds_scale_with_the_inputs():
    y, gamma, beta, rm, rv, dout, keep = _small((2, 3, 40), 3)
    s = 8.0
    a, b = R.stats(y, eps=R.EPS), R.stats(y * np.float32(s), eps=R.EPS * s * s)
    assert np.allclose(b.e_mean, s * a.e_mean, rtol=1e-12) and np.allclose(b.e_rstd, a.e_rstd / s, rtol=1e-12)
    assert (a.e_mean > 0).all() and (a.e_rstd > 0).all() and (a.e_run_mean > 0).all() and (a.e_run_var > 0).all()
    pa = R.stats(y, partials=R.block_partials(y, 4))
    pb = R.stats(y * np.float32(s), partials=R.block_partials(y, 4) * np.float32([s, s * s]), eps=R.EPS * s * s)
    assert np.allclose(pb.e_mean, s * pa.e_mean, rtol=1e-12) and np.allclose(pb.e_rstd, pa.e_rstd / s, rtol=1e-12)
    assert (pa.e_rstd < a.e_rstd).all()                    # rounding only
    mean, rstd = R.stats32(y)
    for act in (R.ACT_NONE, R.ACT_RELU):
        f1 = R.forward(y, mean, rstd, gamma, beta, act, keep_scale=keep)
        f2 = R.forward(y, mean, rstd, gamma * np.float32(s), beta * np.float32(s), act, keep_scale=keep)
        assert np.allclose(f2.e_out, s * f1.e_out, rtol=1e-12)
    for act in (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU):
        for ev in (False, True):
            b1 = R.backward(y, dout, mean, rstd, gamma, beta, act, ev, keep_scale=keep)
            b2 = R.backward(y, dout * np.float32(s), mean, rstd, gamma, beta, act, ev, keep_scale=keep)
            for k in ('e_dy', 'e_dgamma', 'e_dbeta', 'e_dbias'):
                assert np.allclose(getattr(b2, k), s * getattr(b1, k), rtol=1e-12), (act, ev, k)
            # more serial adds, more slices: a wider bound on the sums, never a narrower one
            b3 = R.backward(y, dout, mean, rstd, gamma, beta, act, ev, keep_scale=keep, L=20, P=8)
            assert (b3.e_dbeta > b1.e_dbeta).all() and (b3.e_dy >= b1.e_dy).all()


def _fp32_apply(y, mean, rstd, gamma, beta, act):
    f = np.float32
    g = (gamma * rstd).astype(f)[None, :, None]
    bt = (beta - (mean * gamma).astype(f) * rstd).astype(f)[None, :, None]
    z = (y * g).astype(f) + bt
    return np.tanh(z).astype(f) if act == R.ACT_TANH else np.maximum(z, f(0)) if act == R.ACT_RELU else z


@pytest.mark.parametrize('name', ['fwd_reg_23x3x89_relu', 'fwd_reg_4x3x768_tanh_g40', 'fwd_reg_3x2x683_tanh', 'fwd_reg_4x3x768_tanh_c64'])
def test_honest_fp32_forward_is_inside_the_bounds_and_mutations_are_not(name):
    c = R.BY_NAME[name]
    inp = R.draw(c)
    st = R.stats(inp.y, running_mean=inp.run_mean, running_var=inp.run_var)
    yc = R.chan(inp.y).astype(np.float32)
    n = yc.shape[1]
    s32, q32 = yc.sum(1, dtype=np.float32), (yc * yc).sum(1, dtype=np.float32)          # numpy's pairwise fp32 sums
    mu = s32.astype(np.float64) / n
    var = np.maximum(q32.astype(np.float64) / n - mu * mu, 0)
    mean32, rstd32 = mu.astype(np.float32), (1 / np.sqrt(var + R.EPS)).astype(np.float32)
    assert R.ratio(mean32, st.mean, st.e_mean)[0] <= 1 and R.ratio(rstd32, st.rstd, st.e_rstd)[0] <= 1
    f = R.forward(inp.y, mean32, rstd32, inp.gamma, inp.beta, c.act)
    got = _fp32_apply(inp.y, mean32, rstd32, inp.gamma, inp.beta, c.act)
    assert np.isfinite(got).all() and R.ratio(got, f.out, f.e_out)[0] <= 1
    if c.gamma_hi > 1.5:
        assert np.abs(f.z).max() > 40 and (np.abs(got) == 1).any()                      # saturated: th = +-1 exactly
    drop = np.abs(yc).argmax(1)
    # (an offset of 64 spreads widens the variance bound by 64^2: the ill-conditioned cases are measured, not mutated)
    for m in ('stat_drop', 'biased_running_var', 'eps_1e-3') if c.cond <= 1 else ():
        mt = R.stats(inp.y, running_mean=inp.run_mean, running_var=inp.run_var, mutate=m, drop=drop)
        worst = max(R.ratio(mean32, mt.mean, mt.e_mean)[0], R.ratio(rstd32, mt.rstd, mt.e_rstd)[0],
                    R.ratio(st.run_var.astype(np.float32), mt.run_var, mt.e_run_var)[0])
        assert worst > 1, (m, worst)


@pytest.mark.parametrize('act', (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU))
@pytest.mark.parametrize('ev', (False, True))
def test_honest_fp32_backward_is_inside_the_bounds_and_mutations_are_not(act, ev):
    f = np.float32
    g = np.random.default_rng(act + 7)
    B, M, T = 4, 3, 300
    y = (g.standard_normal((B, M, T)) * 2 + 1).astype(f)
    gamma, beta = g.uniform(0.5, 1.5, M).astype(f), (0.1 * g.standard_normal(M)).astype(f)
    dout = g.standard_normal((B, M, T)).astype(f)
    keep = ((g.uniform(size=(B, M, T)) >= 0.25) / 0.75)
    if act == R.ACT_RELU:
        y, mean, rstd, _ = R.nudge_relu(y, gamma, beta)
    else:
        mean, rstd = R.stats32(y)
    ref = R.backward(y, dout, mean, rstd, gamma, beta, act, ev, keep_scale=keep)
    # the kernel's arithmetic in fp32
    gg = (gamma * rstd).astype(f)[None, :, None]
    z = _fp32_apply(y, mean, rstd, gamma, beta, R.ACT_NONE)
    xh = ((y - mean[None, :, None]).astype(f) * rstd[None, :, None]).astype(f)
    d = (dout * keep.astype(f)).astype(f)
    if act == R.ACT_TANH:
        th = np.tanh(z).astype(f)
        d = (d * (f(1) - th * th)).astype(f)
    elif act == R.ACT_RELU:
        d = np.where(z > 0, d, f(0))
    S1 = R.chan(d).astype(f).sum(1, dtype=f)
    S2 = (R.chan(d).astype(f) * R.chan(xh).astype(f)).sum(1, dtype=f)
    n = f(B * T)
    m1, m2 = (f(0) * S1, f(0) * S2) if ev else (S1 / n, S2 / n)
    dy = (gg * (d - m1[None, :, None] - xh * m2[None, :, None])).astype(f)
    got = dict(dy=dy, dgamma=S2, dbeta=S1, dbias=(gamma * rstd).astype(f) * S1 if ev else 0 * S1)
    for k in got:
        assert R.ratio(got[k], getattr(ref, k), getattr(ref, 'e_' + k))[0] <= 1, k
    muts = ['stat_drop', 'keep_per_channel'] + (['tanh_deriv'] if act == R.ACT_TANH else []) + \
        (['eval_keeps_batch_terms'] if ev else ['bias_nonzero_train'])
    for m in muts:
        ks = np.broadcast_to(keep[:, :1, :], keep.shape) if m == 'keep_per_channel' else keep
        mt = R.backward(y, dout, mean, rstd, gamma, beta, act, ev, keep_scale=ks, mutate=m, drop=np.abs(R.chan(d)).argmax(1))
        assert max(R.ratio(got[k], getattr(mt, k), getattr(mt, 'e_' + k))[0] for k in got) > 1, m


def test_case_table_reaches_every_path_with_the_planned_slices():
    assert set(c.path for c in R.CASES) == set(R.PATHS)
    for c in R.CASES:
        n = c.B * c.T
        sl, chunk = R.plan(c.kind == 'bwd', c.B, c.M, c.T, c.training, int(c.nblk > 0))
        assert sl == c.slices, (c.name, sl)
        if c.kind == 'len':
            continue
        want = 'split' if sl > 1 else 'reg' if n <= 3072 else 'loop'
        assert c.path.split('_')[-1] == want, c.name
        if sl > 1:
            assert (sl - 1) * chunk < n <= sl * chunk and chunk % 256 == 0
    # the boundaries the issue names, on both sides
    ns = lambda path: set(c.B * c.T for c in R.CASES if c.path == path)                               # noqa: E731
    assert {2, 255, 256, 257, 3071, 3072} <= ns('partials_reg') and {3073, 4097} <= ns('partials_loop')
    assert {2, 257, 2047, 2048, 2049, 3072} <= ns('reg') and {3073, 16383, 16384} <= ns('loop')
    assert {2, 257, 3072} <= ns('bwd_reg') and {3073, 8191, 8192} <= ns('bwd_loop') and {8192, 16391, 131073, 12000} <= ns('bwd_split')
    assert set(c.nblk for c in R.CASES if c.nblk) == {1, 3, 256, 257, 600}
    assert any(c.T == 1 for c in R.CASES) and any(c.B == 1 for c in R.CASES)
    # every mutation is seen by a mutation case of every path, or named as invisible to it
    for path in R.PATHS:
        mc = [c for c in R.CASES if c.path == path and c.mut]
        assert mc, path
        for m in R.MUTATIONS:
            assert any(R.visible(m, c) for c in mc) or not any(R.visible(m, c) for c in R.CASES if c.path == path), (path, m)


def test_relu_decisions_the_gpu_test_may_excuse_are_next_to_none():
    """forward ReLU cases: elements with |z_ref| <= E_z (either decision passes).  Expected about 0.8 E_z N of the standard normal
    density, far below one element; counted here for the very seeds the GPU test draws"""
    total = 0
    for c in R.CASES:
        if c.kind == 'bwd' or c.act != R.ACT_RELU:
            continue
        inp = R.draw(c)
        if c.training:
            mean, rstd = R.stats32(inp.y)
        else:
            mean, rstd = inp.run_mean, R.eval_rstd(inp.run_var)[0]
        k = int((R.relu_margin(inp.y, mean, rstd, inp.gamma, inp.beta) <= 1).sum())
        assert k <= max(2, 1e-4 * c.B * c.M * c.T), (c.name, k)
        total += k if c.cond <= 1 else 0        # (E_z grows with |mean g|: at a mean of 64 spreads a few elements fall inside it)
    assert total <= 2, total
