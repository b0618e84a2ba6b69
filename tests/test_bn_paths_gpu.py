"""Every path of csrc/bn_act.hip through the C ABI (t2v_bn_act_fwd, _fwd_len, _bwd, _bwd_eval; no convolution in front), element by
element against the fp64 oracle of tests/bn_ref.py and its per-output worst-case bounds.

Each case of bn_ref.CASES first asserts the slice count t2v_bn_act_slices plans (worked out by hand in the case table), prefills every
output with NaN, runs twice and requires the same bits, then holds every output to the oracle's bound: mean_out, rstd_out and the
running buffers against the statistics oracle, out against the apply oracle evaluated at the DEVICE's saved mean / rstd, dy, dgamma,
dbeta and dconv_bias against the backward oracle.  No step record is installed (tests/conftest.py releases any), so the by-value
seed is what the kernels use and the keep-masks are drop_ref.conv_keep's.  Forward ReLU elements whose pre-activation is within its
own bound of 0 are excused from the element comparison (counted, capped); the backward's inputs are nudged off the threshold instead.
The exact cases (all values small integers or powers of two, so every fp32 sum is exact) prove that every element is counted once:
y = 1 everywhere, a single 1 at every slice / item / register boundary, a single 1 in dout.  The cases marked `mut` are then judged
against every mutated oracle: each must be rejected, or is named as invisible to that path.

One line per case is printed before it is asserted (profiles/bn_parity.txt is that output of an MI355X run); no bound is taken
from it."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p_ in (os.path.join(ROOT, 'tacotron2-vae_amd'), os.path.join(ROOT, 'tests')):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import bn_ref as R                                                        # noqa: E402
import drop_ref                                                           # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
RSTD_ONES = F32(1.0 / math.sqrt(R.EPS))          # var = 0: 1 / sqrt(eps) at the fp32 eps the call passes (316.22778)
KEEP_09 = F32(1.0) - F32(0.1)                    # the kernel's 1.f - momentum


def _lib():
    import t2v_hip
    return t2v_hip.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def _keep_scale(c, per_channel=False):
    """fp64 factors 0 or 1 / (1 - p) of the launch's keep-mask; per_channel: the mutation that indexes the mask by b * T + t"""
    if c.p <= 0 or (c.kind == 'fwd' and not c.training):
        return None
    if per_channel:
        k = np.broadcast_to(drop_ref.conv_keep(R.SEED, R.STREAM, R.RNG_T, c.B, 1, c.T, c.p).numpy(), (c.B, c.M, c.T))
    else:
        k = drop_ref.conv_keep(R.SEED, R.STREAM, R.RNG_T, c.B, c.M, c.T, c.p).numpy()
    return k / (1.0 - float(F32(c.p)))


def run_fwd(lib, B, M, T, y, gamma, beta, run_mean, run_var, act=0, training=1, p=0.0, partials=None, lengths=None):
    """t2v_bn_act_fwd / _fwd_len twice on NaN-prefilled outputs -> (dict of numpy outputs of the first run, same bits?)"""
    yd, gd, bd, pd, ld = _dev(y), _dev(gamma), _dev(beta), _dev(partials), _dev(lengths)
    runs = []
    for _ in range(2):
        rm, rv, out = _dev(run_mean), _dev(run_var), _nan(B, M, T)
        mean, rstd = (_nan(M), _nan(M)) if training else (None, None)
        if lengths is not None:
            rc = lib.t2v_bn_act_fwd_len(_p(yd), _p(gd), _p(bd), _p(rm), _p(rv), _p(out), _p(ld), B, M, T, act, 1e-5, _stream())
        else:
            rc = lib.t2v_bn_act_fwd(_p(yd), _p(pd), partials.shape[0] if partials is not None else 0, _p(gd), _p(bd), _p(rm), _p(rv),
                                    _p(mean), _p(rstd), _p(out), B, M, T, act, training, float(p), 0.1, 1e-5, R.SEED, R.STREAM, R.RNG_T,
                                    _stream())
        assert rc == 0
        runs.append(dict(out=out, run_mean=rm, run_var=rv, **(dict(mean=mean, rstd=rstd) if training else {})))
    torch.cuda.synchronize()
    a, b = [dict((k, v.cpu().numpy()) for k, v in r.items()) for r in runs]
    return a, _same_bits(a, b)


def run_bwd(lib, B, M, T, y, dout, mean, rstd, gamma, beta, act=0, training=1, p=0.0, bias=1):
    yd, dd, md, rd, gd, bd = _dev(y), _dev(dout), _dev(mean), _dev(rstd), _dev(gamma), _dev(beta)
    fn = lib.t2v_bn_act_bwd if training else lib.t2v_bn_act_bwd_eval
    runs = []
    for _ in range(2):
        dy, dg, db, dbias = _nan(B, M, T), _nan(M), _nan(M), _nan(M) if bias else None
        assert fn(_p(yd), _p(dd), _p(md), _p(rd), _p(gd), _p(bd), _p(dy), _p(dg), _p(db), _p(dbias), B, M, T, act, float(p),
                  R.SEED, R.STREAM, R.RNG_T, _stream()) == 0
        runs.append(dict(dy=dy, dgamma=dg, dbeta=db, **(dict(dbias=dbias) if bias else {})))
    torch.cuda.synchronize()
    a, b = [dict((k, v.cpu().numpy()) for k, v in r.items()) for r in runs]
    return a, _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ judging

def _mut_drop(c, m, chunk, big):
    """the element a 'stat_drop' / 'slice_late' oracle leaves out: the channel's largest, or the first of slice 1"""
    return big if m == 'stat_drop' else chunk if m == 'slice_late' else None


def judge_fwd(c, inp, got, mutate=None):
    """rows {output: (worst error / bound, worst error)} and the number of excused ReLU elements"""
    sl, chunk = R.plan(0, c.B, c.M, c.T, c.training, int(c.nblk > 0))
    rows, rel = {}, 0.0
    if c.kind == 'fwd' and c.training:
        st = R.stats(inp.y, partials=inp.partials, n_wg=chunk if sl > 1 else None, running_mean=inp.run_mean, running_var=inp.run_var,
                     mutate=mutate, drop=_mut_drop(c, mutate, chunk, np.abs(R.chan(inp.y)).argmax(1)))
        for k, ref, e in (('mean', st.mean, st.e_mean), ('rstd', st.rstd, st.e_rstd), ('run_mean', st.run_mean, st.e_run_mean),
                          ('run_var', st.run_var, st.e_run_var)):
            rows[k] = R.ratio(got[k], ref, e)
        mean, rstd = got['mean'], got['rstd']
    else:
        mean = inp.run_mean
        rstd, rel = R.eval_rstd(inp.run_var, mutate=mutate)
        for k, old in (('run_mean', inp.run_mean), ('run_var', inp.run_var)):        # eval leaves the buffers alone
            rows[k] = R.ratio(got[k], old.astype(np.float64), 0.0)
    f = R.forward(inp.y, mean, rstd, inp.gamma, inp.beta, c.act, keep_scale=_keep_scale(c, mutate == 'keep_per_channel'),
                  lengths=inp.lengths, rstd_rel=rel, mutate=mutate)
    excuse = (np.abs(f.z) <= f.e_z) if c.act == R.ACT_RELU else None
    rows['out'] = R.ratio(got['out'], f.out, f.e_out, excuse)
    if inp.lengths is not None:     # padded positions: +0.0, the bits
        pad = np.arange(c.T)[None, None, :] >= inp.lengths.reshape(c.B, 1, 1)
        pad = np.broadcast_to(pad, got['out'].shape)
        if mutate is None:
            assert not got['out'].view(np.int32)[pad].any(), 'a padded position is not +0.0'
    return rows, int(excuse.sum()) if excuse is not None else 0


def prep_bwd(c, inp):
    """what the backward is handed: y (nudged off the ReLU threshold), the fp32 batch statistics of that y, how many were moved"""
    if c.act == R.ACT_RELU:
        return R.nudge_relu(inp.y, inp.gamma, inp.beta)
    mean, rstd = R.stats32(inp.y)
    return inp.y, mean, rstd, 0


def judge_bwd(c, y, inp, mean, rstd, got, mutate=None, base=None):
    sl, chunk = R.plan(1, c.B, c.M, c.T)
    L, P = (math.ceil(chunk / 256), sl) if sl > 1 else (math.ceil(c.B * c.T / 256), 1)
    drop = _mut_drop(c, mutate, chunk, np.abs(base.dz).argmax(1) if base is not None else None)
    ref = R.backward(y, inp.dout, mean, rstd, inp.gamma, inp.beta, c.act, not c.training,
                     keep_scale=_keep_scale(c, mutate == 'keep_per_channel'), L=L, P=P, mutate=mutate, drop=drop)
    rows = dict((k, R.ratio(got[k], getattr(ref, k), getattr(ref, 'e_' + k))) for k in got)
    return rows, ref


def _line(tag, c, sl, rows, extra=''):
    k = max(rows, key=lambda r: (rows[r][0] if rows[r][0] == rows[r][0] else float('inf')))
    ratio, err = rows[k]
    return '%s %-50s path %-13s slices %2d  worst %-8s err %.3e  bound %.3e  ratio %.4f%s' % (
        tag, c.name, c.path, sl, k, err, err / ratio if ratio > 0 and math.isfinite(ratio) else 0.0, ratio, extra)


def _ok(rows):
    return all(r[0] <= 1.0 for r in rows.values())


def _slices(lib, c):
    return lib.t2v_bn_act_slices(int(c.kind == 'bwd'), c.B, c.M, c.T, c.training, int(c.nblk > 0))


# ------------------------------------------------------------------------------------------------ bounded cases and mutations

@pytest.mark.parametrize('name', [c.name for c in R.CASES])
def test_path_and_parity(name):
    lib = _lib()
    c = R.BY_NAME[name]
    inp = R.draw(c)
    N = c.B * c.M * c.T
    sl = _slices(lib, c) if c.kind != 'len' else 1
    assert sl == c.slices, (sl, c.slices)
    if c.kind == 'bwd':
        y, mean, rstd, moved = prep_bwd(c, inp)
        got, same = run_bwd(lib, c.B, c.M, c.T, y, inp.dout, mean, rstd, inp.gamma, inp.beta, c.act, c.training, c.p, c.bias)
        rows, base = judge_bwd(c, y, inp, mean, rstd, got)
        print(_line('bn-path', c, sl, rows, '  nudged %d/%d' % (moved, N)))
        if c.gamma_hi > 1.5 and not c.training:     # eval: dy = g dz, and 1 - th^2 is exactly 0 where tanh has saturated
            sat = np.abs(R.forward(y, mean, rstd, inp.gamma, inp.beta, c.act).z) > 20
            assert sat.any() and np.isfinite(got['dy']).all() and not got['dy'][sat].any()
    else:
        got, same = run_fwd(lib, c.B, c.M, c.T, inp.y, inp.gamma, inp.beta, inp.run_mean, inp.run_var, c.act, c.training, c.p,
                            inp.partials, inp.lengths)
        rows, excused = judge_fwd(c, inp, got)
        print(_line('bn-path', c, sl, rows, '  excused %d/%d' % (excused, N)))
        assert excused <= max(2, 1e-4 * N), excused
        if c.gamma_hi > 1.5:        # saturation: th = +-1 exactly, nothing but finite numbers
            assert np.isfinite(got['out']).all() and (np.abs(got['out']) == 1).any()
    assert same, 'two runs differ'
    assert _ok(rows), rows
    if not c.mut:
        return
    for m in R.MUTATIONS:
        if not R.visible(m, c):
            print('bn-mutation %-50s %-24s invisible to this case' % (c.name, m))
            continue
        mrows = judge_bwd(c, y, inp, mean, rstd, got, m, base)[0] if c.kind == 'bwd' else judge_fwd(c, inp, got, m)[0]
        worst = max((r[0] if r[0] == r[0] else float('inf')) for r in mrows.values())
        print('bn-mutation %-50s %-24s %12.1f bounds' % (c.name, m, worst))
        assert worst > 1.0, (m, mrows)


def test_every_path_was_asserted_and_sees_or_names_every_mutation():
    lib = _lib()
    assert set(c.path for c in R.CASES) == set(R.PATHS)
    for c in R.CASES:
        if c.kind != 'len':
            assert _slices(lib, c) == c.slices == R.plan(c.kind == 'bwd', c.B, c.M, c.T, c.training, int(c.nblk > 0))[0], c.name
    for path in R.PATHS:
        mc = [c for c in R.CASES if c.path == path and c.mut]
        for m in R.MUTATIONS:
            seen = any(R.visible(m, c) for c in mc)
            if not seen:
                assert not any(R.visible(m, c) for c in R.CASES if c.path == path), (path, m)
                print('bn-mutation path %-13s %-24s invisible to this path' % (path, m))
    # the plan's thresholds, either side
    q = lib.t2v_bn_act_slices
    assert (q(0, 1, 1, 16383, 1, 0), q(0, 1, 1, 16384, 1, 0), q(0, 1, 129, 16384, 1, 0), q(0, 1, 128, 16384, 1, 0)) == (1, 4, 1, 4)
    assert (q(0, 1, 1, 16384, 0, 0), q(0, 1, 1, 16384, 1, 1)) == (1, 1)                 # eval, partials: never cut forward
    assert (q(1, 1, 1, 8191, 1, 0), q(1, 1, 1, 8192, 1, 0), q(1, 1, 129, 8192, 1, 0), q(1, 1, 1, 8192, 0, 1)) == (1, 4, 1, 4)
    assert q(0, 0, 1, 5, 1, 0) < 0 and q(1, 1, 0, 5, 1, 0) < 0 and q(1, 1, 1, 0, 1, 0) < 0


def test_ill_conditioned_channels_are_measured():
    """rstd_out of channels whose mean is 8 / 64 spreads, relative to the well-conditioned case of the same shape and path.
    Nothing is asserted beyond the bounds test_path_and_parity holds these cases to: q / n - mu^2 stays as it is."""
    lib = _lib()

    def rel_err(c):
        inp = R.draw(c)
        got, _ = run_fwd(lib, c.B, c.M, c.T, inp.y, inp.gamma, inp.beta, inp.run_mean, inp.run_var, c.act, 1, c.p)
        sl, chunk = R.plan(0, c.B, c.M, c.T)
        st = R.stats(inp.y, n_wg=chunk if sl > 1 else None)
        return float(np.abs(got['rstd'] / st.rstd - 1).max()), float((st.e_rstd / st.rstd).max())

    for path, well in R.WELL.items():
        w, wb = rel_err(R.BY_NAME[well])
        for c in R.CASES:
            if c.kind == 'fwd' and c.path == path and c.cond > 1:
                e, b = rel_err(c)
                print('bn-cond path %-6s %dx%dx%d c = %2g std: rstd_out relative error %.3e (bound %.3e), well-conditioned %.3e (bound %.3e), '
                      'ratio %.1f' % (path, c.B, c.M, c.T, c.cond, e, b, w, wb, e / max(w, R.U / 4)))
                assert e <= b


# ------------------------------------------------------------------------------------------------ exact cases

def _boundaries(n, T, chunk, extra=()):
    """first and last element of every slice, n - 1, either side of the item boundaries, 3071 / 3072, the 2048-element passes"""
    s = {0, n - 1, T - 1, T, n - T - 1, n - T, 3071, 3072, 2047, 2048, 255, 256}
    for lo in range(0, n, chunk):
        s |= {lo, min(n, lo + chunk) - 1}
    return sorted(i for i in s | set(extra) if 0 <= i < n)


FWD_EXACT = (('partials_reg', 3, 2, 1024, 3), ('partials_loop', 1, 2, 4097, 600), ('reg', 4, 3, 768, 0), ('reg', 257, 2, 1, 0),
             ('loop', 7, 2, 439, 0), ('loop', 3, 2, 5461, 0), ('split', 1, 1, 16384, 0), ('split', 443, 128, 37, 0),
             ('split', 7, 100, 2400, 0), ('split', 1, 3, 258050, 0))


@pytest.mark.parametrize('path,B,M,T,nblk', FWD_EXACT)
def test_exact_all_ones(path, B, M, T, nblk):
    """y = 1: mean_out == 1, rstd_out == float(1 / sqrt(eps)), out == beta, running_var == 0.9 old, to the bit, on every path"""
    lib = _lib()
    n = B * T
    y = np.ones((B, M, T), dtype=F32)
    gamma = np.where(np.arange(M) % 2 == 0, 1.0, 2.0).astype(F32)
    beta = ((np.arange(M) % 7 - 3) * 2.0 ** -10).astype(F32)
    rv0 = (2.0 ** (np.arange(M) % 3 - 1)).astype(F32)
    part = R.block_partials(y, nblk) if nblk else None
    assert lib.t2v_bn_act_slices(0, B, M, T, 1, int(nblk > 0)) == R.plan(0, B, M, T, 1, int(nblk > 0))[0]
    got, same = run_fwd(lib, B, M, T, y, gamma, beta, np.zeros(M, dtype=F32), rv0, R.ACT_NONE, 1, 0.0, part)
    assert same
    assert np.array_equal(got['mean'], np.ones(M, dtype=F32))
    assert np.array_equal(got['rstd'], np.full(M, RSTD_ONES))
    assert np.array_equal(got['out'], np.broadcast_to(beta[None, :, None], (B, M, T)))
    assert np.array_equal(got['run_var'], KEEP_09 * rv0) and np.array_equal(got['run_mean'], np.full(M, F32(0.1)))
    print('bn-exact all ones      %-13s %dx%dx%d: mean 1, rstd %.5f, out = beta, running_var = 0.9 old' % (path, B, M, T, RSTD_ONES))


def _single_one_runs(B, M, T, idx):
    """inputs (B, M, T) of zeros with a single 1 per channel, channel m at flat index idx[m] of its B*T values; as many launches as
    the indices need"""
    for lo in range(0, len(idx), M):
        use = [idx[min(lo + m, len(idx) - 1)] for m in range(M)]
        a = np.zeros((M, B * T), dtype=F32)
        a[np.arange(M), use] = 1
        yield use, np.ascontiguousarray(R.unchan(a, B, T))


@pytest.mark.parametrize('path,B,M,T,nblk', [r for r in FWD_EXACT if r[0] != 'partials_reg'])
def test_exact_single_one(path, B, M, T, nblk):
    """a single 1 at every boundary index (with partials: in every boundary block): mean_out == float(1 / n) and rstd_out is that of
    var = 1 / n - 1 / n^2, so the element was counted once and only once"""
    lib = _lib()
    n = B * T
    sl, chunk = R.plan(0, B, M, T, 1, int(nblk > 0))
    gamma, beta, zero, one = np.ones(M, dtype=F32), np.zeros(M, dtype=F32), np.zeros(M, dtype=F32), np.ones(M, dtype=F32)
    if (B, M, T) == (1, 3, 258050):             # three channels a launch: the first slices and the short last one
        idx = [0, chunk - 1, chunk, (sl - 1) * chunk - 1, (sl - 1) * chunk, n - 1]
    elif nblk:
        idx = [0, 255, 256, 511, 512, nblk - 1]
    else:
        idx = _boundaries(n, T, chunk)
    want_rstd = 1.0 / math.sqrt(1.0 / n - 1.0 / (n * float(n)) + R.EPS)
    launches = 0
    for use, a in _single_one_runs(B, M, T, idx):
        part = None
        if nblk:                                # the statistics are the partials': a single [1, 1] in block use[m] of channel m
            part = np.zeros((nblk, M, 2), dtype=F32)
            part[use, np.arange(M), :] = 1
        got, same = run_fwd(lib, B, M, T, a, gamma, beta, zero, one, R.ACT_NONE, 1, 0.0, part)
        launches += 1
        assert same
        assert np.array_equal(got['mean'], np.full(M, F32(1.0 / n))), (use, got['mean'])
        assert (np.abs(got['rstd'].astype(np.float64) - want_rstd) <= np.spacing(F32(want_rstd))).all(), (use, got['rstd'])
        assert np.isfinite(got['out']).all()
    print('bn-exact single one    %-13s %dx%dx%d: %d boundary indices in %d launches, mean_out == 1/n' % (path, B, M, T, len(idx), launches))


BWD_EXACT = (('bwd_reg', 3, 6, 1024), ('bwd_reg', 257, 2, 1), ('bwd_loop', 7, 8, 439), ('bwd_loop', 1, 8, 8191), ('bwd_split', 1, 1, 8192),
             ('bwd_split', 443, 128, 37), ('bwd_split', 1, 1, 131073), ('bwd_split', 5, 100, 2400))


@pytest.mark.parametrize('path,B,M,T', BWD_EXACT)
@pytest.mark.parametrize('training', (1, 0), ids=('train', 'eval'))
def test_exact_backward_single_one(path, B, M, T, training):
    """act none, gamma rstd = 1, mean = 0, dout a single 1 at a boundary index i: dbeta == 1 and dgamma == y[i] exactly.  Then, y of
    zeros and ones with y[i] = 1: S1 = S2 = 1, and dy at every other element is -(1 + y) fl(1 / n), half an ulp from the oracle, in
    EVERY slice of the channel: all workgroups of a split channel used the same S1 / S2."""
    lib = _lib()
    n = B * T
    sl, chunk = R.plan(1, B, M, T)
    assert lib.t2v_bn_act_slices(1, B, M, T, training, 0) == sl
    if (B, M, T) == (1, 1, 131073):
        idx = [0, chunk - 1, chunk, (sl - 1) * chunk - 1, (sl - 1) * chunk, n - 1]
    else:
        idx = _boundaries(n, T, chunk)
    g = np.random.default_rng(n + M)
    one, zero = np.ones(M, dtype=F32), np.zeros(M, dtype=F32)
    launches = 0
    for use, dout in _single_one_runs(B, M, T, idx):
        launches += 1
        for binary in (False, True):
            yc = (g.integers(0, 2, size=(M, n)) if binary else g.integers(-3, 4, size=(M, n))).astype(F32)
            if binary:
                yc[np.arange(M), use] = 1
            y = np.ascontiguousarray(R.unchan(yc, B, T))
            got, same = run_bwd(lib, B, M, T, y, dout, zero, one, one, zero, R.ACT_NONE, training, 0.0, 1)
            assert same
            assert np.array_equal(got['dbeta'], one), (use, got['dbeta'])
            assert np.array_equal(got['dgamma'], yc[np.arange(M), use]), (use, got['dgamma'])
            assert np.array_equal(got['dbias'], one if not training else zero)
            if binary:
                ref = R.backward(y, dout, zero, one, one, zero, R.ACT_NONE, not training).dy
                other = R.chan(dout) == 0
                err = np.abs(R.chan(got['dy']) - R.chan(ref))
                assert (err <= np.spacing(np.abs(R.chan(ref)).astype(F32)))[other].all(), use
                if sl > 1 and training:         # two slices, spelled out: the first and the last hold the same -(1 + y) / n
                    dyc = R.chan(got['dy'])
                    for m in range(M):
                        for lo in (0, (sl - 1) * chunk):
                            j = lo + 1 if lo + 1 != use[m] else lo + 2
                            assert dyc[m, j] == -(1 + yc[m, j]) * (F32(1) / F32(n)), (m, j)
    print('bn-exact backward      %-13s %dx%dx%d %s: %d boundary indices in %d launches, dbeta == 1, dgamma == y[i], dy within 1 ulp '
          'in all %d slices' % (path, B, M, T, 'train' if training else 'eval', len(idx), launches, sl))


# ------------------------------------------------------------------------------------------------ argument checks

def test_arguments_that_are_refused_launch_nothing():
    lib = _lib()
    M = 2
    g, b, rm, rv = torch.ones(M, device='cuda'), torch.zeros(M, device='cuda'), torch.zeros(M, device='cuda'), torch.ones(M, device='cuda')
    y, out, mean, rstd = torch.ones(1, M, 1, device='cuda'), _nan(1, M, 1), _nan(M), _nan(M)

    def fwd(B, T, training, mean, rstd):
        return lib.t2v_bn_act_fwd(_p(y), None, 0, _p(g), _p(b), _p(rm), _p(rv), _p(mean), _p(rstd), _p(out), B, M, T, 0, training, 0.0, 0.1,
                                  1e-5, 0, 0, 0, _stream())
    assert fwd(1, 1, 1, mean, rstd) != 0                        # training with B*T < 2
    y2, out2 = torch.ones(2, M, 1, device='cuda'), _nan(2, M, 1)
    assert lib.t2v_bn_act_fwd(_p(y2), None, 0, _p(g), _p(b), _p(rm), _p(rv), None, _p(rstd), _p(out2), 2, M, 1, 0, 1, 0.0, 0.1, 1e-5, 0, 0, 0,
                              _stream()) != 0                  # training without mean_out
    assert lib.t2v_bn_act_fwd(_p(y2), None, 0, _p(g), _p(b), _p(rm), _p(rv), _p(mean), None, _p(out2), 2, M, 1, 0, 1, 0.0, 0.1, 1e-5, 0, 0, 0,
                              _stream()) != 0                  # ... without rstd_out
    lens = torch.zeros(4, dtype=torch.int32, device='cuda')
    assert lib.t2v_bn_act_fwd_len(_p(y), _p(g), _p(b), _p(rm), _p(rv), _p(out), _p(lens), 65536, M, 1, 0, 1e-5, _stream()) != 0
    torch.cuda.synchronize()
    for t in (out, out2, mean, rstd):                           # nothing ran: every output still holds its NaN
        assert torch.isnan(t).all()
    assert torch.equal(rm, torch.zeros(M, device='cuda')) and torch.equal(rv, torch.ones(M, device='cuda'))
    assert fwd(1, 1, 0, None, None) == 0                        # eval needs neither
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
