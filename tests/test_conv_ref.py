"""tests/conv_ref.py can tell a right Conv1d kernel from a subtly wrong one — on the CPU, no kernel launch.

The fp64 oracle equals torch's fp64 conv1d and its autograd; the case table's hand-written routes equal the restated cost model (and,
where the answer needs no device, t2v_conv1d_route itself); honest fp32 arithmetic passes every check of every case, bit for bit
on the exact ones; and in every kernel family each mutation of the oracle that applies misses a bound by at least
gemm_ref.MUTATION_FACTOR on some case, or is named as invisible there with the reason."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p_ in (os.path.join(ROOT, 'tacotron2-vae_amd'), os.path.join(ROOT, 'tests')):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import conv_ref as R                                                     # noqa: E402

SMALL = 160e6           # multiply-adds: the cases the CPU emulation and the mutations run on (every family has some)
_CACHE = {}


def _honest(c):
    if c.name not in _CACHE:
        inp = R.inputs(c)
        _CACHE[c.name] = (inp, R.oracle(c, inp), R.emulate(c, inp))
    return _CACHE[c.name]


def test_oracle_equals_torch_fp64_conv1d_and_its_autograd():
    for name in ('generic_fwd_f32_2x33to70x129_k3', 'generic_fwd_f32_3x20to65x43_k5', 'width32_fwd_f32_2x64to80x83_k5', 'width32_fwd_f32_1x16to64x1_k5'):
        c = R.BY_NAME[name]
        inp = R.inputs(c)
        x, w, b, dy = (t.double() for t in inp)
        x.requires_grad_(True)
        w.requires_grad_(True)
        y = F.conv1d(x, w, b, padding=c.KS // 2)
        dx, dw = torch.autograd.grad(y, (x, w), dy)
        for op, ref in (('fwd', y.detach()), ('dx', dx), ('dw', dw)):
            o = R.oracle(c._replace(op=op, family='gemm' if op != 'dw' or c.family == 'gemm' else 'dw', tile=80 if op == 'dw' else c.tile), inp)
            assert (o['out'] - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), (name, op)
            assert bool((o['scale'] >= o['out'].abs() * (1 - 1e-12)).all())
    # the partial rows add up to the channel's sums, and each row is the sum over exactly its block
    c = R.BY_NAME['generic_fwd_f32_3x20to65x43_k5']
    inp = R.inputs(c)
    o = R.oracle(c, inp)
    y = o['out']
    assert o['part'].shape == (3, 65, 2)
    yc = y.transpose(0, 1).reshape(65, 129)
    assert (o['part'][1, :, 0] - yc[:, 64:128].sum(1)).abs().max().item() < 1e-12
    assert (o['part'][2, :, 1] - (yc[:, 128:] ** 2).sum(1)).abs().max().item() < 1e-12
    c = R.BY_NAME['width32_fwd_f32_2x64to80x83_k5']
    o = R.oracle(c, R.inputs(c))
    assert o['part'].shape == (6, 80, 2)
    assert (o['part'][5, :, 0] - o['out'][1, :, 64:83].sum(1)).abs().max().item() < 1e-12


def test_table_routes_equal_the_restated_cost_model():
    for c in R.CASES:
        m = R.model_route(c)
        assert m is not None and not R.mismatch(c, m), (c.name, R.mismatch(c, m))
    for shape, planes in R.MODE2_BOUNDARY:
        B, Cin, Cout, T = shape
        c = R.Case(name='b', B=B, Cin=Cin, Cout=Cout, T=T, x3=2)
        assert (R.model_route(c)['family'] == 'x3') == planes, shape
        assert (B * ((T + 127) // 128) * ((Cout + 127) // 128) >= 192) == planes


def test_table_routes_equal_the_library_where_no_device_is_needed():
    """x3 modes 0 and 2 below 192 tiles never ask for the plane kernels' scratch, so conv_route() answers without a GPU"""
    import t2v_hip
    lib = t2v_hip.load_library()
    if os.environ.get('T2V_CONV_STAGING', '1') == '0':
        pytest.skip('T2V_CONV_STAGING=0 is set for this process')
    n = 0
    for c in R.CASES:
        if c.x3 == 1 or not c.staging:
            continue
        prev = lib.t2v_conv1d_x3_set_mode(c.x3)
        try:
            got = R.ask_route(lib, c)
        finally:
            lib.t2v_conv1d_x3_set_mode(prev)
        assert isinstance(got, dict) and not R.mismatch(c, got), (c.name, got)
        if c.op == 'dw':
            assert got['dw_scratch_floats'] == (c.dw_splits * c.Cout * c.Cin * 5 if c.dw_splits > 1 else 0)
        n += 1
    assert n > 100
    # the bf16 entries decline what the tiled kernels cannot take, and bad arguments are refused
    for c in R.CASES:
        if c.family == 'gemm':
            assert R.ask_route(lib, c._replace(bf16=1)) == -1, c.name           # T2V_ERR_DIMS
    assert lib.t2v_conv1d_route(3, 1, 16, 1, 16, 5, 0, 0, *([None] * 8)) == -2 and lib.t2v_conv1d_route(0, 1, 16, 1, 16, 4, 0, 0, *([None] * 8)) == -2       # T2V_ERR_ARG
    assert lib.t2v_conv1d_route_name(99).decode() == '?'


def test_the_table_covers_what_it_promises():
    fam = lambda f, op: [c for c in R.CASES if c.family == f and c.op == op]          # noqa: E731
    for f in ('gemm', 'fwd', 'fwd_dma', 'x3', 'bf16', 'bf16k32', 'plane1'):
        assert fam(f, 'fwd') and fam(f, 'dx'), f
        assert any(c.exact for c in fam(f, 'fwd')) and any(c.exact for c in fam(f, 'dx')), f
    for f in ('fwd', 'fwd_dma', 'bf16', 'bf16k32'):
        assert set(c.tile for c in fam(f, 'fwd')) >= {2, 3, 4, 5, 6}, f
    for f in ('fwd', 'fwd_dma'):
        assert set(c.tile for c in fam(f, 'fwd') if c.ksplit == 2) == {2, 3, 4, 5, 6}, f
    for f in ('dw', 'dw_bf16'):
        cs = fam(f, 'dw')
        assert set(c.tile for c in cs) == {80, 96} and set(c.dw_splits for c in cs) == {1, 2, 4, 8}, f
        # splits that do not divide the k-tiles: 5 over 4 leaves one layer empty, 9 over 8 three
        empty = set()
        for c in cs:
            nkt = c.B * ((c.T + c.tile - 1) // c.tile)
            per = (nkt + c.dw_splits - 1) // c.dw_splits
            empty.add(sum(1 for z in range(c.dw_splits) if z * per >= nkt))
        assert empty >= {0, 1, 3}, (f, empty)
    assert any(c.w_off and c.op == 'fwd' and c.tile == 2 for c in R.CASES) and any(c.w_off and c.op == 'fwd' and c.tile == 5 for c in R.CASES)
    assert any(c.w_off and c.op == 'dx' for c in R.CASES)
    assert set(c.psplits for c in R.CASES if c.family == 'x3') >= {1, 2, 4} and set(c.psplits for c in R.CASES if c.family == 'plane1') >= {1, 2}


@pytest.mark.parametrize('name', [c.name for c in R.CASES if R.macs(c) <= SMALL])
def test_honest_fp32_passes(name):
    c = R.BY_NAME[name]
    inp, orc, (out, part) = _honest(c)
    v = R.judge(c, out, part, orc)
    assert v.ok, (name, v)


def _families():
    return sorted(set((c.family, c.op) for c in R.CASES))


@pytest.mark.parametrize('family,op', _families())
def test_every_mutation_is_caught_or_named_invisible(family, op):
    cases = [c for c in R.CASES if c.family == family and c.op == op and R.macs(c) <= SMALL]
    assert cases, (family, op)
    for m in R.MUTATIONS:
        cs = [c for c in cases if m in R.applicable(c)]
        if not cs:
            assert m in R.INVISIBLE and R.INVISIBLE[m], (family, op, m)
            continue
        best = 0.0
        for c in cs:
            inp, orc, (out, part) = _honest(c)
            v = R.judge(c, out, part, R.oracle(c, inp, mutation=m))
            best = max(best, R.worst(v) if not c.exact else (float('inf') if not v.exact_ok else 0.0))
            if best >= R.MUTATION_FACTOR:
                break
        assert best >= R.MUTATION_FACTOR, (family, op, m, best)


@pytest.mark.parametrize('name', R.mutation_cases())
def test_the_cases_the_gpu_test_mutates_see_every_applicable_mutation(name):
    c = R.BY_NAME[name]
    inp, orc, (out, part) = _honest(c)
    muts = R.applicable(c)
    assert len(muts) >= 3, muts
    for m in muts:
        v = R.judge(c, out, part, R.oracle(c, inp, mutation=m))
        assert not v.ok and R.worst(v) >= R.MUTATION_FACTOR, (name, m, v)
