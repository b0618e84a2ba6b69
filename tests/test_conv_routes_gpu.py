"""Every Conv1d route, tile width and split of csrc/conv_gemm.hip and csrc/conv_x3.hip through the C ABI, element by element and
partial row by partial row against the fp64 oracle of tests/conv_ref.py.

Each case of conv_ref.CASES first asserts what t2v_conv1d_route answers for the very call it makes (family, tile, channel cut,
weight-gradient splits, partial blocks, plane splits) against the table's hand-written expectation, then runs t2v_conv1d_fwd /
_bwd / _fwd_bf16 / _bwd_bf16 (t2v_conv1d_flip_weights in front where the case passes W == NULL) twice and checks: the two runs
are the same bits; every operand sits in a buffer that holds NaN around it, so a value read from outside an operand and used
poisons the result; every output (Y, stat_part, dX, dW, dw_scratch) sits in a NaN-prefilled buffer, every element inside is
written and every guard element outside still holds its bits; every element and every partial row is within its bound of the
oracle; the small-integer cases are the oracle's bits.  tests/test_conv_ref.py shows on the CPU that these checks pass honest fp32
arithmetic and fail every mutation; the last test repeats the mutations against the DEVICE results of one case per family.
T2V_CONV_STAGING=0 is read once per process: the register-staged cases run in ONE child process, and their results must be the
staged kernel's bits.

One line per case is printed before it is asserted (profiles/conv_routes_parity.txt is that output of an MI355X run); no bound here
is taken from it."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p_ in (os.path.join(ROOT, 'tacotron2-vae_amd'), os.path.join(ROOT, 'tests')):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import conv_ref as R                                                     # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                     # floats of NaN on either side of every operand and output (a multiple of four: 16-byte alignment stays)
NAN = float('nan')


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Buf:
    """`n` floats `off` floats behind a 16-byte boundary, inside an allocation that holds NaN before and behind them"""

    def __init__(self, n, off=0, data=None):
        self.n, self.at = n, GUARD + off
        self.store = torch.full((n + 2 * GUARD + off,), NAN, device='cuda')
        assert self.store.data_ptr() % 16 == 0
        if data is not None:
            self.store[self.at:self.at + n] = data.reshape(-1).cuda()

    def ptr(self):
        return C.c_void_p(self.store.data_ptr() + 4 * self.at)

    def inside(self):
        return self.store[self.at:self.at + self.n]

    def guards_untouched(self):
        g = torch.cat([self.store[:self.at], self.store[self.at + self.n:]]).view(torch.int32)
        return bool((g == torch.tensor(NAN).view(torch.int32).item()).all())

    def all_written(self):
        return not bool(torch.isnan(self.inside()).any())


def _run_case(lib, c):
    """the route for exactly what is passed, and the call twice -> dict(route, out, part, same, guards, written, staged)"""
    inp = R.inputs(c)
    B, Cin, Cout, T, KS = c.B, c.Cin, c.Cout, c.T, c.KS
    nw = Cout * Cin * KS
    prev = lib.t2v_conv1d_x3_set_mode(c.x3)
    try:
        X, dY = _Buf(B * Cin * T, data=inp.X), _Buf(B * Cout * T, data=inp.dY)
        W = _Buf(nw, off=c.w_off if c.op == 'fwd' else 0, data=inp.W)
        bias = _Buf(Cout, data=inp.bias)
        wt = _Buf(nw, off=c.w_off if c.op == 'dx' else 0)          # Wt_scratch of the fp32 data gradient
        wp = torch.empty(nw + 8, dtype=torch.int16, device='cuda')  # Wp_scratch of the bf16 entries
        route = R.ask_route(lib, c, w_mod16=(W.ptr().value if c.op == 'fwd' else wt.ptr().value) % 16)
        assert isinstance(route, dict), (c.name, route)
        n0 = lib.t2v_conv1d_staged_launches()
        runs = []
        for _ in range(2):
            bufs = {}
            if c.op == 'fwd':
                y, part = _Buf(B * Cout * T), _Buf(route['stat_blocks'] * Cout * 2)
                bufs.update(out=y, part=part)
                if c.bf16:
                    rc = lib.t2v_conv1d_fwd_bf16(W.ptr(), X.ptr(), bias.ptr(), y.ptr(), part.ptr(), C.c_void_p(wp.data_ptr()), B, Cin, T, Cout, KS, _stream())
                else:
                    rc = lib.t2v_conv1d_fwd(W.ptr(), X.ptr(), bias.ptr(), y.ptr(), part.ptr(), B, Cin, T, Cout, KS, _stream())
            elif c.op == 'dx':
                dx = _Buf(B * Cin * T)
                bufs.update(out=dx)
                if c.bf16:
                    rc = lib.t2v_conv1d_bwd_bf16(W.ptr(), X.ptr(), dY.ptr(), dx.ptr(), None, C.c_void_p(wp.data_ptr()), None, B, Cin, T, Cout, KS, _stream())
                else:
                    wt.store.fill_(NAN)
                    if c.preflip:
                        PA, IA = C.c_void_p * 1, C.c_int * 1
                        assert lib.t2v_conv1d_flip_weights(PA(W.ptr().value), PA(wt.ptr().value), IA(Cout), IA(Cin), KS, 1, _stream()) == 0
                    rc = lib.t2v_conv1d_bwd(None if c.preflip else W.ptr(), X.ptr(), dY.ptr(), dx.ptr(), None, wt.ptr(), None, B, Cin, T, Cout, KS, _stream())
                    bufs.update(wt=wt)
            else:
                dw = _Buf(nw)
                bufs.update(out=dw)
                scr = _Buf(route['dw_scratch_floats']) if route['dw_scratch_floats'] else None
                if scr is not None:
                    bufs.update(scr=scr)
                fn = lib.t2v_conv1d_bwd_bf16 if c.bf16 else lib.t2v_conv1d_bwd
                rc = fn(None, X.ptr(), dY.ptr(), None, dw.ptr(), None, scr.ptr() if scr is not None else None, B, Cin, T, Cout, KS, _stream())
            assert rc == 0, (c.name, rc)
            torch.cuda.synchronize()
            runs.append(bufs)
        staged = lib.t2v_conv1d_staged_launches() - n0
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)
    a, b = runs
    same = all(torch.equal(a[k].inside().view(torch.int32), b[k].inside().view(torch.int32)) for k in a if k not in ('scr', 'wt'))
    shape = {'fwd': (B, Cout, T), 'dx': (B, Cin, T), 'dw': (Cout, Cin, KS)}[c.op]
    return dict(route=route, out=a['out'].inside().cpu().reshape(shape),
                part=a['part'].inside().cpu().reshape(route['stat_blocks'], Cout, 2) if 'part' in a else None,
                same=same, staged=staged,
                guards=dict((k, v.guards_untouched()) for k, v in a.items()),
                written=dict((k, v.all_written()) for k, v in a.items()),
                inputs_intact=all(t.guards_untouched() for t in (X, W, bias, dY)))


def _run_all(staging):
    import t2v_hip
    lib = t2v_hip.load_library()
    prev = lib.t2v_gemm_f32_set_mode(1)             # (the three-plane kernels run only while the fp32 GEMM mode is 1)
    try:
        return dict((c.name, _run_case(lib, c)) for c in R.CASES if c.staging == staging)
    finally:
        lib.t2v_gemm_f32_set_mode(prev)


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    """case name -> result: the staged process's, and the register-staged cases' from one child process"""
    assert os.environ.get('T2V_CONV_STAGING', '1') != '0', 'this process must run the staged kernel'
    out = _run_all(1)
    path = str(tmp_path_factory.mktemp('conv_routes') / 'child.pt')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, T2V_CONV_STAGING='0'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out.update(torch.load(path, weights_only=False))
    return out


_ORC = {}


def _oracle(name):
    """inputs and fp64 oracle, once per case"""
    if name not in _ORC:
        c = R.BY_NAME[name]
        inp = R.inputs(c)
        _ORC[name] = (inp, R.oracle(c, inp))
    return _ORC[name]


@pytest.mark.parametrize('name', [c.name for c in R.CASES])
def test_route_and_parity(results, name):
    c = R.BY_NAME[name]
    res = results[name]
    route = res['route']
    assert not R.mismatch(c, route), (name, R.mismatch(c, route))
    inp, orc = _oracle(name)
    v = R.judge(c, res['out'], res['part'], orc)
    print('conv-route ' + R.table_line(c, route, v))
    assert res['same'], 'two runs differ'
    assert res['inputs_intact'], 'an operand buffer was written'
    assert all(res['guards'].values()), ('written outside an output', res['guards'])
    assert all(res['written'].values()), ('elements of an output left unwritten', res['written'])
    assert res['staged'] == (2 if route['family'] == 'fwd_dma' else 0), (route['family'], res['staged'])
    if c.op == 'dw':
        assert route['dw_scratch_floats'] == (c.dw_splits * c.Cout * c.Cin * 5 if c.dw_splits > 1 else 0)
    assert v.main < 1 and v.sums < 1 and v.squares < 1, v
    assert v.exact_ok, 'an exact case differs from the oracle in some bit'


def test_every_family_width_cut_and_split_was_run_and_asserted(results):
    ran = [(R.BY_NAME[n], r['route']) for n, r in results.items()]
    assert len(ran) == len(R.CASES)
    for f in ('gemm', 'fwd', 'fwd_dma', 'x3', 'bf16', 'bf16k32', 'plane1'):
        assert set(c.op for c, r in ran if r['family'] == f) >= {'fwd', 'dx'}, f
    for f in ('fwd', 'fwd_dma', 'bf16', 'bf16k32'):
        assert set(r['tile'] for c, r in ran if r['family'] == f and c.op == 'fwd') >= {2, 3, 4, 5, 6}, f
    for f in ('fwd', 'fwd_dma'):
        assert set(r['tile'] for c, r in ran if r['family'] == f and r['ksplit'] == 2) >= {2, 3, 4, 5, 6}, f
    for f in ('dw', 'dw_bf16'):
        assert set((r['tile']) for c, r in ran if r['family'] == f) == {80, 96}
        assert set((r['dw_splits']) for c, r in ran if r['family'] == f) == {1, 2, 4, 8}


def test_register_staged_kernel_gives_the_staged_kernels_bits(results):
    """k_conv5_fwd against k_conv5_fwd_dma at every width, cut and uncut, forward and data gradient (64 and 96 among them)"""
    seen = set()
    for c in R.CASES:
        if c.staging:
            continue
        twin = c.name.replace('_f32reg_', '_f32_' if not (c.op == 'dx') else '_f32_preflip_')
        a, b = results[c.name], results[twin]
        assert a['route']['family'] == 'fwd' and b['route']['family'] == 'fwd_dma', (c.name, twin)
        assert torch.equal(a['out'].view(torch.int32), b['out'].view(torch.int32)), c.name
        if a['part'] is not None:
            assert torch.equal(a['part'].view(torch.int32), b['part'].view(torch.int32)), c.name
        seen.add((a['route']['tile'], a['route']['ksplit']))
    assert seen >= set((t, k) for t in (2, 3, 4, 5, 6) for k in (1, 2)), seen


def test_mode2_takes_the_planes_from_192_tiles_on():
    """route only: nothing is launched"""
    import t2v_hip
    lib = t2v_hip.load_library()
    prev, prevg = lib.t2v_conv1d_x3_set_mode(2), lib.t2v_gemm_f32_set_mode(1)
    try:
        for shape, planes in R.MODE2_BOUNDARY:
            B, Cin, Cout, T = shape
            for bf16, fam in ((0, 'x3'), (1, 'plane1')):
                got = R.ask_route(lib, R.Case(name='b', B=B, Cin=Cin, Cout=Cout, T=T, bf16=bf16))
                assert (got['family'] == fam) == planes, (shape, bf16, got)
                assert lib.t2v_conv1d_takes_x3(B, Cin, T, Cout, 5, bf16) == int(planes)
                assert got['stat_blocks'] == (lib.t2v_conv1d_stat_blocks_bf16 if bf16 else lib.t2v_conv1d_stat_blocks)(B, T, Cin, Cout, 5)
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)
        lib.t2v_gemm_f32_set_mode(prevg)


def test_bf16_entries_decline_the_generic_shapes():
    import t2v_hip
    lib = t2v_hip.load_library()
    for c in R.CASES:
        if c.family != 'gemm' or c.exact:
            continue
        inp = R.inputs(c)
        X, W, bias, dY = (t.cuda() for t in inp)
        y, dx, dw = torch.full_like(dY, NAN), torch.full_like(X, NAN), torch.full_like(W, NAN)
        wp = torch.empty(W.numel() + 8, dtype=torch.int16, device='cuda')
        p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
        dims = (c.B, c.Cin, c.T, c.Cout, c.KS, _stream())
        assert lib.t2v_conv1d_fwd_bf16(p(W), p(X), p(bias), p(y), None, p(wp), *dims) == -1, c.name           # T2V_ERR_DIMS
        assert lib.t2v_conv1d_bwd_bf16(p(W), p(X), p(dY), p(dx), p(dw), p(wp), None, *dims) == -1, c.name
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and torch.isnan(dx).all() and torch.isnan(dw).all(), c.name
        assert R.ask_route(lib, c._replace(bf16=1)) == -1


@pytest.mark.parametrize('name', R.mutation_cases())
def test_device_results_fail_every_mutated_oracle(results, name):
    """the device result, which passed against the oracle, against each mutated oracle that applies: must fail"""
    c = R.BY_NAME[name]
    res = results[name]
    inp, orc = _oracle(name)
    assert R.judge(c, res['out'], res['part'], orc).ok
    muts = R.applicable(c)
    assert len(muts) >= 3
    for m in muts:
        v = R.judge(c, res['out'], res['part'], R.oracle(c, inp, mutation=m))
        print('conv-mutation %-52s %-20s %12.1f bounds' % (name, m, R.worst(v)))
        assert not v.ok and R.worst(v) >= R.MUTATION_FACTOR, (m, v)


if __name__ == '__main__':
    torch.save(_run_all(0), sys.argv[1])
