"""Every route of csrc/gemm.hip through the C ABI, element by element against the fp64 oracle of tests/gemm_ref.py.

Each case of gemm_ref.CASES first asserts the kernel t2v_gemm_route reports for the very pointers and strides it passes, then runs
t2v_gemm_f32 / _splitk / t2v_gemm_bf16 / _splitk twice and checks: the two runs are the same bits; the columns next to a column block
are untouched; every element is within 2e-7 * max(4, sqrt(K)) of the oracle relative to its sum of absolute terms; every ReLU / keep
decision is the oracle's outside the excused zone, which holds at most 0.1 % of the elements.  tests/test_gemm_ref.py shows on the CPU
that these checks pass for honest fp32 arithmetic and fail for every mutation; (b) below repeats the mutations against the DEVICE
results of one case per route.  The 128x128 bf16 kernel's own split-K needs T2V_BF16_GEMM_PLANES=0, read once per process: those
cases run in one child process.  Then the batched and grouped entry points and t2v_gemm_epilogue_bwd.

One line per case is printed before it is asserted (profiles/gemm_routes_parity.txt is that output of an MI355X run); no bound here
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

import gemm_ref as G                                                      # noqa: E402

pytestmark = pytest.mark.gpu


def _p(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run_case(lib, c):
    """(route answer for the pointers passed, the whole output matrix after the call on the CPU, second run identical?)"""
    inp = G.inputs(c)
    A = G.place(inp.A, c.a, c.a_pad, c.a_off, 'cuda')
    B = G.place(inp.B, c.b, c.b_pad, c.b_off, 'cuda')
    bias = inp.bias.cuda() if inp.bias is not None else None
    sAi, sAk, sBj, sBk = G.strides(c)
    assert A.stride() == (sAi, sAk) and B.stride() == (sBj, sBk)
    prev = lib.t2v_gemm_f32_set_mode(c.x3)
    try:
        scr, scr_off = None, 0
        if c.scratch:
            n = (lib.t2v_gemm_bf16_splitk_scratch_floats if c.bf16 else lib.t2v_gemm_splitk_scratch_floats)(c.M, c.N, c.K)
            assert n > 0, c.name
            scr_off = 4 if c.scratch == 2 else 0
            scr = torch.empty(n + 4, device='cuda')
            assert scr.data_ptr() % 16 == 0
        # the route for exactly what is passed
        form, splits, kps = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        r = lib.t2v_gemm_route(c.M, c.N, c.K, sAi, sAk, sBj, sBk, A.data_ptr() % 16, B.data_ptr() % 16,
                               (scr.data_ptr() + scr_off) % 16 if scr is not None else 0, int(scr is not None), c.relu, float(c.p), c.bf16,
                               C.byref(form), C.byref(splits), C.byref(kps))
        route = (lib.t2v_gemm_route_name(r).decode(), form.value, splits.value, kps.value)
        assert route == G.ask_route(lib, c), (c.name, route)
        fn = getattr(lib, 't2v_gemm_%s%s' % ('bf16' if c.bf16 else 'f32', '_splitk' if c.scratch else ''))
        outs = []
        for _ in range(2):
            Cm = inp.C0.cuda()
            args = [_p(A), sAi, sAk, _p(B), sBj, sBk, _p(bias), _p(Cm, 4 * inp.c0), inp.ldc, c.M, c.N, c.K, c.relu, c.acc, float(c.p),
                    G.SEED, G.STREAM, G.RNG_T]
            if c.scratch:
                args.append(_p(scr, scr_off))
            assert fn(*(args + [_stream()])) == 0, c.name
            outs.append(Cm)
        torch.cuda.synchronize()
    finally:
        lib.t2v_gemm_f32_set_mode(prev)
    return route, outs[0].cpu(), bool(torch.equal(outs[0], outs[1]))


def _run_all(env=None):
    import t2v_hip
    lib = t2v_hip.load_library()
    return dict((c.name, _run_case(lib, c)) for c in G.CASES if c.env == env)


@pytest.fixture(scope='module')
def results(tmp_path_factory):
    """case name -> (route, output, reproducible) of every case: this process's, and one child process per process-wide switch"""
    out = _run_all()
    for env in sorted(set(c.env for c in G.CASES if c.env)):
        assert os.environ.get(env[0]) is None, env
        path = str(tmp_path_factory.mktemp('gemm_routes') / 'child.pt')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path, env[0], env[1]], env=dict(os.environ, **dict([env])),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out.update(torch.load(path, weights_only=False))
    return out


_ORC = {}


def _oracle(name):
    """inputs and fp64 oracle, once per case"""
    if name not in _ORC:
        c = G.BY_NAME[name]
        inp = G.inputs(c)
        _ORC[name] = (inp, G.oracle(c, inp))
    return _ORC[name]


@pytest.mark.parametrize('name', [c.name for c in G.CASES])
def test_route_and_parity(results, name):
    c = G.BY_NAME[name]
    (route, form, splits, kps), full, same = results[name]
    assert route == c.route and (c.splits is None or splits == c.splits), (route, splits)
    inp, orc = _oracle(name)
    v = G.judge(c, full[:, inp.c0:inp.c0 + c.N], orc)
    print('gemm-route ' + G.table_line(c, route, form, splits, v))
    assert same, 'two runs differ'
    outside = torch.ones(inp.ldc, dtype=torch.bool)
    outside[inp.c0:inp.c0 + c.N] = False
    assert torch.equal(full[:, outside].view(torch.int32), inp.C0[:, outside].view(torch.int32)), 'columns next to the block were written'
    assert v.worst < v.bound, v
    assert v.wrong_decisions == 0 and v.excused <= G.CAP * v.elements, v


def test_every_route_was_run_and_asserted(results):
    assert set(r[0][0] for r in results.values()) == set(G.ROUTES)
    assert all(results[c.name][0][0] == c.route for c in G.CASES)


def _mutation_cases():
    """per route the case the most mutations apply to, and the fp32 split-K case with the empty trailing split"""
    pick = {}
    for c in G.CASES:
        n = len(G.applicable(c, c.splits or (2 if c.route.endswith('splitk') else 1)))
        if c.route not in pick or n > pick[c.route][0]:
            pick[c.route] = (n, c.name)
    names = [pick[r][1] for r in G.ROUTES]
    return names + [n for n in ('f32_64_splitk_kk_65x33x1100_allblock',) if n not in names]


@pytest.mark.parametrize('name', _mutation_cases())
def test_device_results_fail_every_mutated_oracle(results, name):
    """(b) the device result, which passed against the oracle, against each mutated oracle that applies: must fail"""
    c = G.BY_NAME[name]
    (route, form, splits, kps), full, _ = results[name]
    inp, orc = _oracle(name)
    block = full[:, inp.c0:inp.c0 + c.N]
    assert G.judge(c, block, orc).ok
    muts = G.applicable(c, splits)
    assert len(muts) >= 3
    for m in muts:
        for z in (range(splits) if m == 'split_dropped' else (0,)):
            v = G.judge(c, block, G.oracle(c, inp, m, splits, kps, z))
            print('gemm-mutation %-46s %-24s%s %9.1f bounds' % (name, m, ' z=%d' % z if m == 'split_dropped' else '', v.worst / v.bound))
            if m == 'split_dropped' and z * kps >= c.K:
                assert v.ok, (m, z, v)                      # the empty trailing split: nothing is lost with it
            else:
                assert not v.ok and v.worst >= G.MUTATION_FACTOR * v.bound, (m, z, v)
    if name == 'f32_64_splitk_kk_65x33x1100_allblock':
        assert splits == 8 and 7 * kps >= c.K > 6 * kps


# ---------------------------------------------------------------- batched

def _batched(lib, nbatch, M, N, K, layout):
    """t2v_gemm_f32_batched on operands laid out as `layout` says -> (list of per-item inputs, output (nbatch, M, N) on the CPU)"""
    g = torch.Generator().manual_seed(7 * nbatch + M + 3 * N + 11 * K)
    As, Bs = G.heavy(g, nbatch, M, K), G.heavy(g, nbatch, N, K)
    if layout == 'reverse_pass':        # AL (T, B, T_in), DCTX (T, B, E): item b is A_b = AL[:, b, :]^T, B_b = DCTX[:, b, :]^T
        Ad, Bd = As.permute(2, 0, 1).contiguous().cuda(), Bs.permute(2, 0, 1).contiguous().cuda()
        sa, sb = (M, 1, nbatch * M), (N, 1, nbatch * N)
    else:                               # items one after the other, k-contiguous rows 3 floats apart
        Ad, Bd = torch.full((nbatch, M, K + 3), G.GARBAGE, device='cuda'), torch.full((nbatch, N, K + 3), G.GARBAGE, device='cuda')
        Ad[:, :, :K], Bd[:, :, :K] = As.cuda(), Bs.cuda()
        sa, sb = (M * (K + 3), K + 3, 1), (N * (K + 3), K + 3, 1)
    ldc = N + 5
    Cd = torch.full((nbatch, M, ldc), G.SENTINEL, device='cuda')
    assert lib.t2v_gemm_f32_batched(_p(Ad), sa[0], sa[1], sa[2], _p(Bd), sb[0], sb[1], sb[2], _p(Cd), M * ldc, ldc, nbatch, M, N, K, _stream()) == 0
    torch.cuda.synchronize()
    return As, Bs, Cd.cpu()


@pytest.mark.parametrize('nbatch,M,N,K,layout', [(3, 37, 70, 5, 'reverse_pass'), (1, 37, 70, 5, 'reverse_pass'), (3, 40, 65, 1, 'rows'),
                                                 (1, 129, 31, 97, 'rows'), (3, 65, 33, 33, 'rows')])
def test_batched(nbatch, M, N, K, layout):
    import t2v_hip
    lib = t2v_hip.load_library()
    As, Bs, out = _batched(lib, nbatch, M, N, K, layout)
    As2, Bs2, out2 = _batched(lib, nbatch, M, N, K, layout)
    assert torch.equal(out, out2)
    c = G.Case(name='batched', M=M, N=N, K=K, bias=0, route='f32_64')
    assert torch.equal(out[:, :, N:], torch.full((nbatch, M, 5), G.SENTINEL))
    for z in range(nbatch):
        inp = G.Inputs(As[z], Bs[z], None, torch.full((M, N + 5), G.SENTINEL), 0, N + 5)
        v = G.judge(c, out[z, :, :N], G.oracle(c, inp))
        print('gemm-route ' + G.table_line(c._replace(name='batched_%s_%dx%dx%dx%d[%d]' % (layout, nbatch, M, N, K, z)), 'f32_64 (batched)',
                                           1 if layout == 'rows' else 0, 1, v))
        assert v.worst < v.bound, (z, v)
        for m in ('last_k', 'last_row', 'last_col'):
            assert not G.judge(c, out[z, :, :N], G.oracle(c, inp, m)).ok, (z, m)
        if nbatch > 1:                  # the neighbour's operands must not do either
            other = G.Inputs(As[(z + 1) % nbatch], Bs[z], None, inp.C0, 0, N + 5)
            assert not G.judge(c, out[z, :, :N], G.oracle(c, other)).ok, z


# ---------------------------------------------------------------- grouped

def _grouped(lib, bf16, M, K, parts, accumulate):
    """the grouped product of `parts` (a list of column-width lists, one per group; operands stored (K, rows), as the weight gradients'
    are) and the same products issued singly -> per part: (case, inputs, grouped result, single result, route of the single call)"""
    import t2v_hip
    g = torch.Generator().manual_seed(M + K + sum(sum(p) for p in parts) + bf16)
    GG = t2v_hip._GemmGroup * len(parts)
    gr = GG()
    keep, items = [], []
    for gi, widths in enumerate(parts):
        A = G.heavy(g, M, K)
        Ad = G.place(A, 'r', 0, 0, 'cuda')
        total = sum(widths) + 7
        old = G.heavy(g, M, total)
        Cg, Cs = old.cuda(), old.cuda()              # one row-major matrix per group: the parts are its column blocks
        gr[gi].A, gr[gi].sAi, gr[gi].sAk, gr[gi].nb = Ad.data_ptr(), 1, M, len(widths)
        col = 3
        for pi, N in enumerate(widths):
            B = G.heavy(g, N, K)
            Bd = G.place(B, 'k' if pi % 2 else 'r', 0, 0, 'cuda')
            gr[gi].B[pi], gr[gi].sBj[pi], gr[gi].sBk[pi], gr[gi].N[pi] = Bd.data_ptr(), Bd.stride(0), Bd.stride(1), N
            gr[gi].C[pi], gr[gi].ldc[pi] = Cg.data_ptr() + 4 * col, total
            items.append((gi, col, N, A, B, Ad, Bd, old, Cg, Cs, total))
            col += N
        keep.append((Ad, Cg, Cs))
    tag = 'bf16' if bf16 else 'f32'
    n = getattr(lib, 't2v_gemm_%s_grouped_scratch_floats' % tag)(gr, len(parts), M, K)
    scr = torch.empty(max(n, 4), device='cuda')
    assert getattr(lib, 't2v_gemm_%s_grouped' % tag)(gr, len(parts), M, K, accumulate, _p(scr), _stream()) == 0
    out = []
    for (gi, col, N, A, B, Ad, Bd, old, Cg, Cs, total) in items:
        c = G.Case(name='grouped_%s_g%d_%dx%dx%d' % (tag, gi, M, N, K), bf16=bf16, M=M, N=N, K=K, a='r', b='r' if Bd.stride(0) == 1 else 'k',
                   a_pad=0, b_pad=0, bias=0, acc=accumulate, pad=total - N, scratch=1)
        ns = getattr(lib, 't2v_gemm_%ssplitk_scratch_floats' % ('bf16_' if bf16 else ''))(M, N, K)
        sscr = torch.empty(ns, device='cuda') if ns else None
        route = G.ask_route(lib, c, scratch=sscr is not None)
        args = [_p(Ad), 1, M, _p(Bd), Bd.stride(0), Bd.stride(1), None, _p(Cs, 4 * col), total, M, N, K, 0, accumulate, 0.0, 0, 0, 0]
        fn = getattr(lib, 't2v_gemm_%s%s' % (tag, '_splitk' if sscr is not None else ''))
        assert fn(*(args + ([_p(sscr)] if sscr is not None else []) + [_stream()])) == 0
        C0 = torch.full((M, total), G.SENTINEL)
        if accumulate:
            C0[:, col:col + N] = old[:, col:col + N]
        out.append((c, G.Inputs(A, B, None, C0, col, total), Cg, Cs, col, old, route))
    torch.cuda.synchronize()
    return [(c, inp, Cg.cpu(), Cs.cpu(), col, old, route) for (c, inp, Cg, Cs, col, old, route) in out]


@pytest.mark.parametrize('bf16', (0, 1), ids=('f32', 'bf16'))
@pytest.mark.parametrize('M,parts,plane_form', [(1024, ([1024, 1024], [1024]), True), (1024, ([256, 384], [384]), True),
                                                (1024, ([256, 384], [256]), False), (256, ([128, 256], [128]), False)],
                         ids=('planes', 'planes_64_tiles', 'fallback_56_tiles', 'fallback'))
@pytest.mark.parametrize('accumulate', (0, 1), ids=('write', 'accumulate'))
def test_grouped(bf16, M, parts, plane_form, accumulate):
    """two groups, every part a whole number of 128-column tiles: from 64 tiles on (8 x (2 + 3 + 3)) one launch on the operand planes,
    below that (8 x (2 + 3 + 2)) the products one by one.  Each part against the oracle, and the same bits as the product issued
    singly wherever the single call takes the same route (a part of under 64 tiles on its own goes to a 64x64 kernel)"""
    import t2v_hip
    lib = t2v_hip.load_library()
    K = 72
    gr = (t2v_hip._GemmGroup * 2)()
    for gi, widths in enumerate(parts):
        gr[gi].nb = len(widths)
        for pi, N in enumerate(widths):
            gr[gi].N[pi] = N
    assert (lib.t2v_gemm_f32_grouped_group_offset(gr, 2, M, K, 1) >= 0) == plane_form      # (the same rule decides for one plane)
    want = ('bf16_planes' if bf16 else 'f32_x3') if plane_form else ('bf16_64' if bf16 else 'f32_64')
    got = _grouped(lib, bf16, M, K, parts, accumulate)
    if M == 1024 and len(parts[0]) == 2 and parts[0][0] == 1024:
        assert all(r[6][0] == want for r in got)              # every part is 64 tiles on its own: the single calls take the plane route too
    if not plane_form:
        assert all(r[6][0] == want for r in got)
    for (c, inp, Cg, Cs, col, old, route) in got:
        v = G.judge(c, Cg[:, col:col + c.N], G.oracle(c, inp, route=want))
        print('gemm-route ' + G.table_line(c, want + ' (grouped)', route[1], 1, v))
        assert v.worst < v.bound, v
        if route[0] == want:
            assert route[2] == 1, route
            assert torch.equal(Cg[:, col:col + c.N], Cs[:, col:col + c.N]), 'grouped and single products differ'
        else:
            vs = G.judge(c, Cs[:, col:col + c.N], G.oracle(c, inp, route=route[0]))
            assert vs.worst < vs.bound, (route, vs)
        for m in G.applicable(c, 1, want):
            assert not G.judge(c, Cg[:, col:col + c.N], G.oracle(c, inp, m, route=want)).ok, m
        # nothing outside the parts' columns moved
        edge = torch.ones(Cg.shape[1], dtype=torch.bool)
        edge[3:Cg.shape[1] - 4] = False
        assert torch.equal(Cg[:, edge], old[:, edge])


def test_grouped_handed_skips_the_tiles_already_done():
    """t2v_gemm_f32_grouped_handed behind a kernel that left group 1's planes in the scratch and took its first tiles: no tile of
    the first min(*done_ctr, done_cap) of that group is written, every other element has the grouped launch's bits"""
    import t2v_hip
    lib = t2v_hip.load_library()
    M, K, parts = 1024, 72, ([256, 384], [384])
    g = torch.Generator().manual_seed(99)
    gr = (t2v_hip._GemmGroup * 2)()
    keep, outs = [], []
    for gi, widths in enumerate(parts):
        Ad = G.place(G.heavy(g, M, K), 'r', 0, 0, 'cuda')
        Cm = torch.full((M, sum(widths)), G.SENTINEL, device='cuda')
        gr[gi].A, gr[gi].sAi, gr[gi].sAk, gr[gi].nb = Ad.data_ptr(), 1, M, len(widths)
        col = 0
        for pi, N in enumerate(widths):
            Bd = G.place(G.heavy(g, N, K), 'r', 0, 0, 'cuda')
            gr[gi].B[pi], gr[gi].sBj[pi], gr[gi].sBk[pi], gr[gi].N[pi] = Bd.data_ptr(), 1, N, N
            gr[gi].C[pi], gr[gi].ldc[pi] = Cm.data_ptr() + 4 * col, sum(widths)
            keep.append(Bd)
            col += N
        keep.append(Ad)
        outs.append(Cm)
    scr = torch.empty(lib.t2v_gemm_f32_grouped_scratch_floats(gr, 2, M, K), device='cuda')
    assert lib.t2v_gemm_f32_grouped_group_offset(gr, 2, M, K, 1) > 0
    assert lib.t2v_gemm_f32_grouped(gr, 2, M, K, 0, _p(scr), _stream()) == 0          # leaves the planes of both groups in scr
    torch.cuda.synchronize()
    whole = [o.cpu() for o in outs]
    assert not (whole[0] == G.SENTINEL).any() and not (whole[1] == G.SENTINEL).any()
    for done, cap, skipped in ((5, 100, 5), (5, 3, 3), (0, 100, 0), (100, 100, 24)):        # group 1: 8 x 3 tiles
        for o in outs:
            o.fill_(G.SENTINEL)
        ctr = torch.tensor([done], dtype=torch.int32, device='cuda')
        assert lib.t2v_gemm_f32_grouped_handed(gr, 2, M, K, 0, _p(scr), 1, _p(ctr), cap, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[0].cpu(), whole[0])
        got = outs[1].cpu()
        for t in range(24):
            by, bx = t // 3, t % 3
            tile, ref = got[128 * by:128 * by + 128, 128 * bx:128 * bx + 128], whole[1][128 * by:128 * by + 128, 128 * bx:128 * bx + 128]
            assert bool((tile == G.SENTINEL).all()) if t < skipped else torch.equal(tile, ref), (done, cap, t)


# ---------------------------------------------------------------- backward of the relu / dropout epilogue

@pytest.mark.parametrize('n', (1, 3, 4, 5, 1023, 1025))
@pytest.mark.parametrize('scale', (1.0, 2.0))
def test_epilogue_bwd_is_exact(n, scale):
    """out = dy * scale where y != 0, else +0: the float4 body and the tail kernel, +0 / -0 / denormal / negative y"""
    import t2v_hip
    lib = t2v_hip.load_library()
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -3.5, 1.0, 0.0, -0.0])
    y = torch.where(torch.rand(n, generator=g) < 0.5, torch.zeros(n), G.heavy(g, n))
    y[torch.arange(n) % 3 == 0] = special[(torch.arange(n) // 3) % len(special)][torch.arange(n) % 3 == 0]
    y[n - 1] = special[n % len(special)]
    dy = G.heavy(g, n)
    dy[n // 2] = 1e-41
    pad = 8                                 # SENTINEL behind the n elements: the tail must stop at n
    yd, dyd = y.cuda(), dy.cuda()
    out = torch.full((n + pad,), G.SENTINEL, device='cuda')
    assert lib.t2v_gemm_epilogue_bwd(_p(dyd), _p(yd), _p(out), n, scale, _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    want = torch.where(y != 0, dy * scale, torch.zeros(n))
    assert torch.equal(got[:n].view(torch.int32), want.view(torch.int32)), (got[:n] - want).abs().max()
    assert torch.equal(got[n:], torch.full((pad,), G.SENTINEL))
    if n > 4:
        assert lib.t2v_gemm_epilogue_bwd(_p(dyd, 4), _p(yd), _p(out), n - 1, scale, _stream()) != 0       # 16-byte alignment is required


if __name__ == '__main__':
    torch.save(_run_all((sys.argv[2], sys.argv[3])), sys.argv[1])
