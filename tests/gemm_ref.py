"""fp64 oracle of the dense products of csrc/gemm.hip, their case table and its mutations — TEST INFRASTRUCTURE, NOT PRODUCT.

    C[i][j] = drop(relu(sum_k A(i,k) B(j,k) + bias[j] (+ C_old[i][j])))        A(i,k) = A[i*sAi + k*sAk], B(j,k) = B[j*sBj + k*sBk]

The epilogue order is the kernels' (gemm64_epilogue, k_gemm_f32_big, gx_tile): bias, then `accumulate`, then ReLU, then the dropout
factor drawn at idx = i*ldc + j (tests/drop_ref.py).  The bf16 routes round both operands to bf16 (RNE, tests/bf16_ref.py) and
accumulate exact products in fp32, so against the product of the ROUNDED operands they owe the fp32-accumulation bound and nothing
more.  One route is the exception by construction: bf16_to_f32_big is a bf16 call that the fp32 large-tile kernel takes — it rounds
nothing, and its oracle is the product of the operands as given.

Every element is held to     |out - ref| / scale < 2e-7 * max(4, sqrt(K)),     scale = sum_k |a||b| + |bias| (+ |C_old|),
(times the dropout factor 1 / (1 - p) where there is one: it multiplies the sum, so it multiplies every term of it),
the bound tests/test_gemm_gpu.py::test_x3_gemm_is_fp32_class and tests/test_conv5_staging_gpu.py use.  Where ReLU or dropout decide
between a value and zero the decision must be the oracle's, except where |pre-activation| / scale is itself under the bound (either
side of zero is then a correct fp32 answer); a case may have at most 0.1 % of such elements (CAP: a condition on the case table that
tests/test_gemm_ref.py checks, not a measurement).

CASES is the table tests/test_gemm_routes_gpu.py runs through the C ABI and tests/test_gemm_ref.py proves, on the CPU, to be able to
tell a right kernel from a subtly wrong one: honest fp32 results (emulate) pass, every applicable entry of MUTATIONS misses the
bound by at least MUTATION_FACTOR.  The mutations alter the ORACLE, never a kernel.
"""
import collections
import math

import numpy as np
import torch

import bf16_ref
import drop_ref

SENTINEL = 12345.0                # what an output element holds before a call that does not accumulate, and the columns next to a block
GARBAGE = 777.0                   # what the gaps of a strided operand hold: finite, and wrong if a kernel reads it
CAP = 1e-3                        # share of a case's elements whose ReLU / keep decision may be excused
MUTATION_FACTOR = 8.0
SEED, STREAM, RNG_T = 0x5DEECE66D, 5, 3          # of the dropout legs

ROUTES = ('f32_64', 'f32_64_splitk', 'f32_big_128', 'f32_big_64', 'f32_x3', 'bf16_64', 'bf16_64_splitk', 'bf16_big',
          'bf16_big_splitk', 'bf16_planes', 'bf16_to_f32_big')            # T2V_GEMM_ROUTE_* of include/t2vae.h, in order
K_TILE = {'f32_x3': 16}           # k per staged tile of a route (32 everywhere else)

MUTATIONS = ('last_k', 'k_tail', 'last_row', 'last_col', 'bias_per_split', 'relu_before_accumulate', 'drop_index_n', 'bias_by_row',
             'bf16_truncated', 'split_dropped')


def bound(K):
    return 2e-7 * max(4.0, math.sqrt(K))


_FIELDS = dict(name=None, bf16=0, M=0, N=0, K=0,
               a='k', b='k',            # operand layout: k = contiguous along k, r = along the rows, s = neither (stride 3 / 3 K + 1)
               a_pad=3, b_pad=3,        # floats between consecutive rows (k) / k-rows (r) beyond the dense stride
               a_off=0, b_off=0,        # floats between the (256-byte aligned) allocation and the operand's base
               bias=1, acc=0, relu=0, p=0.0,
               pad=0,                   # > 0: the output is a column block of a row-major matrix N + pad wide (ldc > N), 3 columns in
               scratch=0,               # 0: the entry point without scratch; 1: scratch of the size the library asks for; 2: ... 4 bytes off
               x3=1,                    # t2v_gemm_f32_set_mode for the call
               route=None, splits=None,  # what t2v_gemm_route must answer (splits None: whatever it answers, > 1 on a split-K route)
               env=None,                # a process-wide switch read once: the case runs in a child process
               seed=0)
Case = collections.namedtuple('Case', list(_FIELDS))
Case.__new__.__defaults__ = tuple(_FIELDS.values())

# epilogue legs: bias, accumulate, relu, p_drop, pad
LEGS = (('nobias', dict(bias=0)), ('bias', dict()), ('acc', dict(acc=1)), ('relu', dict(relu=1)), ('drop', dict(p=0.5)),
        ('all', dict(acc=1, relu=1, p=0.5)), ('block', dict(acc=1, pad=7)))
LEG_ALL_BLOCK = ('allblock', dict(acc=1, relu=1, p=0.5, pad=7))          # the C ABI draws the mask at i*ldc + j whatever ldc is
FORMS = ('kk', 'kr', 'rk', 'rr')
SMALL = ((1, 129, 1), (31, 65, 31), (64, 64, 32), (65, 31, 33), (129, 1, 97))    # every M, N of {1, 31, 64, 65, 129} and K of {1, 31, 32, 33, 97}


def _cases():
    out = []

    def add(name, **kw):
        out.append(Case(name=name, seed=len(out) + 1, **kw))

    for bf16, tag, route in ((0, 'f32_64', 'f32_64'), (1, 'bf16_64', 'bf16_64')):
        for f in FORMS:
            for (M, N, K) in SMALL:
                add('%s_%s_%dx%dx%d' % (tag, f, M, N, K), bf16=bf16, M=M, N=N, K=K, a=f[0], b=f[1], route=route)
        add('%s_strided_65x33x33' % tag, bf16=bf16, M=65, N=33, K=33, a='s', b='s', a_off=1, b_off=1, route=route)
        for i, (leg, kw) in enumerate(LEGS + (LEG_ALL_BLOCK,)):
            f = FORMS[i % 4]
            add('%s_%s_65x33x33_%s' % (tag, f, leg), bf16=bf16, M=65, N=33, K=33, a=f[0], b=f[1], route=route, **kw)
    # split-K of the 64x64 kernels.  fp32: gridDim.z stays the number asked for — (65, 33, 1100) is 8 splits of 160 k, the last empty;
    # bf16: the empty one is not launched
    for (M, N, K), ns32, ns16 in (((65, 33, 257), 2, 2), ((65, 33, 1100), 8, 7), ((129, 70, 515), 4, 4)):
        for i, (leg, kw) in enumerate(LEGS + (LEG_ALL_BLOCK,)):
            f = FORMS[(i + 1) % 4]
            add('f32_64_splitk_%s_%dx%dx%d_%s' % (f, M, N, K, leg), M=M, N=N, K=K, a=f[0], b=f[1], scratch=1, route='f32_64_splitk',
                splits=ns32, **kw)
        for i, (leg, kw) in enumerate((LEGS[1], LEGS[5], LEG_ALL_BLOCK)):
            f = FORMS[(i + 2) % 4]
            add('bf16_64_splitk_%s_%dx%dx%d_%s' % (f, M, N, K, leg), bf16=1, M=M, N=N, K=K, a=f[0], b=f[1], scratch=1,
                route='bf16_64_splitk', splits=ns16, **kw)
    # fp32 large tile (native mode): 1924 x 1028 = 16 x 17 tiles of 128 x 64, both edges ragged -> the 128-wide tile; N = 1020 -> the 64-wide
    for f in FORMS:
        for K in (4, 36, 68):
            add('f32_big_%s_1924x1028x%d' % (f, K), M=1924, N=1028, K=K, a=f[0], b=f[1], a_pad=0, b_pad=0, x3=0, route='f32_big_128')
        add('f32_big_%s_1924x1020x36' % f, M=1924, N=1020, K=36, a=f[0], b=f[1], a_pad=0, b_pad=0, x3=0, route='f32_big_64')
    for i, (leg, kw) in enumerate(LEGS + (LEG_ALL_BLOCK,)):
        add('f32_big_kr_1924x1028x36_%s' % leg, M=1924, N=1028, K=36, a='k', b='r', a_pad=0, b_pad=0, x3=0, route='f32_big_128', **kw)
    # neighbours that just miss gemm_big_ok: the 64x64 kernel must take them
    big = dict(M=1924, N=1028, a_pad=0, b_pad=0, x3=0, route='f32_64')
    add('f32_gate_kk_K37', K=37, a='k', b='k', **big)
    add('f32_gate_kr_a_base4', K=36, a='k', b='r', a_off=1, **big)
    add('f32_gate_rk_b_stride2', K=36, a='r', b='k', **dict(big, b_pad=2))
    add('f32_gate_rr_a_stride2', K=36, a='r', b='r', **dict(big, a_pad=2))
    add('f32_gate_rr_b_base4', K=36, a='r', b='r', b_off=1, **big)
    # x3 (default mode, with scratch): 9 x 8 tiles of 128 x 128
    for f in FORMS:
        add('f32_x3_%s_1028x1020x36' % f, M=1028, N=1020, K=36, a=f[0], b=f[1], scratch=1, route='f32_x3', splits=1)
    for i, (leg, kw) in enumerate((LEGS[0], LEGS[1], LEGS[5], LEGS[6], LEG_ALL_BLOCK)):
        f = FORMS[i % 4]
        add('f32_x3_%s_1028x1020x548_%s' % (f, leg), M=1028, N=1020, K=548, a=f[0], b=f[1], scratch=1, route='f32_x3', splits=2, **kw)
    # K = 1 and 3 mod 4: the split pass's float4 loads end before the k-tail
    add('f32_x3_kk_1028x1020x37', M=1028, N=1020, K=37, a_pad=3, b_pad=3, scratch=1, route='f32_x3', splits=1)
    add('f32_x3_scratch_off4_1028x1020x548', M=1028, N=1020, K=548, scratch=2, route='f32_64', splits=1)
    # bf16 large tile (no scratch): 9 x 8 tiles of 128 x 128; k-contiguous operands need K % 32 == 0 and rows a multiple of 4 apart
    for f in FORMS:
        for K in (32, 96):
            add('bf16_big_%s_1028x1024x%d' % (f, K), bf16=1, M=1028, N=1024, K=K, a=f[0], b=f[1], a_pad=0, b_pad=0, route='bf16_big')
    add('bf16_big_rr_1028x1024x96_acc_block', bf16=1, M=1028, N=1024, K=96, a='r', b='r', a_pad=0, b_pad=0, acc=1, pad=7, route='bf16_big')
    for K in (64, 548):
        for i, (leg, kw) in enumerate((LEGS[1], LEG_ALL_BLOCK)):
            f = FORMS[(i + (K > 64)) % 4]
            add('bf16_planes_%s_1028x1020x%d_%s' % (f, K, leg), bf16=1, M=1028, N=1020, K=K, a=f[0], b=f[1], scratch=1,
                route='bf16_planes', **kw)
    add('bf16_planes_kk_1028x1020x67', bf16=1, M=1028, N=1020, K=67, a_pad=1, b_pad=1, scratch=1, route='bf16_planes', splits=1)
    # ... and deep enough for the one-plane kernel's own k-split (34 stages of 32 k: two splits of 17), K no multiple of the stage
    add('bf16_planes_kr_1028x1020x1032_all', bf16=1, M=1028, N=1020, K=1032, b='r', scratch=1, route='bf16_planes', splits=2,
        acc=1, relu=1, p=0.5)
    # K = 36 along k: gemm_bf16_big_operand_ok declines, gemm_big_ok accepts
    add('bf16_to_f32_big_kk_1924x1028x36', bf16=1, M=1924, N=1028, K=36, a_pad=0, b_pad=0, route='bf16_to_f32_big')
    add('bf16_to_f32_big_kr_1924x1028x36_relu', bf16=1, M=1924, N=1028, K=36, b='r', a_pad=0, b_pad=0, relu=1, route='bf16_to_f32_big')
    # the 128x128 bf16 kernel's own split-K: only with the one-plane route switched off
    for f, kw in (('rr', dict()), ('kr', dict(acc=1, pad=7))):
        add('bf16_big_splitk_%s_1024x1024x1056' % f, bf16=1, M=1024, N=1024, K=1056, a=f[0], b=f[1], a_pad=0, b_pad=0, scratch=1,
            route='bf16_big_splitk', splits=2, env=('T2V_BF16_GEMM_PLANES', '0'), **kw)
    assert len(set(c.name for c in out)) == len(out)
    return tuple(out)


CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)


# ---------------------------------------------------------------- inputs and layouts

def heavy(g, *shape):
    """randn * 2^randint(-6, 7): magnitudes over 2^+-6, so that a dropped low-order term shows"""
    return torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())


def layout(form, rows, K, pad):
    """(stride between rows, stride between k) of an operand"""
    if form == 'k':
        return K + pad, 1
    if form == 'r':
        return 1, rows + pad
    return 3 * K + 1, 3


def strides(case):
    sAi, sAk = layout(case.a, case.M, case.K, case.a_pad)
    sBj, sBk = layout(case.b, case.N, case.K, case.b_pad)
    return sAi, sAk, sBj, sBk


def place(x, form, pad, off, device='cpu'):
    """the logical matrix x (rows, K) as a view with the layout's strides, `off` floats into storage that is GARBAGE elsewhere"""
    rows, K = x.shape
    s_row, s_k = layout(form, rows, K, pad)
    store = torch.full((off + (rows - 1) * s_row + (K - 1) * s_k + 1,), GARBAGE, device=device)
    view = torch.as_strided(store, (rows, K), (s_row, s_k), off)
    view.copy_(x)
    return view


Inputs = collections.namedtuple('Inputs', 'A B bias C0 c0 ldc')


def inputs(case):
    """logical fp32 operands, the bias, and the whole output matrix as it is before the call: (M, ldc), SENTINEL outside the column
    block [c0, c0 + N) and inside it too unless the call accumulates"""
    g = torch.Generator().manual_seed(1000 + case.seed)
    A, B = heavy(g, case.M, case.K), heavy(g, case.N, case.K)
    bias = heavy(g, case.N) if case.bias else None
    old = heavy(g, case.M, case.N)
    c0 = 3 if case.pad else 0
    ldc = case.N + case.pad
    C0 = torch.full((case.M, ldc), SENTINEL)
    if case.acc:
        C0[:, c0:c0 + case.N] = old
    return Inputs(A, B, bias, C0, c0, ldc)


def rounding(case, route=None):
    """what a route does to its operands before it multiplies"""
    route = route or case.route
    return bf16_ref.rne if (case.bf16 and route != 'bf16_to_f32_big') else bf16_ref.identity


def drop_factor(case, ldc):
    """fp32 dropout factors of the (M, N) block, drawn at i*ldc + j relative to the block's first element"""
    i = np.arange(case.M, dtype=np.int64)[:, None]
    j = np.arange(case.N, dtype=np.int64)[None, :]
    return torch.from_numpy(drop_ref.drop_scale(SEED, STREAM, RNG_T, (i * ldc + j).reshape(-1), case.p).reshape(case.M, case.N))


# ---------------------------------------------------------------- oracle

def applicable(case, splits, route=None):
    """the mutations that can change this case's result"""
    route = route or case.route
    kt = K_TILE.get(route, 32)
    m = ['last_k']
    if case.K > kt and case.K % kt:
        m.append('k_tail')
    if case.M > 1:
        m.append('last_row')
    if case.N > 1:
        m.append('last_col')
    if case.bias and splits > 1:
        m.append('bias_per_split')
    if case.relu and case.acc:
        m.append('relu_before_accumulate')
    if case.p > 0 and case.pad:
        m.append('drop_index_n')
    if case.bias and case.N > 1:
        m.append('bias_by_row')
    if case.bf16 and route != 'bf16_to_f32_big':
        m.append('bf16_truncated')
    if splits > 1:
        m.append('split_dropped')
    return m


def oracle(case, inp, mutation=None, splits=1, k_per_split=None, drop_split=0, route=None):
    """fp64 result of the block (M, N) with the kernels' epilogue order.  Returns dict(ref, scale, pre, pre_scale): the expected
    block, the sum of absolute terms every error is relative to (never mutated; a dropout leg's kept elements are 1 / (1 - p) times
    their sum, so their terms are too), the value ReLU sees and the sum of ITS absolute terms.  mutation: one of MUTATIONS;
    split_dropped leaves out the k range of split `drop_split`."""
    route = route or case.route
    M, N, K = case.M, case.N, case.K
    q = rounding(case, route)
    a, b = q(inp.A).double(), q(inp.B).double()
    bias = inp.bias.double() if inp.bias is not None else None
    old = inp.C0[:, inp.c0:inp.c0 + N].double()
    scale = a.abs() @ b.abs().t()
    if bias is not None:
        scale = scale + bias.abs()[None, :]
    if case.acc:
        scale = scale + old.abs()
    if mutation == 'bf16_truncated':
        a, b = bf16_ref.truncate(inp.A).double(), bf16_ref.truncate(inp.B).double()
    keep = torch.ones(K, dtype=torch.bool)
    if mutation == 'last_k':
        keep[K - 1] = False
    elif mutation == 'k_tail':
        kt = K_TILE.get(route, 32)
        keep[K // kt * kt:] = False
    elif mutation == 'split_dropped':
        keep[drop_split * k_per_split:(drop_split + 1) * k_per_split] = False
    pre = a[:, keep] @ b[:, keep].t()
    if bias is not None:
        if mutation == 'bias_by_row':
            pre = pre + bias[torch.arange(M) % N][:, None]
        else:
            pre = pre + bias[None, :] * (splits if mutation == 'bias_per_split' else 1)
    if mutation == 'relu_before_accumulate':
        v = pre.clamp(min=0) + old
        pre = v
    else:
        if case.acc:
            pre = pre + old
        v = pre.clamp(min=0) if case.relu else pre
    pre_scale = scale
    if case.p > 0:
        v = v * drop_factor(case, N if mutation == 'drop_index_n' else inp.ldc).double()
        scale = scale / (1.0 - case.p)         # the factor multiplies every term of the sum, exactly (a power of two at p = 0.5)
    ref = v.clone()
    if mutation == 'last_row':
        ref[M - 1] = inp.C0[M - 1, inp.c0:inp.c0 + N].double()
    elif mutation == 'last_col':
        ref[:, N - 1] = inp.C0[:, inp.c0 + N - 1].double()
    return dict(ref=ref, scale=scale, pre=pre, pre_scale=pre_scale)


Verdict = collections.namedtuple('Verdict', 'worst bound excused wrong_decisions elements ok')


def judge(case, out, orc):
    """a result block (M, N) against an oracle: the worst |out - ref| / scale, how many elements sit where the ReLU / keep decision
    is excused, how many decisions are wrong outside that zone, and whether the case passes"""
    bd = bound(case.K)
    out = out.double()
    err = (out - orc['ref']).abs() / orc['scale']
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    worst = err.max().item()
    excused = wrong = 0
    if case.relu or case.p > 0:
        zone = orc['pre'].abs() / orc['pre_scale'] < bd
        excused = int(zone.sum())
        wrong = int((((out != 0) != (orc['ref'] != 0)) & ~zone).sum())
    n = case.M * case.N
    return Verdict(worst, bd, excused, wrong, n, bool(worst < bd and wrong == 0 and excused <= CAP * n))


# ---------------------------------------------------------------- honest fp32 results (the CPU stand-ins of a right kernel)

def emulate(case, inp, how, splits=1, k_per_split=None, route=None):
    """fp32 results a correct kernel may give.  how = 'torch': one fp32 product; 'tiles': k in tiles of 32, each tile's fp32 product
    added to its split's partial sum, the partials added in split order — the order the split-K kernels keep.  The epilogue in fp32."""
    q = rounding(case, route)
    a, b = q(inp.A), q(inp.B)
    K = case.K
    if how == 'torch':
        acc = a @ b.t()
    else:
        kps = k_per_split or K
        acc = torch.zeros(case.M, case.N)
        for z in range(splits):
            part = torch.zeros(case.M, case.N)
            for k0 in range(z * kps, min(K, (z + 1) * kps), 32):
                k1 = min(K, k0 + 32, (z + 1) * kps)
                part = part + a[:, k0:k1] @ b[:, k0:k1].t()
            acc = acc + part
    v = acc + inp.bias[None, :] if inp.bias is not None else acc
    if case.acc:
        v = v + inp.C0[:, inp.c0:inp.c0 + case.N]
    if case.relu:
        v = v.clamp(min=0)
    if case.p > 0:
        v = v * drop_factor(case, inp.ldc)
    return v


# ---------------------------------------------------------------- the route query

def ask_route(lib, case, scratch=None):
    """t2v_gemm_route for a case as tests/test_gemm_routes_gpu.py lays it out (allocations 256-byte aligned, operands a_off / b_off
    floats in, scratch 4 bytes off when case.scratch == 2) -> (route name, form, splits, k per split)"""
    import ctypes as C
    sAi, sAk, sBj, sBk = strides(case)
    form, splits, kps = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    has = int(case.scratch != 0 if scratch is None else scratch)
    r = lib.t2v_gemm_route(case.M, case.N, case.K, sAi, sAk, sBj, sBk, 4 * case.a_off % 16, 4 * case.b_off % 16,
                           4 if case.scratch == 2 else 0, has, case.relu, float(case.p), case.bf16,
                           C.byref(form), C.byref(splits), C.byref(kps))
    assert 0 <= r < len(ROUTES), r
    assert lib.t2v_gemm_route_name(r).decode() == ROUTES[r]
    return ROUTES[r], form.value, splits.value, kps.value


def table_line(case, route, form, splits, v):
    return '%-46s %-15s form %s splits %d  err/scale %.2e  bound %.2e  excused %d/%d' % (
        case.name, route, 'rk'[form & 1] + 'rk'[form >> 1 & 1], splits, v.worst, v.bound, v.excused, v.elements)


def routes_in_child(cases, env):
    """ask_route for `cases` in one fresh process with `env` set: the switches the dispatch reads once per process.  No GPU needed."""
    import json
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [c.name for c in cases], env=dict(os.environ, **dict([env])),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict((k, tuple(v)) for k, v in json.loads(r.stdout.strip().split('\n')[-1]).items())


if __name__ == '__main__':
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tacotron2-vae_amd'))
    import t2v_hip
    _lib = t2v_hip.load_library()
    print(json.dumps(dict((n, ask_route(_lib, BY_NAME[n])) for n in sys.argv[1:])))
