"""fp64 oracle of the Conv1d kernels of csrc/conv_gemm.hip and csrc/conv_x3.hip, their case table, judge and mutations — TEST
INFRASTRUCTURE, NOT PRODUCT.

    forward          Y[b][m][t]   = sum_{c,k} W[m][c][k] X[b][c][t + k - P] + bias[m]                    K = KS Cin
    data gradient    dX[b][c][t]  = sum_{m,k} W[m][c][KS-1-k] dY[b][m][t + k - P]                        K = KS Cout
    weight gradient  dW[m][c][k]  = sum_{b,t} dY[b][m][t] X[b][c][t + k - P]                             K = B T
    BatchNorm partials  stat_part[r][m] = [sum, sum of squares] of conv + bias over the positions of block r

Every element of Y, dX, dW is held to |out - ref| / scale < gemm_ref.bound(K), scale = the sum of the absolute terms (the project's
fp32-class rule).  The bf16 families (k_conv5_fwd_bf16, _bf16k32, k_conv5_x3<1, 4>, k_conv5_dw_bf16) round BOTH operands to bf16
(RNE) and accumulate exact products in fp32: k_conv5_pack_bf16 rounds W (the data gradient's flip folded in), the forward kernels
round X (dY as a data gradient) while staging, k_conv5_dw_bf16 rounds dY and X while staging, the split passes of conv_x3.hip round
W and X once.  Against the convolution of the ROUNDED operands they owe the same bound.  k_conv5_x3<3, 2> cuts fp32 operands exactly
in three planes and rounds nothing.

Partial blocks, read from the kernels (a row holds one block's sums for every channel):
    tiled  (k_conv5_fwd, _dma, _bf16, _bf16k32)   row b * ceil(T / BN) + j : positions [j BN, (j + 1) BN) of item b, BN = 16 * tile
    gemm   (k_conv_gemm)                          row j : columns [64 j, 64 j + 64) of n = b T + t, across item boundaries
    plane  (k_conv5_x3)                           row b * ceil(T / 128) + j : positions [128 j, 128 j + 128) of item b
and their bounds, counted from the epilogues (u = 2^-24, first order; e_i = bound(K) scale_i is what an element may be off by):
    sum            sum e_i + d u sum|v_i|
    sum of squares sum (2 |v_i| e_i + e_i^2) + (d + 1) u sum v_i^2        (one more rounding: the product, or the fma that adds it)
    d = roundings a value goes through on its way into the row:
        tiled  a lane adds its `tile` columns serially (the first addition to 0 is exact: tile - 1), row16_sum is 4 levels: tile + 3
        gemm   row16_sum 4, the other half-wave 1, the two waves of a block row 1: 6
        plane  a lane adds its two columns (1), then one thread adds the 64 column slots serially (<= 64): 65
No constant here was fitted to a device result.

Exact cases: impulses in X / dY, small integers everywhere else, so that every product and every partial sum is an integer below
2^24 whatever the order (oracle() asserts it): the device must return the oracle's bits.

CASES carries for each case the route t2v_conv1d_route must answer, written by hand from the cost model of conv_gemm.hip
(conv5_pick_bn_ks, conv5_dw_bt, conv5_dw_splits, T2V_NWG = 256) and cx_splits of conv_x3.hip; model_route() restates that model
and tests/test_conv_ref.py holds the table to it on the CPU.  The mutations alter the ORACLE, never a kernel.
"""
import collections
import zlib

import torch
import torch.nn.functional as F

import bf16_ref
from gemm_ref import MUTATION_FACTOR, bound

U = 2.0 ** -24
NWG = 256                           # T2V_NWG
FAMILIES = ('gemm', 'fwd', 'fwd_dma', 'x3', 'bf16', 'bf16k32', 'plane1', 'dw', 'dw_bf16')     # T2V_CONV_ROUTE_* in order
OPS = ('fwd', 'dx', 'dw')                                                                      # T2V_CONV_OP_* in order
BF16_FAMILIES = ('bf16', 'bf16k32', 'plane1', 'dw_bf16')
PLANE_FAMILIES = ('x3', 'plane1')
MUTATIONS = ('taps_reversed', 'halo_left', 'halo_right', 'halo_neighbour', 'last_block_dropped', 'cut_half_dropped', 'bias_per_half',
             'dw_split_dropped', 'dw_split_twice', 'dw_tail_counted', 'dx_untransposed', 'stat_row_shift', 'sq_before_bias',
             'stat_pad_counted', 'bf16_truncated')

_FIELDS = dict(name=None, op='fwd', B=1, Cin=16, Cout=64, T=1, KS=5,
               bf16=0,              # the bf16_run entry points
               x3=0,                # t2v_conv1d_x3_set_mode for the call
               staging=1,           # 0: T2V_CONV_STAGING=0, read once per process: the case runs in the one child process
               w_off=0,             # floats between a 16-byte boundary and the weights the kernel reads (W, or Wt_scratch as a data gradient)
               preflip=0,           # data gradient with W == NULL after t2v_conv1d_flip_weights
               exact=0,             # small-integer operands: bit equality
               family=None, tile=0, ksplit=1, dw_splits=1, stat_blocks=0, psplits=0, pchunk=0)      # what t2v_conv1d_route must answer
Case = collections.namedtuple('Case', list(_FIELDS))
Case.__new__.__defaults__ = tuple(_FIELDS.values())


# ---------------------------------------------------------------- the cost model, restated (model_route)

def _cdiv(a, b):
    return (a + b - 1) // b


def pick_bn(T, B, M):
    best, best_cost = 80, -1
    for bn in (32, 48, 64, 80, 96):
        wgs = B * _cdiv(T, bn) * _cdiv(M, 64)
        cost = _cdiv(wgs, NWG) * (bn + 40)
        if best_cost < 0 or cost < best_cost or (cost == best_cost and bn > best):
            best, best_cost = bn, cost
    return best


def pick_bn_ks(T, B, M, Cin):
    bn1 = pick_bn(T, B, M)
    if Cin < 256:
        return bn1, 1
    w1 = B * _cdiv(T, bn1) * _cdiv(M, 64)
    best, best_cost, ks = bn1, 2 * _cdiv(w1, NWG) * (bn1 + 40), 1
    for bn in (32, 48, 64, 80, 96):
        wgs = 2 * B * _cdiv(T, bn) * _cdiv(M, 64)
        if wgs > NWG:
            continue
        cost = _cdiv(wgs, NWG) * (bn + 40 + 16)
        if cost < best_cost:
            best, best_cost, ks = bn, cost, 2
    return best, ks


def dw_bt(T):
    return 80 if _cdiv(T, 80) * 80 <= _cdiv(T, 96) * 96 else 96


def dw_splits(B, Cin, T, Cout, BT, bf16):
    wgs, nkt = (Cin // 16) * _cdiv(Cout, 64), B * _cdiv(T, BT)
    want = 8 * NWG if bf16 else NWG
    ns = 1
    while wgs * ns * 2 <= want and ns * 2 <= nkt and ns < 8:
        ns *= 2
    return ns


def cx_splits(tiles, nst):
    """(gridDim.z, stages per split) of t2v_conv5_x3_run"""
    best, best_w = 1, 1e30
    if tiles < 192:
        ns = 1
        while ns <= 8 and (ns == 1 or nst // ns >= 2):
            w = float(_cdiv(tiles * ns, 768)) * (1.0 / ns + 0.08 * 30.0 / nst) + 0.08 * (ns - 1)
            if w < best_w - 1e-9:
                best_w, best = w, ns
            ns += 1
    if best > 1:
        chunk = _cdiv(nst, best)
        nz = _cdiv(nst, chunk)
        if nz > 1:
            return nz, chunk
    return 1, nst


def run_dims(c):
    """(Cin, M) of the convolution as it runs: a data gradient is the convolution Cout -> Cin"""
    return (c.Cout, c.Cin) if c.op == 'dx' else (c.Cin, c.Cout)


def model_route(c):
    """what conv_route() answers for a case, by the restated model: dict of the route fields; None where the bf16 entry declines"""
    Cr, M = run_dims(c)
    r = dict(family='gemm', tile=0, ksplit=1, dw_splits=1, stat_blocks=0 if c.op == 'dw' else _cdiv(c.B * c.T, 64), psplits=0, pchunk=0)
    if c.KS != 5 or Cr % 16:
        return None if c.bf16 else r
    if c.op == 'dw':
        bt = dw_bt(c.T)
        return dict(r, family='dw_bf16' if c.bf16 else 'dw', tile=bt, dw_splits=dw_splits(c.B, c.Cin, c.T, c.Cout, bt, c.bf16))
    bn, ks = pick_bn_ks(c.T, c.B, M, Cr)
    r.update(tile=bn // 16, stat_blocks=c.B * _cdiv(c.T, bn))
    if c.bf16:
        r['family'] = 'bf16k32' if Cr % 32 == 0 else 'bf16'
    else:
        r.update(family='fwd_dma' if c.staging and not c.w_off else 'fwd', ksplit=ks)
    tiles = c.B * _cdiv(c.T, 128) * _cdiv(M, 128)
    if c.x3 and Cr >= 64 and M >= 64 and not (c.x3 == 2 and tiles < 192):
        ng = 4 if c.bf16 else 2
        nst = _cdiv(Cr, 8 * ng)
        nz, chunk = cx_splits(tiles, nst)
        r.update(family='plane1' if c.bf16 else 'x3', ksplit=1, stat_blocks=c.B * _cdiv(c.T, 128), psplits=nz, pchunk=chunk)
    return r


# ---------------------------------------------------------------- the case table

def _cases():
    out = []

    def add(tag, shape, twin=True, **kw):
        B, Cin, Cout, T = shape
        c = Case(name=None, B=B, Cin=Cin, Cout=Cout, T=T, **kw)
        name = '%s_%s_%s%s_%dx%dto%dx%d_k%d' % (tag, c.op, 'bf16' if c.bf16 else ('f32' if c.staging else 'f32reg'),
                                               ('_x3m%d' % c.x3 if c.x3 else '') + ('_woff' if c.w_off else '') + ('_preflip' if c.preflip else ''),
                                               B, Cin, Cout, T, c.KS)
        out.append(c._replace(name=name))
        if twin:
            out.append(c._replace(name=name + '_exact', exact=1))

    def tiled(tag, shape, op, tile, ks, precisions=('f32', 'f32reg', 'bf16'), **kw):
        B, Cin, Cout, T = shape
        Cr = Cout if op == 'dx' else Cin
        sb = B * _cdiv(T, 16 * tile)
        for p in precisions:
            if p == 'bf16':
                add(tag, shape, op=op, bf16=1, family='bf16k32' if Cr % 32 == 0 else 'bf16', tile=tile, stat_blocks=sb, **kw)
            else:
                add(tag, shape, op=op, staging=int(p == 'f32'), family='fwd_dma' if p == 'f32' else 'fwd', tile=tile, ksplit=ks,
                    stat_blocks=sb, preflip=int(op == 'dx' and p == 'f32'), **kw)

    # forward tile widths 32 .. 96 on the staged, the register-staged and the bf16 K32 kernel (Cin = 16: the K16 one) ...
    for shape, tile in (((1, 16, 64, 1), 2), ((1, 64, 64, 33), 2), ((2, 64, 80, 83), 2), ((7, 64, 512, 129), 3), ((7, 64, 512, 193), 4),
                        ((5, 64, 512, 400), 5), ((6, 64, 512, 401), 6)):
        tiled('width%d' % (16 * tile), shape, 'fwd', tile, 1)
    # ... and on the bf16 K16 kernel: Cin = 48 is three blocks of 16 and no multiple of 32
    for shape, tile in (((2, 48, 80, 83), 2), ((7, 48, 512, 129), 3), ((7, 48, 512, 193), 4), ((5, 48, 512, 400), 5), ((6, 48, 512, 401), 6)):
        tiled('k16width%d' % (16 * tile), shape, 'fwd', tile, 1, precisions=('bf16',))
    # the cut of the input channels in two (fp32 kernels only), at all five widths, and the data gradients of the same layers: the
    # convolution Cout -> Cin, cut where Cout >= 256
    for shape, tile, dx_tile, dx_ks in (((1, 256, 64, 37), 2, 2, 1), ((2, 272, 128, 84), 2, 2, 1), ((5, 256, 80, 400), 3, 3, 1),
                                        ((8, 256, 80, 400), 4, 4, 1), ((6, 256, 512, 129), 5, 2, 2), ((6, 272, 512, 161), 6, 3, 2)):
        tiled('cut', shape, 'fwd', tile, 2, precisions=('f32', 'f32reg'))
        tiled('cutdx', shape, 'dx', dx_tile, dx_ks, precisions=('f32', 'f32reg'))
    # the data gradient on the bf16 kernels (the flip folded into the pack pass): Cout = 80 -> K16, 512 -> K32
    tiled('dx', (2, 64, 80, 83), 'dx', 2, 1, precisions=('bf16',))
    tiled('dx', (7, 64, 512, 129), 'dx', 2, 2, precisions=('f32', 'bf16'))
    # default dispatch (x3 mode 2): under 192 plane tiles the tiled kernels keep the call
    tiled('default', (8, 512, 512, 400), 'fwd', 4, 1, precisions=('f32',), x3=2, twin=False)
    tiled('default', (3, 512, 512, 400), 'fwd', 5, 2, precisions=('f32',), x3=2, twin=False)
    # weights 4 bytes off a 16-byte boundary: k_conv5_fwd (W forward, Wt_scratch as a data gradient)
    for shape, tile, dx_tile, dx_ks in (((1, 64, 64, 33), 2, 2, 1), ((5, 64, 512, 400), 5, 2, 2)):
        add('unaligned', shape, op='fwd', w_off=1, family='fwd', tile=tile, stat_blocks=shape[0] * _cdiv(shape[3], 16 * tile))
        add('unaligned', shape, op='dx', w_off=1, family='fwd', tile=dx_tile, ksplit=dx_ks, stat_blocks=shape[0] * _cdiv(shape[3], 16 * dx_tile))
    # weight gradient: both k-tile depths, 1 / 2 / 4 / 8 splits, splits that do not divide the k-tiles (the last layers get nothing)
    for shape, bt, ns32, ns16 in (((1, 16, 64, 96), 96, 1, 1), ((1, 16, 64, 97), 80, 2, 2), ((5, 16, 64, 37), 80, 4, 4),
                                  ((9, 16, 64, 80), 80, 8, 8), ((2, 16, 64, 320), 80, 8, 8), ((3, 32, 80, 160), 80, 4, 4),
                                  ((3, 32, 80, 161), 96, 4, 4), ((6, 256, 512, 129), 80, 2, 8)):
        add('dw', shape, op='dw', family='dw', tile=bt, dw_splits=ns32)
        add('dw', shape, op='dw', bf16=1, family='dw_bf16', tile=bt, dw_splits=ns16)
    # the generic kernel: KS = 3, KS = 5 with Cin % 16 != 0, smaller than a tile in every dimension, 64-column blocks across items
    for shape, KS in (((2, 33, 70, 129), 3), ((2, 33, 70, 129), 5), ((1, 5, 3, 7), 3), ((3, 20, 65, 43), 5)):
        sb = _cdiv(shape[0] * shape[3], 64)
        for op in OPS:
            add('generic', shape, op=op, KS=KS, family='gemm', stat_blocks=0 if op == 'dw' else sb)
    # the plane kernels (x3 mode 1), three planes (fp32 entries) and one (bf16_run): channel splits even and uneven, M % 128 != 0,
    # the unsplit form at 192 tiles.  A stage is 16 channels on three planes, 32 on one
    P = 'plane'
    for shape, (z3, c3), (z1, c1) in (((1, 64, 64, 2), (2, 2), (1, 2)), ((2, 64, 64, 130), (2, 2), (1, 2)),
                                      ((2, 80, 64, 130), (2, 3), (1, 3)), ((2, 128, 200, 131), (4, 2), (2, 2))):
        sb = shape[0] * _cdiv(shape[3], 128)
        add(P, shape, op='fwd', x3=1, family='x3', tile=2, stat_blocks=sb, psplits=z3, pchunk=c3)
        add(P, shape, op='fwd', x3=1, bf16=1, family='plane1', tile=2, stat_blocks=sb, psplits=z1, pchunk=c1)
    add(P, (8, 64, 1024, 384), op='fwd', x3=1, family='x3', tile=6, stat_blocks=24, psplits=1, pchunk=4, twin=False)
    add(P, (8, 64, 1024, 384), op='fwd', x3=1, bf16=1, family='plane1', tile=6, stat_blocks=24, psplits=1, pchunk=2, twin=False)
    # data gradients on the planes: 64 -> 64, 64 -> 80 (one-plane: the library's flipped-weight ring), and 1024 -> 64 in 24 tiles: split
    add(P, (2, 64, 64, 130), op='dx', x3=1, family='x3', tile=2, stat_blocks=4, psplits=2, pchunk=2)
    add(P, (2, 64, 64, 130), op='dx', x3=1, bf16=1, family='plane1', tile=2, stat_blocks=4, psplits=1, pchunk=2)
    add(P, (2, 80, 64, 130), op='dx', x3=1, preflip=1, family='x3', tile=2, stat_blocks=4, psplits=2, pchunk=2)
    add(P, (2, 80, 64, 130), op='dx', x3=1, bf16=1, family='plane1', tile=2, stat_blocks=4, psplits=1, pchunk=2)
    add(P, (8, 64, 1024, 384), op='dx', x3=1, family='x3', tile=2, stat_blocks=24, psplits=4, pchunk=16, twin=False)
    add(P, (8, 64, 1024, 384), op='dx', x3=1, bf16=1, family='plane1', tile=2, stat_blocks=24, psplits=4, pchunk=8, twin=False)
    assert len(set(c.name for c in out)) == len(out)
    return tuple(out)


CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)
# x3 mode 2 takes the planes from 192 tiles of 128 x 128 on: (B, Cin, Cout, T) -> takes the planes?  Route only, nothing is launched
MODE2_BOUNDARY = (((191, 64, 64, 1), False), ((192, 64, 64, 1), True), ((3, 64, 8192, 1), True), ((3, 64, 8191, 1), True),
                  ((3, 64, 8064, 1), False))


def macs(c):
    return c.B * c.T * c.Cin * c.Cout * c.KS


def case_id(c):
    return c.name


# ---------------------------------------------------------------- geometry

def geometry(c):
    """('tiled' | 'gemm' | 'plane', positions per partial block)"""
    if c.family == 'gemm':
        return 'gemm', 64
    if c.family in PLANE_FAMILIES:
        return 'plane', 128
    return 'tiled', 16 * c.tile


def block_rows(c):
    """(B, T) int64: the stat_part row of every (b, t), and the number of rows"""
    kind, w = geometry(c)
    b = torch.arange(c.B)[:, None]
    t = torch.arange(c.T)[None, :]
    if kind == 'gemm':
        return (b * c.T + t) // 64, _cdiv(c.B * c.T, 64)
    per = _cdiv(c.T, w)
    return b * per + t // w, c.B * per


def row_depth(c):
    kind, _ = geometry(c)
    return {'tiled': c.tile + 3, 'gemm': 6, 'plane': 65}[kind]


def reduction_length(c):
    return {'fwd': c.KS * c.Cin, 'dx': c.KS * c.Cout, 'dw': c.B * c.T}[c.op]


def rounding(c, mutation=None):
    if c.family in BF16_FAMILIES:
        return bf16_ref.truncate if mutation == 'bf16_truncated' else bf16_ref.rne
    return bf16_ref.identity


# ---------------------------------------------------------------- inputs

Inputs = collections.namedtuple('Inputs', 'X W bias dY')


def _seed(c):
    return zlib.crc32(('%d,%d,%d,%d,%d,%d' % (c.B, c.Cin, c.Cout, c.T, c.KS, c.exact)).encode())


def _positions(c):
    """positions t that get an impulse: the ends of an item, both sides of every boundary of a forward tile of every width, of a
    128-position plane tile and of a weight-gradient k-tile of either depth"""
    T = c.T
    ps = {0, 1, T - 2, T - 1}
    for w in (32, 48, 64, 80, 96, 128):
        for e in range(w, T, w):
            ps.update((e - 1, e))
    return sorted(p for p in ps if 0 <= p < T)


def _channels(C):
    """the first and last channel of the first and last 16-channel block and of each half of a channel cut"""
    h = 16 * ((C // 16) // 2)
    cs = {0, 15, C - 16, C - 1, h - 1, h}
    return sorted(x for x in cs if 0 <= x < C)


def _rows(M):
    return sorted(x for x in {0, 63, 64, M - 1} if 0 <= x < M)


def _impulses(B, C, T, chans, pos, c):
    """(B, C, T) zeros with amplitudes 1 .. 3 at chans x pos of the first and last item, and at both sides of every 64-column
    boundary of n = b T + t (which lie inside items)"""
    x = torch.zeros(B, C, T)
    pts = set((b, t) for b in {0, B - 1} for t in pos)
    for n in range(64, B * T, 64):
        pts.add(((n - 1) // T, (n - 1) % T))
        pts.add((n // T, n % T))
    for (b, t) in pts:
        for ch in chans:
            x[b, ch, t] = 1 + (3 * b + 5 * ch + 7 * t) % 3
    return x


def inputs(c):
    """the fp32 operands of a case (X, W, bias, dY), the same for every op, precision and route of a shape"""
    g = torch.Generator().manual_seed(_seed(c))
    B, Cin, Cout, T, KS = c.B, c.Cin, c.Cout, c.T, c.KS
    if not c.exact:
        X = torch.randn(B, Cin, T, generator=g) * torch.exp2(torch.randint(-4, 5, (B, Cin, T), generator=g).float())
        W = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
        bias = torch.randn(Cout, generator=g) * 0.5
        dY = torch.randn(B, Cout, T, generator=g) * torch.exp2(torch.randint(-4, 5, (B, Cout, T), generator=g).float())
        return Inputs(X, W, bias, dY)
    m = torch.arange(Cout)[:, None, None]
    ch = torch.arange(Cin)[None, :, None]
    k = torch.arange(KS)[None, None, :]
    W = ((3 * m + 5 * ch + 2 * k) % 15 - 7).float()                    # the five taps of a (row, channel) are five different integers
    bias = ((torch.arange(Cout) * 5) % 9 - 4).float()
    pos = _positions(c)
    dY = _impulses(B, Cout, T, sorted(set(_rows(Cout)) | set(_channels(Cout))), pos, c)     # rows of dW, channels of the data gradient
    if c.op == 'dw':                                                    # the other operand of the weight gradient is dense
        b = torch.arange(B)[:, None, None]
        cc = torch.arange(Cin)[None, :, None]
        t = torch.arange(T)[None, None, :]
        X = ((2 * b + 3 * cc + 5 * t) % 13 - 6).float()
    else:
        X = _impulses(B, Cin, T, _channels(Cin), pos, c)
    return Inputs(X, W, bias, dY)


# ---------------------------------------------------------------- oracle

def flip_t(W):
    """(Cout, Cin, KS) -> (Cin, Cout, KS) with the taps reversed: the weights of the data-gradient convolution"""
    return W.transpose(0, 1).flip(2).contiguous()


def applicable(c):
    """the mutations that can change this case's result; see invisible() for the ones a case cannot see"""
    Cr, M = run_dims(c)
    kind, w = geometry(c)
    m = ['taps_reversed', 'halo_left', 'halo_right']
    if c.B > 1:
        m.append('halo_neighbour')
    if c.op != 'dw':
        if Cr > (16 if Cr % 16 == 0 else 1):
            m.append('last_block_dropped')
        if c.ksplit == 2:
            m.append('cut_half_dropped')
            if c.op == 'fwd':
                m.append('bias_per_half')
    else:
        if c.dw_splits > 1:
            m += ['dw_split_dropped', 'dw_split_twice']
        if c.family != 'gemm' and c.T % c.tile:
            m.append('dw_tail_counted')
    if c.op == 'dx':
        m.append('dx_untransposed')
    if c.op == 'fwd':
        m.append('sq_before_bias')
        if block_rows(c)[1] > 1:
            m.append('stat_row_shift')
        if (c.B * c.T if kind == 'gemm' else c.T) % w:
            m.append('stat_pad_counted')
    if c.family in BF16_FAMILIES and not c.exact:
        m.append('bf16_truncated')
    return m


INVISIBLE = {
    'halo_neighbour': 'B = 1: there is no neighbouring item',
    'last_block_dropped': 'a single channel block: dropping it leaves nothing to compare (the weight gradient has no channel loop)',
    'cut_half_dropped': 'only k_conv5_fwd[_dma] with ksplit = 2 cut the input channels',
    'bias_per_half': 'only a forward launch with ksplit = 2 has halves and a bias',
    'dw_split_dropped': 'dw_splits = 1, or not a weight gradient',
    'dw_split_twice': 'dw_splits = 1, or not a weight gradient',
    'dw_tail_counted': 'T is a multiple of the k-tile depth (no position beyond T in a k-tile), k_conv_gemm, or not a weight gradient',
    'dx_untransposed': 'not a data gradient',
    'stat_row_shift': 'one partial block, or no partials (data and weight gradients are handed none)',
    'sq_before_bias': 'no partials',
    'stat_pad_counted': 'the blocks end at T (at B T for k_conv_gemm), or no partials',
    'bf16_truncated': 'fp32 families round nothing; the exact cases hold integers that bf16 represents',
}


def _pad(x, P, mutation=None, extra=0):
    """(B, C, T) -> (B, C, P + T + P + extra): zero halo (the mutations put something else there)"""
    B, C, T = x.shape
    xp = x.new_zeros(B, C, T + 2 * P + extra)
    xp[:, :, P:P + T] = x
    if mutation == 'halo_left':
        xp[:, :, P - 1] = x[:, :, 0]
    elif mutation == 'halo_right':
        xp[:, :, P + T] = x[:, :, T - 1]
    elif mutation == 'halo_neighbour' and B > 1:
        n = min(P, T)
        xp[1:, :, P - n:P] = x[:-1, :, T - n:]
        xp[:-1, :, P + T:P + T + n] = x[1:, :, :n]
    return xp


def _flat_tail(x, Tend):
    """(B, C, Tend): x with the positions at and beyond T read on in memory (the next row; zero behind the tensor)"""
    B, C, T = x.shape
    flat = torch.cat([x.reshape(-1), x.new_zeros(Tend)])
    idx = (torch.arange(B * C)[:, None] * T + torch.arange(Tend)[None, :]).reshape(B, C, Tend)
    return flat[idx]


def oracle(c, inp, mutation=None):
    """fp64 results of a case on its expected route: dict(out, scale[, part, e_part]).  scale and e_part are never mutated."""
    P, KS, B, T = c.KS // 2, c.KS, c.B, c.T
    K = reduction_length(c)
    bd = bound(K)
    q, q0 = rounding(c, mutation), rounding(c)
    if c.op == 'dw':
        dy, x = q(inp.dY).double(), q(inp.X).double()
        xp = _pad(x, P, mutation)
        ady, axp = q0(inp.dY).double().abs(), _pad(q0(inp.X).double().abs(), P)
        wgt = torch.ones(B, 1, T, dtype=torch.float64)
        if mutation in ('dw_split_dropped', 'dw_split_twice'):
            tiles = _cdiv(T, c.tile)
            per = _cdiv(B * tiles, c.dw_splits)
            kt = torch.arange(B)[:, None, None] * tiles + torch.arange(T)[None, None, :] // c.tile
            wgt = torch.where(kt < per, torch.full_like(wgt, 0.0 if mutation == 'dw_split_dropped' else 2.0), wgt)
        out = torch.stack([torch.einsum('bmt,bct->mc', dy * wgt, xp[:, :, k:k + T]) for k in range(KS)], 2)
        scale = torch.stack([torch.einsum('bmt,bct->mc', ady, axp[:, :, k:k + T]) for k in range(KS)], 2)
        if mutation == 'dw_tail_counted':
            Tend = _cdiv(T, c.tile) * c.tile
            dye = _flat_tail(dy, Tend)
            dye[:, :, :T] = 0
            xe = _flat_tail(x, Tend + P)
            xe = torch.cat([x.new_zeros(B, x.shape[1], P), xe], 2)
            out = out + torch.stack([torch.einsum('bmt,bct->mc', dye, xe[:, :, k:k + Tend]) for k in range(KS)], 2)
        if mutation == 'taps_reversed':
            out = out.flip(2)
        res = dict(out=out, scale=scale)
    else:
        if c.op == 'fwd':
            x, w, w0, bias = q(inp.X).double(), q(inp.W).double(), q0(inp.W).double(), inp.bias.double()
            x0 = q0(inp.X).double()
        else:
            x, x0, bias = q(inp.dY).double(), q0(inp.dY).double(), None
            w0 = flip_t(q0(inp.W).double())
            w = q(inp.W).double().reshape(c.Cin, c.Cout, KS).clone() if mutation == 'dx_untransposed' else flip_t(q(inp.W).double())
        Cr = w.shape[1]
        if mutation == 'taps_reversed':
            w = w.flip(2)
        elif mutation == 'last_block_dropped':
            w = w.clone()
            w[:, Cr - (16 if Cr % 16 == 0 else 1):, :] = 0
        elif mutation == 'cut_half_dropped':
            w = w.clone()
            w[:, 16 * ((Cr // 16) // 2):, :] = 0
        kind, width = geometry(c)
        Text = _cdiv(T, width) * width if kind != 'gemm' else T
        xp = _pad(x, P, mutation, extra=Text - T)
        conv = F.conv1d(xp, w)                                   # (B, M, Text)
        scale = F.conv1d(_pad(x0.abs(), P), w0.abs())
        v = conv
        if bias is not None:
            v = conv + bias[None, :, None] * (2 if mutation == 'bias_per_half' else 1)
            scale = scale + bias.abs()[None, :, None]
        res = dict(out=v[:, :, :T].contiguous(), scale=scale)
        if c.op == 'fwd':
            rows, nblk = block_rows(c)
            M = w.shape[0]

            def sums(val):
                """(nblk, M) block sums of a (B, M, T) array"""
                o = torch.zeros(nblk, M, dtype=torch.float64)
                return o.index_add_(0, rows.reshape(-1), val.transpose(1, 2).reshape(B * T, M))

            vt = v[:, :, :T]
            sq = (conv[:, :, :T] if mutation == 'sq_before_bias' else vt) ** 2
            part = torch.stack([sums(vt), sums(sq)], 2)
            if mutation == 'stat_pad_counted':
                if kind == 'gemm':              # the columns behind B T of the last block: the kernel's zero operands plus the bias
                    npad = _cdiv(B * T, 64) * 64 - B * T
                    part[nblk - 1, :, 0] += npad * bias
                    part[nblk - 1, :, 1] += npad * bias * bias
                else:                           # positions [T, end of the tile) of every item: the convolution runs on into the zeros
                    last = rows[:, T - 1]
                    part[last, :, 0] += v[:, :, T:].sum(2)
                    part[last, :, 1] += (v[:, :, T:] ** 2).sum(2)
            if mutation == 'stat_row_shift':
                part = part.roll(1, 0)
            # bounds, from the unmutated values
            e = bd * scale
            if mutation is None:
                v0 = vt
            else:
                v0 = oracle(c, inp)['out']
            d = row_depth(c)
            e_s = sums(e) + d * U * sums(v0.abs())
            e_q = sums(2 * v0.abs() * e + e * e) + (d + 1) * U * sums(v0 * v0)
            res.update(part=part, e_part=torch.stack([e_s, e_q], 2))
    if c.exact and mutation is None:
        for t in inp:
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= 256
        assert float(res['scale'].max()) < 2 ** 24, 'a sum of absolute products reaches 2^24'
        if 'part' in res:
            assert float(res['part'].abs().max()) < 2 ** 24, "a block's sum of squares reaches 2^24"
    return res


def mutation_cases(limit=160e6):
    """per (family, op) the random case of at most `limit` multiply-adds that the most mutations apply to: the cases on which the
    GPU test repeats the mutations against the device's results (tests/test_conv_ref.py holds each of them to every one first)"""
    pick = {}
    for c in CASES:
        if c.exact or macs(c) > limit:
            continue
        n = len(applicable(c))
        if (c.family, c.op) not in pick or n > pick[(c.family, c.op)][0]:
            pick[(c.family, c.op)] = (n, c.name)
    return [pick[k][1] for k in sorted(pick)]


# ---------------------------------------------------------------- judge

Verdict = collections.namedtuple('Verdict', 'main sums squares bound exact_ok ok')


def _ratio(got, ref, bnd):
    """worst |got - ref| / bnd; a bound of 0 asks for equality; a NaN or inf is infinitely wrong"""
    got = got.double()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float('inf')))
    return float(r.max())


def judge(c, out, part, orc):
    """a device (or emulated) result against an oracle: worst error over bound of the elements, of the partial sums and of the
    partial sums of squares (each must stay under 1); an exact case must also equal the oracle bit for bit"""
    bd = bound(reduction_length(c))
    main = _ratio(out, orc['out'], bd * orc['scale'])
    s = q = 0.0
    if 'part' in orc:
        s = _ratio(part[:, :, 0], orc['part'][:, :, 0], orc['e_part'][:, :, 0])
        q = _ratio(part[:, :, 1], orc['part'][:, :, 1], orc['e_part'][:, :, 1])
    exact_ok = True
    if c.exact:
        exact_ok = bool(torch.equal(out.float(), orc['out'].float()))
        if 'part' in orc:
            exact_ok = exact_ok and bool(torch.equal(part.float(), orc['part'].float()))
    return Verdict(main, s, q, bd, exact_ok, bool(main < 1 and s < 1 and q < 1 and exact_ok))


def worst(v):
    return max(v.main, v.sums, v.squares)


def table_line(c, route, v):
    return '%-52s %-8s tile %2d ks %d dw %d blk %3d pz %d  err/bound %.3f  sum %.3f  sq %.3f  (bound %.2e)%s' % (
        c.name, route['family'], route['tile'], route['ksplit'], route['dw_splits'], route['stat_blocks'], route['psplits'],
        v.main, v.sums, v.squares, v.bound, '  bit-equal' if c.exact and v.exact_ok else '')


# ---------------------------------------------------------------- honest fp32 results (the CPU stand-in of a right kernel)

def emulate(c, inp):
    """(out, part) in fp32 as a correct kernel may give them: one fp32 convolution of the (rounded) operands, fp32 block sums"""
    q, P, T = rounding(c), c.KS // 2, c.T
    if c.op == 'dw':
        dy, xp = q(inp.dY), _pad(q(inp.X), P)
        return torch.stack([torch.einsum('bmt,bct->mc', dy, xp[:, :, k:k + T]) for k in range(c.KS)], 2), None
    if c.op == 'dx':
        return F.conv1d(_pad(q(inp.dY), P), flip_t(q(inp.W))), None
    y = F.conv1d(_pad(q(inp.X), P), q(inp.W), inp.bias)
    rows, nblk = block_rows(c)
    yt = y.transpose(1, 2).reshape(c.B * T, c.Cout)
    part = torch.stack([torch.zeros(nblk, c.Cout).index_add_(0, rows.reshape(-1), yt),
                        torch.zeros(nblk, c.Cout).index_add_(0, rows.reshape(-1), yt * yt)], 2)
    return y, part


# ---------------------------------------------------------------- the route query

def ask_route(lib, c, w_mod16=None):
    """t2v_conv1d_route for a case -> dict of the route fields, or the negative error code"""
    import ctypes as C
    v = [C.c_int(-1) for _ in range(8)]
    r = lib.t2v_conv1d_route(OPS.index(c.op), c.B, c.Cin, c.T, c.Cout, c.KS, c.bf16, 4 * c.w_off if w_mod16 is None else w_mod16,
                             *[C.byref(x) for x in v])
    if r < 0:
        return r
    assert lib.t2v_conv1d_route_name(r).decode() == FAMILIES[r]
    fb, tile, ks, dws, sb, scr, pz, pc = (x.value for x in v)
    return dict(family=FAMILIES[r], fallback=FAMILIES[fb], tile=tile, ksplit=ks, dw_splits=dws, stat_blocks=sb, dw_scratch_floats=scr,
                psplits=pz, pchunk=pc)


def expected_route(c):
    return dict(family=c.family, tile=c.tile, ksplit=c.ksplit, dw_splits=c.dw_splits, stat_blocks=c.stat_blocks, psplits=c.psplits,
                pchunk=c.pchunk)


ROUTE_KEYS = ('family', 'tile', 'ksplit', 'dw_splits', 'stat_blocks', 'psplits', 'pchunk')


def mismatch(c, got):
    """the fields in which a route answer differs from the case's expectation (a weight gradient is handed no partials)"""
    exp = expected_route(c)
    return dict((k, (got[k], exp[k])) for k in ROUTE_KEYS if got[k] != exp[k])
