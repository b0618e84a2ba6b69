"""fp64 reference of csrc/bn_act.hip (BatchNorm + tanh / ReLU / identity + dropout, forward and backward) with a worst-case
error bound per output, the cases tests/test_bn_paths_gpu.py runs and the mutated oracles it must reject.  Plain numpy, no GPU.

One function per kernel contract; each takes exactly the fp32 arrays the kernel receives:
    stats()     the statistics stage of t2v_bn_act_fwd in training: mean_out, rstd_out, the running buffers
    forward()   the apply stage, a function of the DEVICE's saved fp32 mean / rstd (running_* in eval), so that apply errors and
                statistics errors are judged separately; `lengths` gives t2v_bn_act_fwd_len
    backward()  t2v_bn_act_bwd / _bwd_eval: dy, dgamma, dbeta, dconv_bias

The bounds are first-order counts of the roundings of the kernels' operation sequence, u = 2^-24 per fp32 operation:
  statistics without partials   every thread adds L = ceil(n_wg / 256) values serially, 8 more adds go through the wave / block tree
                                (n_wg = B*T, or the slice's chunk on the split path; the slices' partials are then added in fp64):
                                ds <= (L + 8) u sum|y|, dq <= (L + 9) u sum y^2 (one more for the product), dmu = ds / n + u |mu|,
                                dvar = dq / n + 2 |mu| ds / n, drstd = u rstd + 0.5 rstd^3 dvar
  statistics from partials      the kernel adds the very fp32 partials it is given in fp64: u relative on mean_out,
                                dvar = 512 * 2^-53 * q / n
  running buffers               0.1 d + 3 u (|0.9 old| + |0.1 new|); d includes the rounding of the new value to fp32
  pre-activation z              g = gamma rstd (1 rounding), bt = beta - mean gamma rstd (3), z = fma(y, g, bt) (1):
                                E_z = 4 u (|y g| + |mean g| + |beta|)
  tanh                          tanhf_ = 1 - 2 rcp(1 + exp(2 z)), hardware exp and rcp taken as 1 ulp: 6 u + (1 - th^2) E_z
  keep scale                    1 / (1 - p) is rounded unless it is a power of two, and so is the product: 2 u |out|
  backward                      E_x = 2 u |xhat|, E_dz = 2 u |dz| (+ under tanh |dout scale| (2 |th| (6 u + (1 - th^2) E_z) + 3 u)),
                                dS1 = (L + 8 + P) u sum|dz| + sum E_dz, dS2 = (L + 9 + P) u sum|dz xhat| + sum(E_dz |xhat| + |dz| E_x),
                                ddy = |g| (E_dz + dS1 / n + |xhat| dS2 / n + E_x |S2| / n) + 6 u |g| (|dz| + |S1| / n + |xhat S2| / n);
                                P = slices whose partials are added serially (1 on the unsplit paths)
No constant here was fitted to a device result.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
EPS = float(np.float32(1e-5))            # eps and momentum cross the C ABI as floats
MOM = 0.1                                # (the 0.25 u between 0.1f and 0.1 is inside the 3 u of the running buffers)
ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
ACT_NAME = ('none', 'tanh', 'relu')
SEED, STREAM, RNG_T = 0x1234ABCD5678, 5, 7        # by-value dropout seed of every launch of the GPU test

MUTATIONS = ('stat_drop', 'slice_late', 'biased_running_var', 'eps_1e-3', 'tanh_deriv', 'eval_keeps_batch_terms',
             'bias_nonzero_train', 'keep_per_channel', 'pad_beta')


def chan(a):
    """(B, M, T) -> (M, B*T) float64: a channel's values in the order i = b * T + t the kernels index them by"""
    a = np.asarray(a, dtype=np.float64)
    B, M, T = a.shape
    return a.transpose(1, 0, 2).reshape(M, B * T)


def unchan(a, B, T):
    return a.reshape(a.shape[0], B, T).transpose(1, 0, 2)


def _col(v):
    return np.asarray(v, dtype=np.float64).reshape(1, -1, 1)


def plan(backward, B, M, T, training=1, has_partials=0):
    """(slices, chunk) as include/t2vae.h documents t2v_bn_act_slices: restated here, not read from the library"""
    n, per = B * T, 2048 if backward else 4096
    if M > 128 or n < 4 * per or (not backward and (not training or has_partials)):
        return 1, n
    S = (n + per - 1) // per
    if S * M > 1024:
        S = 1024 // M
    S = min(S, 64)
    if S < 2:
        return 1, n
    chunk = ((n + S - 1) // S + 255) // 256 * 256
    return (n + chunk - 1) // chunk, chunk


# ------------------------------------------------------------------------------------------------ statistics

Stats = namedtuple('Stats', 'mean var rstd run_mean run_var e_mean e_rstd e_run_mean e_run_var')


def stats(y, partials=None, n_wg=None, running_mean=None, running_var=None, eps=EPS, mutate=None, drop=None):
    """mu, biased var (clamped at 0), rstd, the new running buffers, and their bounds.  partials: the (nblk, M, 2) fp32 array the
    kernel is handed.  mutate 'stat_drop' / 'slice_late': element `drop` (per channel, or one index) is left out of the sums —
    with partials the last block is.  'biased_running_var', 'eps_1e-3': as they say."""
    yc = chan(y)
    M, n = yc.shape
    if partials is not None:
        p = np.asarray(partials, dtype=np.float64)
        tree = 512 * 2.0 ** -53
        if mutate == 'stat_drop':
            p = p[:-1]
        s, q = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
        ds, dq = tree * np.abs(p[:, :, 0]).sum(0), tree * p[:, :, 1].sum(0)
    else:
        if mutate in ('stat_drop', 'slice_late'):
            yc = yc.copy()
            yc[np.arange(M), np.broadcast_to(drop, (M,))] = 0.0
        L = math.ceil((n_wg or n) / 256)
        s, q = yc.sum(1), (yc * yc).sum(1)
        ds, dq = (L + 8) * U * np.abs(yc).sum(1), (L + 9) * U * q
    mu = s / n
    var = np.maximum(q / n - mu * mu, 0.0)
    e = 1e-3 if mutate == 'eps_1e-3' else eps
    rstd = 1.0 / np.sqrt(var + e)
    e_mean = ds / n + U * np.abs(mu)
    dvar = dq / n + 2 * np.abs(mu) * ds / n
    e_rstd = U * rstd + 0.5 * rstd ** 3 * dvar
    unb = var if mutate == 'biased_running_var' else var * n / (n - 1.0)
    e_unb = dvar * n / (n - 1.0) + U * unb
    rm0 = np.zeros(M) if running_mean is None else np.asarray(running_mean, dtype=np.float64)
    rv0 = np.ones(M) if running_var is None else np.asarray(running_var, dtype=np.float64)
    rm, rv = (1 - MOM) * rm0 + MOM * mu, (1 - MOM) * rv0 + MOM * unb
    e_rm = MOM * e_mean + 3 * U * (np.abs((1 - MOM) * rm0) + np.abs(MOM * mu))
    e_rv = MOM * e_unb + 3 * U * (np.abs((1 - MOM) * rv0) + np.abs(MOM * unb))
    return Stats(mu, var, rstd, rm, rv, e_mean, e_rstd, e_rm, e_rv)


def eval_rstd(running_var, eps=EPS, mutate=None):
    """rstd of the eval paths, 1.0f / sqrtf(running_var + eps) on the device: (fp64 value, relative bound).  The sum is rounded
    (u, halved by the root), the root and the quotient are correctly rounded (u each): 2.5 u, taken as 3 u."""
    e = 1e-3 if mutate == 'eps_1e-3' else eps
    return 1.0 / np.sqrt(np.asarray(running_var, dtype=np.float64) + e), 3 * U


# ------------------------------------------------------------------------------------------------ apply

def _pre(y, mean, rstd, gamma, beta, rstd_rel=0.0):
    y = np.asarray(y, dtype=np.float64)
    mean, rstd, gamma, beta = _col(mean), _col(rstd), _col(gamma), _col(beta)
    g = gamma * rstd
    z = (y - mean) * g + beta
    e_z = 4 * U * (np.abs(y * g) + np.abs(mean * g) + np.abs(beta)) + rstd_rel * np.abs((y - mean) * g)
    return z, e_z, g, (y - mean) * rstd


def _scale(keep_scale, shape):
    """(scale array, 2 u if some factor is no power of two else 0)"""
    if keep_scale is None:
        return np.ones(shape), 0.0
    s = np.asarray(keep_scale, dtype=np.float64)
    nz = s[s != 0]
    pow2 = nz.size == 0 or bool(np.all(np.frexp(nz)[0] == 0.5))
    return s, (0.0 if pow2 else 2 * U)


Fwd = namedtuple('Fwd', 'out e_out z e_z')


def forward(y, mean32, rstd32, gamma, beta, act, keep_scale=None, lengths=None, rstd_rel=0.0, mutate=None):
    """out = act(z) * keep_scale with z = (y - mean) gamma rstd + beta, 0 at t >= lengths[b]; keep_scale: (B, M, T) factors 0 or
    1 / (1 - p) in fp64 (None: no dropout).  rstd_rel: relative error of rstd itself where the kernel forms it (eval)."""
    z, e_z, g, _ = _pre(y, mean32, rstd32, gamma, beta, rstd_rel)
    if act == ACT_TANH:
        a = np.tanh(z)
        e_a = 6 * U + (1 - a * a) * e_z
    elif act == ACT_RELU:
        a, e_a = np.maximum(z, 0.0), e_z
    else:
        a, e_a = z, e_z
    s, e_s = _scale(keep_scale, z.shape)
    out = a * s
    e_out = e_a * s + e_s * np.abs(out)
    if lengths is not None:
        B, M, T = z.shape
        pad = np.arange(T)[None, None, :] >= np.asarray(lengths).reshape(B, 1, 1)
        pad = np.broadcast_to(pad, z.shape)
        out = np.where(pad, _col(beta) + 0 * z if mutate == 'pad_beta' else 0.0, out)
        e_out = np.where(pad, 0.0, e_out)
    return Fwd(out, e_out, z, e_z)


Bwd = namedtuple('Bwd', 'dy dgamma dbeta dbias e_dy e_dgamma e_dbeta e_dbias dz')


def backward(y, dout, mean32, rstd32, gamma, beta, act, eval_mode, keep_scale=None, L=None, P=1, mutate=None, drop=None):
    """dy, dgamma = S2, dbeta = S1, dconv_bias (exactly 0 in training, g S1 in eval) and their bounds.  L: values a thread adds
    serially (default ceil(n / 256)), P: slices added serially.  mutate 'stat_drop' / 'slice_late': element `drop` of every
    channel is left out of S1 / S2."""
    z, e_z, g, xhat = _pre(y, mean32, rstd32, gamma, beta)
    B, M, T = z.shape
    n = B * T
    s, e_s = _scale(keep_scale, z.shape)
    d = np.asarray(dout, dtype=np.float64) * s
    if act == ACT_TANH:
        th = np.tanh(z)
        dz = d * ((1 - th) if mutate == 'tanh_deriv' else (1 - th * th))
        e_dz = 2 * U * np.abs(dz) + np.abs(d) * (2 * np.abs(th) * (6 * U + (1 - th * th) * e_z) + 3 * U)
    else:
        dz = d * (z > 0) if act == ACT_RELU else d
        e_dz = 2 * U * np.abs(dz)
    e_x = 2 * U * np.abs(xhat)
    dzc, xc, e_dzc, e_xc = chan(dz), chan(xhat), chan(e_dz), chan(e_x)
    dzs = dzc
    if mutate in ('stat_drop', 'slice_late'):
        dzs = dzc.copy()
        dzs[np.arange(M), np.broadcast_to(drop, (M,))] = 0.0
    L = math.ceil(n / 256) if L is None else L
    S1, S2 = dzs.sum(1), (dzs * xc).sum(1)
    dS1 = (L + 8 + P) * U * np.abs(dzc).sum(1) + e_dzc.sum(1)
    dS2 = (L + 9 + P) * U * np.abs(dzc * xc).sum(1) + (e_dzc * np.abs(xc) + np.abs(dzc) * e_xc).sum(1)
    gs = g.reshape(M)
    gc = np.abs(gs)[:, None]
    if eval_mode and mutate != 'eval_keeps_batch_terms':
        dy = gs[:, None] * dzc
        e_dy = gc * e_dzc + 6 * U * gc * np.abs(dzc)
    else:
        dy = gs[:, None] * (dzc - S1[:, None] / n - xc * S2[:, None] / n)
        e_dy = gc * (e_dzc + dS1[:, None] / n + np.abs(xc) * dS2[:, None] / n + e_xc * np.abs(S2)[:, None] / n) \
            + 6 * U * gc * (np.abs(dzc) + np.abs(S1)[:, None] / n + np.abs(xc * S2[:, None]) / n)
    if eval_mode or mutate == 'bias_nonzero_train':
        dbias = gs * S1
        e_dbias = (np.abs(gs) * dS1 + 3 * U * np.abs(dbias)) if eval_mode else np.zeros(M)
    else:
        dbias, e_dbias = np.zeros(M), np.zeros(M)
    return Bwd(unchan(dy, B, T), S2, S1, dbias, unchan(e_dy, B, T), dS2, dS1, e_dbias, dzc)


def ratio(got, ref, bound, excuse=None):
    """(worst |got - ref| / bound, worst |got - ref|); a bound of 0 asks for equality, a NaN or inf is infinitely wrong"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    err = np.where(np.isfinite(got), err, np.inf)
    if excuse is not None:
        r = np.where(excuse, 0.0, r)
    return float(r.max()), float(err.max())


# ------------------------------------------------------------------------------------------------ cases

Case = namedtuple('Case', 'name kind path B M T act p training nblk slices cond gamma_hi bias lengths mut')
Case.__new__.__defaults__ = (ACT_NONE, 0.0, 1, 0, 1, 1.0, 1.5, 0, None, False)
# kind: 'fwd' t2v_bn_act_fwd, 'len' t2v_bn_act_fwd_len, 'bwd' t2v_bn_act_bwd (training = 1) / _bwd_eval (training = 0)
# slices: what t2v_bn_act_slices must answer, worked out by hand from the rule in include/t2vae.h
# cond: the channel offset c in units of the channel's spread (<= 1: c = uniform(-1, 1) std); mut: the mutation rows run on it


def _mk():
    cs = []

    def add(kind, path, B, M, T, **kw):
        tr = kw.get('training', 1)
        name = '%s_%s_%dx%dx%d_%s%s%s%s%s%s' % (
            kind, path, B, M, T, ACT_NAME[kw.get('act', 0)], '_p%g' % kw['p'] if kw.get('p') else '',
            '' if tr or kind != 'bwd' else '_eval', '_bias' if kw.get('bias') else '', '_nblk%d' % kw['nblk'] if kw.get('nblk') else '',
            ('_c%g' % kw['cond'] if kw.get('cond', 1.0) > 1 else '') + ('_g%g' % kw['gamma_hi'] if kw.get('gamma_hi', 1.5) != 1.5 else ''))
        cs.append(Case(name=name, kind=kind, path=path, B=B, M=M, T=T, **kw))

    N, TH, RE = ACT_NONE, ACT_TANH, ACT_RELU
    # forward, training, partials given: register apply n <= 3072, loop apply above
    add('fwd', 'partials_reg', 2, 3, 1, act=TH, nblk=1)
    add('fwd', 'partials_reg', 1, 5, 255, act=RE, nblk=3)
    add('fwd', 'partials_reg', 2, 4, 128, act=N, nblk=256)
    add('fwd', 'partials_reg', 1, 3, 257, act=TH, nblk=257)
    add('fwd', 'partials_reg', 37, 2, 83, act=RE, nblk=600)
    add('fwd', 'partials_reg', 3, 2, 1024, act=TH, nblk=3, p=0.5, mut=True)
    add('fwd', 'partials_loop', 7, 2, 439, act=N, nblk=257)
    add('fwd', 'partials_loop', 1, 2, 4097, act=TH, nblk=600, p=0.25, mut=True)
    # forward, training, no partials, one workgroup per channel
    add('fwd', 'reg', 1, 2, 2, act=N)
    add('fwd', 'reg', 257, 2, 1, act=TH)
    add('fwd', 'reg', 23, 3, 89, act=RE)
    add('fwd', 'reg', 2, 2, 1024, act=N)
    add('fwd', 'reg', 3, 2, 683, act=TH)
    add('fwd', 'reg', 4, 3, 768, act=TH, p=0.5, mut=True)
    add('fwd', 'reg', 4, 3, 768, act=RE, p=0.25)
    add('fwd', 'reg', 4, 3, 768, act=TH, gamma_hi=40.0)
    add('fwd', 'loop', 439, 2, 7, act=TH, p=0.25, mut=True)
    add('fwd', 'loop', 439, 2, 7, act=RE, p=0.5)
    add('fwd', 'loop', 3, 2, 5461, act=RE)
    add('fwd', 'loop', 1, 129, 16384, act=N)
    # forward, split over gridDim.y
    add('fwd', 'split', 1, 1, 16384, act=N, slices=4)
    add('fwd', 'split', 1, 1, 16384, act=TH, slices=4)
    add('fwd', 'split', 1, 1, 16384, act=RE, slices=4, p=0.5)
    add('fwd', 'split', 1, 1, 16384, act=N, slices=4, p=0.25)
    add('fwd', 'split', 443, 128, 37, act=TH, slices=5, p=0.5)
    add('fwd', 'split', 1, 3, 258050, act=RE, slices=64)          # ceil(258050 / 4096) = 64 of 4096: the last holds 2 elements
    add('fwd', 'split', 7, 100, 2400, act=TH, slices=5, p=0.25, mut=True)       # (5 x 100 workgroups: under the 1024 / M cap)
    add('fwd', 'split', 1, 1, 262145, act=TH, slices=61)          # 65 slices asked for, capped at 64, 61 hold an element
    add('fwd', 'split', 1, 128, 36900, act=RE, slices=8)          # 10 slices asked for, 1024 / M = 8
    # forward, eval: running statistics, no mean_out / rstd_out, p_drop ignored, never split
    add('fwd', 'eval_reg', 3, 4, 700, act=TH, p=0.5, training=0, mut=True)
    add('fwd', 'eval_reg', 1, 2, 1, act=RE, training=0)
    add('fwd', 'eval_loop', 5, 3, 1000, act=RE, p=0.25, training=0, mut=True)
    add('fwd', 'eval_loop', 1, 2, 20000, act=N, training=0)
    # eval over a ragged batch
    for T, act in ((1, N), (255, TH), (256, RE), (257, TH), (700, RE)):
        add('len', 'len', 5, 3, T, act=act, training=0, lengths=(0, 1, T - 1, T, T + 5), mut=(T == 257))
    # backward: register n <= 3072, loop, split; training and eval, dconv_bias NULL and given
    shapes = (('bwd_reg', 2, 3, 1, 1), ('bwd_reg', 1, 3, 257, 1), ('bwd_reg', 3, 2, 1024, 1),
              ('bwd_loop', 7, 2, 439, 1), ('bwd_loop', 1, 2, 8191, 1), ('bwd_loop', 1, 129, 8192, 1),
              ('bwd_split', 1, 1, 8192, 4), ('bwd_split', 443, 128, 37, 8), ('bwd_split', 1, 1, 131073, 57),
              ('bwd_split', 5, 100, 2400, 6))
    for k, (path, B, M, T, sl) in enumerate(shapes):
        mut = (B, M, T) in ((3, 2, 1024), (7, 2, 439), (5, 100, 2400))
        for v, (tr, bias) in enumerate(((1, 0), (1, 1), (0, 0), (0, 1))):
            act = TH if mut else (N, TH, RE)[(k + v) % 3]
            p = (0.5 if tr else 0.25) if mut else 0.0
            add('bwd', path, B, M, T, act=act, p=p, training=tr, bias=bias, slices=sl, mut=mut and bias == 1)
    add('bwd', 'bwd_reg', 4, 3, 768, act=RE, p=0.5, bias=1)
    add('bwd', 'bwd_reg', 4, 3, 768, act=TH, gamma_hi=40.0, bias=1)
    add('bwd', 'bwd_reg', 4, 3, 768, act=TH, gamma_hi=40.0, training=0, bias=1)      # eval: dy = g dz, exactly 0 where tanh saturates
    # ill-conditioned channels (mean = 8 / 64 spreads), measured with the same bounds: one case per statistics path
    for c in (8.0, 64.0):
        add('fwd', 'reg', 4, 3, 768, act=TH, cond=c)
        add('fwd', 'loop', 3, 2, 5461, act=RE, cond=c)
        add('fwd', 'split', 1, 1, 16384, act=N, slices=4, cond=c)
    add('bwd', 'bwd_reg', 4, 3, 768, act=TH, cond=64.0, bias=1)
    add('bwd', 'bwd_loop', 1, 2, 8191, act=N, cond=64.0, bias=1)
    add('bwd', 'bwd_split', 1, 1, 8192, act=RE, cond=64.0, slices=4, bias=1)
    return cs


CASES = _mk()
BY_NAME = dict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)
PATHS = ('partials_reg', 'partials_loop', 'reg', 'loop', 'split', 'eval_reg', 'eval_loop', 'len', 'bwd_reg', 'bwd_loop', 'bwd_split')
WELL = {'reg': 'fwd_reg_4x3x768_tanh_p0.5', 'loop': 'fwd_loop_3x2x5461_relu', 'split': 'fwd_split_1x1x16384_none'}


def visible(m, c):
    """can case c tell mutation m from the truth?  What a path cannot see is named here, not skipped in silence."""
    fwd_train = c.kind == 'fwd' and c.training
    split = c.path in ('split', 'bwd_split')
    return {'stat_drop': fwd_train or c.kind == 'bwd',                 # eval forward / fwd_len form no sums
            'slice_late': split,                                        # one workgroup per channel has no slices
            'biased_running_var': fwd_train,
            'eps_1e-3': c.kind != 'bwd',                                # the backward is handed rstd, it never sees eps
            'tanh_deriv': c.kind == 'bwd' and c.act == ACT_TANH,
            'eval_keeps_batch_terms': c.kind == 'bwd' and not c.training,
            'bias_nonzero_train': c.kind == 'bwd' and c.training and c.bias,
            'keep_per_channel': c.p > 0 and c.M > 1 and (fwd_train or c.kind == 'bwd'),     # eval forward ignores p_drop
            'pad_beta': c.kind == 'len'}[m]


Inputs = namedtuple('Inputs', 'y gamma beta run_mean run_var dout partials lengths')


def draw(c):
    """the fp32 arrays of a case: y = N(0, 1) 2^k + c per channel, gamma in [0.5, gamma_hi], beta = N(0, 0.1)"""
    g = np.random.default_rng(zlib.crc32(c.name.encode()))
    B, M, T = c.B, c.M, c.T
    k = g.integers(-3, 4, size=M)
    std = (2.0 ** k).astype(np.float32)
    off = (g.uniform(-1, 1, size=M) if c.cond <= 1 else c.cond * g.choice([-1.0, 1.0], size=M)).astype(np.float32) * std
    y = g.standard_normal((B, M, T), dtype=np.float32) * std[None, :, None] + off[None, :, None]
    gamma = g.uniform(0.5, c.gamma_hi, size=M).astype(np.float32)
    beta = (0.1 * g.standard_normal(M)).astype(np.float32)
    if c.training:
        rm, rv = g.standard_normal(M).astype(np.float32), g.uniform(0.5, 2.0, size=M).astype(np.float32)
    else:       # eval: running statistics near the channel's own
        rm = (off + 0.1 * std * g.standard_normal(M)).astype(np.float32)
        rv = (std * std * g.uniform(0.5, 2.0, size=M)).astype(np.float32)
    dout = g.standard_normal((B, M, T), dtype=np.float32) if c.kind == 'bwd' else None
    part = block_partials(y, c.nblk) if c.nblk else None
    lengths = np.asarray(c.lengths, dtype=np.int32) if c.lengths is not None else None
    return Inputs(y, gamma, beta, rm, rv, dout, part, lengths)


def block_partials(y, nblk):
    """(nblk, M, 2) fp32: fp64 [sum, sum of squares] of nblk consecutive runs of every channel (empty runs where nblk > n)"""
    yc = chan(y)
    M, n = yc.shape
    edges = (np.arange(nblk + 1) * n) // nblk
    out = np.zeros((nblk, M, 2), dtype=np.float64)
    cs, cq = np.concatenate([np.zeros((M, 1)), np.cumsum(yc, 1)], 1), np.concatenate([np.zeros((M, 1)), np.cumsum(yc * yc, 1)], 1)
    if n * nblk <= 1 << 22:      # exact block sums where that is cheap, differences of running sums (1e-16 relative) otherwise
        for b in range(nblk):
            out[b, :, 0] = yc[:, edges[b]:edges[b + 1]].sum(1)
            out[b, :, 1] = (yc[:, edges[b]:edges[b + 1]] ** 2).sum(1)
    else:
        out[:, :, 0] = (cs[:, edges[1:]] - cs[:, edges[:-1]]).T
        out[:, :, 1] = (cq[:, edges[1:]] - cq[:, edges[:-1]]).T
    return out.astype(np.float32)


def stats32(y, eps=EPS):
    """fp32 mean / rstd of y's own batch statistics: what a backward test hands the kernel"""
    st = stats(y, eps=eps)
    return st.mean.astype(np.float32), st.rstd.astype(np.float32)


def relu_margin(y, mean32, rstd32, gamma, beta):
    """|z| / E_z per element: below 1 a ReLU decision may go either way"""
    z, e_z, _, _ = _pre(y, mean32, rstd32, gamma, beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(e_z > 0, np.abs(z) / e_z, np.inf)


def nudge_relu(y, gamma, beta, rounds=3, margin=16.0):
    """y with every element whose pre-activation lies within margin * E_z of 0 moved away from it, the fp32 statistics of the
    moved y (they are recomputed every round, as the kernel is handed them), and how many elements were moved"""
    y = np.array(y, dtype=np.float32)
    moved = 0
    for _ in range(rounds):
        mean32, rstd32 = stats32(y)
        z, e_z, g, _ = _pre(y, mean32, rstd32, gamma, beta)
        bad = np.abs(z) < margin * e_z
        if not bad.any():
            break
        moved += int(bad.sum())
        step = 8 * margin * e_z / np.abs(g)
        y = np.where(bad, y + np.where(z >= 0, step, -step), y).astype(np.float32)
    mean32, rstd32 = stats32(y)
    assert not (relu_margin(y, mean32, rstd32, gamma, beta) < margin).any(), 'elements left at the ReLU threshold'
    return y, mean32, rstd32, moved
