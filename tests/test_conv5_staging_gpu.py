"""The k = 5 Conv1d forward / data-gradient kernel with its operands staged by LDS-DMA into a ring of k-tile stages
(k_conv5_fwd_dma in csrc/conv_gemm.hip) against the register-staged kernel it replaces (the same entry points with
T2V_CONV_STAGING=0, read once per process: that route runs in one child process for all shapes) and against an fp64 convolution.
Y, the BatchNorm partials, dX (with W given, and with W = NULL after t2v_conv1d_flip_weights: the training path) and dW must be
the same bits on both routes, and within the fp32 kernels' tolerance of tests/test_conv_bn_gpu.py of fp64."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, T)
SHAPES = [(1, 16, 64, 37),        # one k-tile, shorter than the ring; T < BN; unaligned rows
          (2, 32, 80, 83),        # two k-tiles; Cout not a multiple of 64; odd T
          (3, 48, 512, 37),       # three k-tiles, equal to the ring depth
          (2, 272, 128, 84),      # channel-split form with uneven halves (8 + 9 blocks)
          (6, 512, 512, 84),      # the encoder's launch
          (2, 512, 80, 400),      # last Postnet layer; halo at both utterance edges of every tile
          (6, 80, 512, 400)]      # Cin = 80
NAMES = ('y', 'stat_part', 'dx', 'dx_preflipped', 'dw')


def _inputs(B, Cin, Cout, T):
    g = torch.Generator().manual_seed(B * 1000 + T + Cin)
    x = torch.randn(B, Cin, T, generator=g) * torch.exp2(torch.randint(-4, 5, (B, Cin, T), generator=g).float())
    w = torch.randn(Cout, Cin, 5, generator=g) / (Cin * 5) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(B, Cout, T, generator=g)
    return x, w, bias, dy


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _conv(lib, gw, gx, gb, gdy, B, Cin, Cout, T):
    """(y, stat_part, dx, dx from pre-flipped weights, dw) through the C ABI, on the CPU"""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float('nan')
    nblk = lib.t2v_conv1d_stat_blocks(B, T, Cin, Cout, 5)
    y = torch.full((B, Cout, T), nan, device='cuda')
    part = torch.full((nblk, Cout, 2), nan, device='cuda')
    assert lib.t2v_conv1d_fwd(_p(gw), _p(gx), _p(gb), _p(y), _p(part), B, Cin, T, Cout, 5, st) == 0
    dx = torch.full((B, Cin, T), nan, device='cuda')
    wt = torch.empty_like(gw)
    assert lib.t2v_conv1d_bwd(_p(gw), _p(gx), _p(gdy), _p(dx), None, _p(wt), None, B, Cin, T, Cout, 5, st) == 0
    dx2 = torch.full((B, Cin, T), nan, device='cuda')
    wt2 = torch.empty_like(gw)
    PA, IA = C.c_void_p * 1, C.c_int * 1
    assert lib.t2v_conv1d_flip_weights(PA(gw.data_ptr()), PA(wt2.data_ptr()), IA(Cout), IA(Cin), 5, 1, st) == 0
    assert lib.t2v_conv1d_bwd(None, _p(gx), _p(gdy), _p(dx2), None, _p(wt2), None, B, Cin, T, Cout, 5, st) == 0
    dw = torch.full((Cout, Cin, 5), nan, device='cuda')
    nscr = lib.t2v_conv1d_dw_scratch_floats(B, Cin, T, Cout, 5)
    scr = torch.empty(nscr, device='cuda') if nscr else None
    assert lib.t2v_conv1d_bwd(None, _p(gx), _p(gdy), None, _p(dw), None, _p(scr), B, Cin, T, Cout, 5, st) == 0
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (y, part, dx, dx2, dw))


def _run_all():
    """every shape on the route this process's environment selects, x3 convolutions off (the fp32-MFMA kernels are under test)"""
    import t2v_hip
    lib = t2v_hip.load_library()
    prev = lib.t2v_conv1d_x3_set_mode(0)
    try:
        out = {}
        n0 = lib.t2v_conv1d_staged_launches()
        for shape in SHAPES:
            x, w, bias, dy = _inputs(*shape)
            out[shape] = _conv(lib, w.cuda(), x.cuda(), bias.cuda(), dy.cuda(), *shape)
        out['staged_launches'] = lib.t2v_conv1d_staged_launches() - n0
        return out
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)


@pytest.fixture(scope='module')
def routes(tmp_path_factory):
    """(staged route in this process, register-staged route from one child process)"""
    assert os.environ.get('T2V_CONV_STAGING', '1') != '0', 'this process must run the staged kernel'
    path = str(tmp_path_factory.mktemp('conv5_staging') / 'parent_route.pt')
    env = dict(os.environ, T2V_CONV_STAGING='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = _run_all(), torch.load(path, weights_only=False)
    # forward and both data gradients of every shape took the staged kernel here, and none of them in the child
    assert new['staged_launches'] == 3 * len(SHAPES) and old['staged_launches'] == 0, (new['staged_launches'], old['staged_launches'])
    return new, old


_REF = {}


def _fp64(shape):
    """fp64 results and the sums of absolute products that scale their errors, once per shape"""
    if shape not in _REF:
        x, w, bias, dy = (t.double() for t in _inputs(*shape))
        wr = w.clone().requires_grad_(True)
        y = F.conv1d(x, wr, bias, padding=2)
        dw, = torch.autograd.grad(y, wr, dy)
        wa = w.abs().requires_grad_(True)
        adw, = torch.autograd.grad(F.conv1d(x.abs(), wa, None, padding=2), wa, dy.abs())
        _REF[shape] = dict(y=y.detach(), ay=F.conv1d(x.abs(), w.abs(), bias.abs(), padding=2),
                           dx=F.conv_transpose1d(dy, w, padding=2), adx=F.conv_transpose1d(dy.abs(), w.abs(), padding=2),
                           dw=dw, adw=adw)
    return _REF[shape]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d_%dto%d_T%d' % (s[0], s[1], s[2], s[3]))
def test_staged_route_same_bits_and_fp32_class(routes, shape):
    B, Cin, Cout, T = shape
    new, old = routes[0][shape], routes[1][shape]
    for name, a, b in zip(NAMES, new, old):
        assert a.shape == b.shape and not torch.isnan(a).any(), name
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    y, part, dx, dx2, dw = (t.double() for t in new)
    r = _fp64(shape)
    # the bounds of test_conv1d_x3_is_fp32_class for the fp32-MFMA kernels: error over the sum of absolute products, K terms deep
    e_y = ((y - r['y']).abs() / r['ay']).max().item()
    e_dx = ((dx - r['dx']).abs() / (r['adx'] + 1e-30)).max().item()
    e_dx2 = ((dx2 - r['dx']).abs() / (r['adx'] + 1e-30)).max().item()
    e_dw = ((dw - r['dw']).abs() / (r['adw'] + 1e-30)).max().item()
    s = part.sum(0)
    e_s = (s[:, 0] - r['y'].sum((0, 2))).abs().max().item() / r['y'].abs().sum((0, 2)).max().item()
    e_q = (s[:, 1] - (r['y'] * r['y']).sum((0, 2))).abs().max().item() / (r['y'] * r['y']).sum((0, 2)).max().item()
    print('conv5 staging B=%d %d->%d T=%d: y %.2e dx %.2e / %.2e dw %.2e (BN sums %.1e / %.1e)' % (
        B, Cin, Cout, T, e_y, e_dx, e_dx2, e_dw, e_s, e_q))
    assert e_y < 2e-7 * max(4.0, (5 * Cin) ** 0.5), e_y
    assert e_dx < 2e-7 * max(4.0, (5 * Cout) ** 0.5) and e_dx2 < 2e-7 * max(4.0, (5 * Cout) ** 0.5), (e_dx, e_dx2)
    assert e_dw < 2e-7 * max(4.0, (B * T) ** 0.5), e_dw          # (the same rule for a sum over B T positions)
    assert e_s < 1e-5 and e_q < 1e-5, (e_s, e_q)


def test_weights_updated_in_place_are_seen():
    """nothing derived from the weights outlives a call: after an in-place update the next call computes with the new values"""
    import t2v_hip
    lib = t2v_hip.load_library()
    shape = B, Cin, Cout, T = (2, 32, 80, 83)
    x, w, bias, dy = _inputs(*shape)
    gw, gx, gb, gdy = w.cuda(), x.cuda(), bias.cuda(), dy.cuda()
    prev = lib.t2v_conv1d_x3_set_mode(0)
    try:
        first = _conv(lib, gw, gx, gb, gdy, *shape)
        gw.mul_(-0.5).add_(0.25)
        second = _conv(lib, gw, gx, gb, gdy, *shape)
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)
    w2 = gw.cpu().double()
    ref_y = F.conv1d(x.double(), w2, bias.double(), padding=2)
    ref_dx = F.conv_transpose1d(dy.double(), w2, padding=2)
    assert not torch.equal(first[0], second[0])
    assert (second[0].double() - ref_y).abs().max().item() < 1e-4 * ref_y.abs().max().item()
    for dx in (second[2], second[3]):
        assert (dx.double() - ref_dx).abs().max().item() < 1e-4 * ref_dx.abs().max().item()


if __name__ == '__main__':
    torch.save(_run_all(), sys.argv[1])
