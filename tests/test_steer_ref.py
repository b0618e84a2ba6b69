"""The steering recipe of tests/steer_ref.py on the reference alone: no GPU.  These are the conditions that make the bounds of
tests/test_decoder_steered_gpu.py mean something — the steered decoder is as well conditioned as the plain one (the fp32 oracle
stays at round-off of the fp64 one), every cut has mass on both sides at every step, and one halo tap of the location filter
lost at a cut, in the forward values or in the reverse pass alone, stands at least 1000 floors above the floor.

One case per cut (the one with the shortest T_in whose longest item contains it) and the two further (cut, case) pairs that the
device's mutation checks use; every figure is printed (pytest -s).  Measured: the least visible forward tap moves the alignments
by 10,800 floors (cut 384 at T_in = 555), the least visible reverse tap moves d memory by 4,200 floors (cut 480 at T_in = 555)."""
import pytest
import torch

import steer_ref as S

F32, F64 = torch.float32, torch.float64
# every cut in its smallest case, and the (cut, case) pairs that the device's mutation checks use beyond those; grouped by case, so
# that the cached oracles of a case are reused
BOUNDARIES = sorted(set((b, S.boundary_case(b)) for b in S.CUTS) | set(S.MUTATION_CUTS), key=lambda p: (p[1][1], p[0]))


def _id(case):
    return 'B%d-Tin%d-T%d' % case[:3]


def test_targets_and_boundary_cases():
    assert S.targets(20) == [0, 15, 16, 19] and S.targets(7) == [0, 6] and S.targets(16) == [0, 15] and S.targets(17) == [0, 15, 16]
    assert S.targets(97) == [0, 15, 16, 31, 32, 95, 96]
    assert S.targets(555) == [0, 15, 16, 31, 32, 95, 96, 127, 128, 191, 192, 287, 288, 383, 384, 479, 480, 511, 512, 554]
    assert S.targets(512)[-3:] == [479, 480, 511] and S.targets(513)[-3:] == [480, 511, 512]
    assert [S.boundary_case(b)[:3] for b in S.CUTS] == [(2, 20, 5), (16, 40, 3), (3, 97, 5), (2, 224, 4), (2, 224, 4),
                                                        (2, 555, 3), (2, 555, 3), (2, 555, 3), (2, 555, 3)]
    # every cut is inside some case, and every case's longest item is T_in
    assert all(c[3][0] == c[1] and len(c[3]) == c[0] and max(c[3]) == c[1] for c in S.CASES)


def test_steer_moves_the_processed_memory_along_sign_v_and_scales_the_location_term():
    import model as M
    import test_decoder_gpu as TD
    old = M.drop_rate
    try:
        dec, memory, lengths = (TD._setup(2, 20, 5, [20, 7])[i] for i in (2, 3, 5))
    finally:
        M.drop_rate = old
    al = dec.attention_layer
    dense = al.location_layer.location_dense.linear_layer.weight.detach().clone()
    steered = S.steer(dec, memory, [20, 7])
    assert steered.dtype == memory.dtype and steered is not memory
    assert torch.equal(al.location_layer.location_dense.linear_layer.weight.detach(), dense * 60)
    w, v = al.memory_layer.linear_layer.weight.detach().double(), al.v.linear_layer.weight.detach().double()[0]
    moved = (steered.double() - memory.double()) @ w.t()                        # (2, 20, 128)
    want = torch.zeros(2, 20, 128, dtype=F64)
    want[0, [0, 15, 16, 19]] = 0.4 * torch.sign(v)
    want[1, [0, 6]] = 0.4 * torch.sign(v)
    assert (moved - want).abs().max().item() < 1e-5                             # fp32 rounding of the steered memory
    # the same inputs every time: the oracle and the device are handed the same numbers
    a, b = S.inputs(S.CASES[0]), S.inputs(S.CASES[0])
    assert torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[0].state_dict().values(), b[0].state_dict().values()))
    assert torch.equal(a[1], steered)


def test_mutated_convolutions_lose_exactly_one_tap():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 2, 50, generator=g, dtype=F64)
    w = torch.randn(32, 2, 31, generator=g, dtype=F64)
    go = torch.randn(2, 32, 50, generator=g, dtype=F64)
    b = 32
    ref = torch.nn.functional.conv1d(x, w, None, padding=15)
    # by hand: output j of filter f loses w[f, c, b + 14 - j] x[c, b - 1] for j = b .. b + 14
    lost = torch.zeros_like(ref)
    for j in range(b, b + 15):
        lost[:, :, j] = torch.einsum('fc,nc->nf', w[:, :, b + 14 - j], x[:, :, b - 1])
    fwd = S._Functional(('fwd', b)).conv1d(x, w, None, padding=15)
    assert (fwd - (ref - lost)).abs().max().item() < 1e-12 and lost.abs().max().item() > 0.1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (torch.nn.functional.conv1d(xr, wr, None, padding=15) * go).sum().backward()
    xm, wm = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = S._Functional(('bwd', b)).conv1d(xm, wm, None, padding=15)
    assert torch.equal(y, ref)
    (y * go).sum().backward()
    dlost = torch.zeros_like(x)
    for j in range(b, b + 15):
        dlost[:, :, b - 1] += torch.einsum('fc,nf->nc', w[:, :, b + 14 - j], go[:, :, j])
    assert (xm.grad - (xr.grad - dlost)).abs().max().item() < 1e-12 and dlost.abs().max().item() > 0.1
    assert torch.equal(wm.grad, wr.grad)
    # the substitution ends with the call
    import t2v_oracle as O
    with S._substituted(('fwd', 16)):
        assert isinstance(O.F, S._Functional)
    assert O.F is torch.nn.functional


@pytest.mark.parametrize("case", S.CASES, ids=_id)
def test_floor_and_mass(case):
    """the fp32 oracle's alignments are within 1e-6 of the fp64 oracle's, and every target of every item holds at least 1e-3 of
    the mass at every step"""
    fl = S.floor(case)
    align = S.oracle(case, F64)[2]
    mass = min(align[i, :, S.targets(n)].min().item() for i, n in enumerate(case[3]))
    off = max(align[i, :, n:].abs().max().item() for i, n in enumerate(case[3]) if n < case[1])
    print('steered floor %s: ' % _id(case) + ' '.join('%s %.2e' % (q, fl[q]) for q in S.QUANTITIES) + '; least target mass %.2e' % mass)
    assert fl['align'] < 1e-6, fl
    assert mass >= 1e-3, mass
    assert off == 0.0


@pytest.mark.parametrize("b,case", BOUNDARIES, ids=['%d-%s' % (b, _id(c)) for b, c in BOUNDARIES])
def test_a_lost_halo_tap_is_visible(b, case):
    """input position b - 1 no longer reaches location-conv outputs b .. b + 14: in the forward pass the alignments move by at
    least 1000 floors; in the reverse pass alone the forward values stay bit-identical and the worse of parameter gradients and
    d memory moves by at least 1000 floors"""
    fl, ref = S.floor(case), S.oracle(case, F64)
    fwd = S.compare(S.oracle(case, F64, ('fwd', b)), ref)
    ratio_f = fwd['align'][0] / fl['align']
    bwd_res = S.oracle(case, F64, ('bwd', b))
    assert all(torch.equal(bwd_res[i], ref[i]) for i in range(3))
    bwd = S.compare(bwd_res, ref)
    ratio_g, ratio_m = bwd['grad'][0] / fl['grad'], bwd['d_memory'][0] / fl['d_memory']
    print('lost tap at %d in %s: fwd align %.2e = %.0f floors; bwd grad %.2e = %.0f floors (%s), d_memory %.2e = %.0f floors' % (
        b, _id(case), fwd['align'][0], ratio_f, bwd['grad'][0], ratio_g, bwd['grad'][1][0], bwd['d_memory'][0], ratio_m))
    assert ratio_f >= 1000, ratio_f
    assert max(ratio_g, ratio_m) >= 1000, (ratio_g, ratio_m)


@pytest.mark.parametrize("T_in,B", S.DECODE_CASES)
def test_decode_floor_and_mass(T_in, B):
    """free-running decode, 6 frames: the same two conditions"""
    fl = S.decode_floor(T_in, B)
    mel, gate, align = S.decode_oracle(T_in, B, F64)
    assert mel.shape == (B, 80, 6) and gate.shape == (B, 6) and align.shape == (B, 6, T_in)
    mass = align[:, :, S.targets(T_in)].min().item()
    print('steered decode floor T_in=%d B=%d: ' % (T_in, B) + ' '.join('%s %.2e' % (q, fl[q]) for q in ('mel', 'gate', 'align')) +
          '; least target mass %.2e' % mass)
    assert fl['align'] < 1e-6, fl
    assert mass >= 1e-3, mass
