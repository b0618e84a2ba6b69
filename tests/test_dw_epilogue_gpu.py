"""decoder_rnn's weight gradients from the reverse pass's own workgroups (t2v_achain_dw: the decoder_rnn role of k_achain_bwd goes on
with [d_w_ih_dec | d_w_hh_dec] = DGD^T · x_cur once its chain has ended, the grouped launch behind the pass computes what is left)
against the route without it (T2V_DW_EPILOGUE=0) and against an fp64 product of the saved DGD and XS."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

pytestmark = pytest.mark.gpu

KOEMO_IN = [84, 80, 71, 66, 50, 37]          # bench.py --koemo


def _nd(B, T_in):
    """decoder_rnn workgroups of k_achain_bwd (pba_na in csrc/decoder_train_bwd_persist.hip): the parties of the epilogue's barriers"""
    import t2v_hip as H
    NL = 256 - B * H.load_library().t2v_decoder_bwd_persist_slices(T_in)
    NA = NL - 128 if NL - 128 >= 86 else max((3 * NL + 4) // 8, 79)
    return NL - NA


def _epilogue_words(B, T_in, T):
    """(tiles taken, arrivals at barrier 1, arrivals at barrier 2) of the last kept reverse pass"""
    import t2v_hip as H
    off = H.load_library().t2v_decoder_bwd_achain_dw_offset(B, T_in, T)
    return H.DecoderCore.last_bwd_persist[2][6][off:off + 3].view(torch.int32).tolist()


def _decoder_grads(monkeypatch, B, T_in, T, lens=None, env=None, max_dec_b=None, cap=None, overlap=False):
    """one Decoder forward + backward; returns (d_w_ih_dec, d_w_hh_dec, DGD, XS, kernels, plans) — DGD / XS of the first chunk"""
    import hparams as HP
    import model as M
    import t2v_hip as H
    monkeypatch.delenv('T2V_DW_EPILOGUE', raising=False)
    monkeypatch.setattr(H.DecoderCore, 'dw_tile_cap', cap)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if max_dec_b is not None:
        monkeypatch.setattr(H, 'MAX_DEC_B', max_dec_b)
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    monkeypatch.setattr(H.DecoderCore, 'keep_last', True)
    torch.manual_seed(0)
    dec = M.Decoder(HP.create_hparams()).cuda().train()
    dec.p_attention_dropout = dec.p_decoder_dropout = 0.0
    g = torch.Generator().manual_seed(B * 1000 + T)
    mem = (torch.randn(B, T_in, 512, generator=g) * 0.5).cuda().requires_grad_(True)
    mels = torch.randn(B, 80, T, generator=g).cuda()
    lens = torch.tensor(lens if lens is not None else [T_in] * B, device='cuda')
    plans = H.DecoderCore.plan(H.load_library(), B, T_in, T, True)
    # overlap: the side streams of a training engine are active (weight gradients on the deferred-work / deferred-GEMM streams)
    # As in the engine, the two gradients then live in registered arena slots: autograd takes a returned gradient on the current
    # stream at once, the side streams are only joined afterwards.
    prev = H.set_overlap(H.Overlap()) if overlap else None
    w_ih, w_hh = dec.decoder_rnn.weight_ih, dec.decoder_rnn.weight_hh
    flat = torch.zeros(w_ih.numel() + w_hh.numel(), device='cuda')
    if overlap:
        H.register_grad_slots({w_ih.data_ptr(): (flat, 0, w_ih.shape), w_hh.data_ptr(): (flat, w_ih.numel(), w_hh.shape)})
    try:
        mel, gate, _ = dec(mem, mels, lens)
        (mel.sum() + gate.sum()).backward()
        if overlap:
            H.overlap().join()
    finally:
        if overlap:
            H.set_overlap(prev)
            H.register_grad_slots({})
    torch.cuda.synchronize()
    H.check_async_errors()
    DGD = XS = None
    if H.DecoderCore.last_bwd_persist is not None:
        _, _, bufs, _, keep = H.DecoderCore.last_bwd_persist
        DGD, XS = bufs[2], keep[4]
    if overlap:
        d_ih, d_hh = flat[:w_ih.numel()].view(w_ih.shape).clone(), flat[w_ih.numel():].view(w_hh.shape).clone()
    else:
        d_ih, d_hh = w_ih.grad.clone(), w_hh.grad.clone()
    return d_ih, d_hh, DGD, XS, list(H.DecoderCore.chunk_bwd_kernels), plans


def _rel_err(d_ih, d_hh, DGD, XS):
    """max |err| / sum_k |a b| of [d_w_ih_dec | d_w_hh_dec] against the fp64 product DGD^T · XS[1 : T + 1]"""
    T, B, _ = DGD.shape
    a = DGD.reshape(T * B, -1).double()
    x = XS[1:T + 1].reshape(T * B, -1).double()
    ref, absref = a.t() @ x, a.abs().t() @ x.abs()
    got = torch.cat([d_ih, d_hh], 1).double()
    return ((got - ref).abs() / absref.clamp_min(1e-30)).max().item()


SHAPES = [(6, 84, 400, None), (6, 84, 400, KOEMO_IN), (2, 37, 50, None)]


@pytest.mark.parametrize("B,T_in,T,lens", SHAPES, ids=['headline', 'koemo', 'small'])
def test_epilogue_matches_the_grouped_launch_and_fp64(monkeypatch, B, T_in, T, lens):
    """Both routes are fp32-class against fp64 (the bound of tests/test_gemm_gpu.py::test_x3_gemm_is_fp32_class), the epilogue's error is
    no more than 1.1 x the other route's + 2e-8 — and, since a tile is computed by the same code on the same planes whichever kernel
    takes it, the two routes agree bit for bit."""
    off = _decoder_grads(monkeypatch, B, T_in, T, lens, {'T2V_DW_EPILOGUE': '0'})
    on = _decoder_grads(monkeypatch, B, T_in, T, lens)
    assert on[4] == off[4] == ['k_achain_bwd']
    assert [p.dw_epilogue for p in on[5]] == [True] and [p.dw_epilogue for p in off[5]] == [False]
    assert torch.equal(on[2], off[2]) and torch.equal(on[3][1:T + 1], off[3][1:T + 1]), 'the two runs did not see the same DGD / x_cur'
    K = T * B
    e_off, e_on = _rel_err(off[0], off[1], off[2], off[3]), _rel_err(on[0], on[1], on[2], on[3])
    d = max((on[0] - off[0]).abs().max().item(), (on[1] - off[1]).abs().max().item())
    print('dW epilogue B=%d T_in=%d T=%d: max |err| / sum|ab|  epilogue %.3e  grouped launch %.3e  (bound %.3e); max |on - off| %.3e'
          % (B, T_in, T, e_on, e_off, 2e-7 * max(4.0, K ** 0.5), d))
    bound = 2e-7 * max(4.0, K ** 0.5)
    assert e_on < bound and e_off < bound, (e_on, e_off)
    assert e_on <= 1.1 * e_off + 2e-8, (e_on, e_off)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    # the epilogue ran: every decoder_rnn workgroup passed both barriers (the last run kept is the one with the epilogue)
    words = _epilogue_words(B, T_in, T)
    print('   tiles taken inside the pass %d of 640, barrier arrivals %s of %d' % (words[0], words[1:], _nd(B, T_in)))
    assert words[1] == words[2] == _nd(B, T_in), words


@pytest.mark.parametrize("max_dec_b,overlap", [(None, False), (6, False), (6, True)], ids=['one-chunk', 'two-chunks', 'two-chunks-side-streams'])
def test_batch_of_twelve(monkeypatch, max_dec_b, overlap):
    """B = 12.  As ONE chunk (the plan's 16 items per chunk) it is beyond the fp32 one-launch reverse pass: both switches give the
    launch-per-step pass and no epilogue.  As two chunks of 6 (the chunk size lowered for the test) the second chunk's epilogue and
    grouped launch add to what the first left: `accumulate`.  With side streams active the second chunk's pass (current stream) has to
    wait for the first chunk's grouped launch (deferred-GEMM stream): both add to the same tensors."""
    off = _decoder_grads(monkeypatch, 12, 84, 120, None, {'T2V_DW_EPILOGUE': '0'}, max_dec_b)
    on = _decoder_grads(monkeypatch, 12, 84, 120, None, None, max_dec_b, overlap=overlap)
    if max_dec_b is None:
        assert on[4] == off[4] and 'k_achain_bwd' not in on[4]
    else:
        assert on[4] == off[4] == ['k_achain_bwd'] * 2
    d = max((on[0] - off[0]).abs().max().item(), (on[1] - off[1]).abs().max().item())
    print('B = 12 (%s): max |on - off| %.3e of max |d_w_ih_dec| %.3e' % (max_dec_b, d, off[0].abs().max().item()))
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_hand_over_at_any_point_gives_the_same_bits(monkeypatch):
    """The test-only cap on the epilogue's tiles (DecoderCore.dw_tile_cap) at 0 (planes only), about half of the 640 tiles, an odd count
    (the second tile of the last pair is left to the grouped launch) and none: all within the fp32-class bound, a fixed cap is
    reproducible, and cap 0 equals the route without the epilogue bit for bit (so does every other cap)."""
    B, T_in, T = 6, 84, 400
    off = _decoder_grads(monkeypatch, B, T_in, T, None, {'T2V_DW_EPILOGUE': '0'})
    e_off = _rel_err(off[0], off[1], off[2], off[3])
    bound = 2e-7 * max(4.0, (T * B) ** 0.5)
    seen = {}
    for cap in (0, 320, 320, 37, None):
        r = _decoder_grads(monkeypatch, B, T_in, T, None, cap=cap)
        if cap in seen:         # a fixed cap, twice: identical bits
            assert torch.equal(r[0], seen[cap][0]) and torch.equal(r[1], seen[cap][1]), cap
        seen[cap] = r
        e = _rel_err(r[0], r[1], r[2], r[3])
        print('cap %s: max |err| / sum|ab| %.3e (route without the epilogue %.3e, bound %.3e)' % (cap, e, e_off, bound))
        assert e < bound and e <= 1.1 * e_off + 2e-8, (cap, e, e_off)
        assert torch.equal(r[0], off[0]) and torch.equal(r[1], off[1]), cap


def test_tiles_taken_are_counted_and_capped(monkeypatch):
    """the counter the grouped launch reads: a cap of 0 leaves it at 0; without a cap at the headline shape the pass takes tiles"""
    import t2v_hip as H
    lib = H.load_library()
    B, T_in, T = 6, 84, 400
    off = lib.t2v_decoder_bwd_achain_dw_offset(B, T_in, T)
    assert 0 < off == lib.t2v_decoder_bwd_achain_scratch_floats(B, T_in, T) - 16
    for cap, want in ((0, lambda n: n == 0), (None, lambda n: n > 0)):
        _decoder_grads(monkeypatch, B, T_in, T, None, cap=cap)
        n, *arrived = _epilogue_words(B, T_in, T)
        print('cap %s: %d of 640 tiles taken inside the pass; barrier arrivals %s' % (cap, n, arrived))
        assert want(n) and arrived[0] == arrived[1] == _nd(B, T_in), (cap, n, arrived)


def test_malformed_epilogue_struct_is_refused_before_any_launch(monkeypatch):
    """t2v_decoder_bwd_achain with a t2v_achain_dw that lacks planes or a gradient tensor, has misaligned planes or too short a row
    stride, or a product too shallow for the plane form (T * B < 32) returns an error and launches nothing: the buffers of a real
    pass, one field wrong at a time."""
    import t2v_hip as H
    lib = H.load_library()
    B, T_in, T = 2, 37, 50
    _decoder_grads(monkeypatch, B, T_in, T)
    PW, Sb, bufs, dims, keep = H.DecoderCore.last_bwd_persist
    good = keep[-1].dw
    before = bufs[6].clone()          # the pass's scratch: a launch (its preparation first) would refill the exchange arrays
    fields = [n for n, _ in H._AchainDw._fields_]

    def call(dw, dims):
        return lib.t2v_decoder_bwd_achain(C.byref(PW), C.byref(dw), C.byref(Sb), *([C.c_void_p(t.data_ptr()) for t in bufs] + list(dims) +
                                          [C.c_void_p(torch.cuda.current_stream().cuda_stream)]))

    for name, value in (('planes', None), ('planes', good.planes + 4), ('d_w_ih', None), ('d_w_hh', None), ('ld_ih', 1535), ('ld_hh', 1023)):
        bad = H._AchainDw(*[value if n == name else getattr(good, n) for n in fields])
        assert call(bad, dims) != 0, (name, value)
    assert call(good, (1, T_in, 16) + tuple(dims[3:])) != 0          # T * B = 16 < 32
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), bufs[6].view(torch.int32)), 'something was launched'


def test_argument_checks():
    """the error paths that need no fault: a hand-over without planes / counter, shapes without a plane form"""
    import t2v_hip as H
    lib = H.load_library()
    assert lib.t2v_decoder_bwd_achain_dw_offset(7, 84, 400) == -1 and lib.t2v_decoder_bwd_achain_dw_offset(6, 84, 0) == -1
    a = torch.zeros(64, 4096, device='cuda')
    x = torch.zeros(64, 2560, device='cuda')
    outs = [torch.zeros(4096, n, device='cuda') for n in (1024, 512, 1536, 1024)]
    groups = [(a.t(), [(x[:, :1024].t(), outs[0]), (x[:, 1024:1536].t(), outs[1])]),
              (a.t(), [(x[:, :1536].t(), outs[2]), (x[:, 1536:].t(), outs[3])])]
    arr = H._group_array(groups)
    ctr = torch.zeros(4, dtype=torch.int32, device='cuda')
    scr = torch.empty(lib.t2v_gemm_f32_grouped_scratch_floats(arr, 2, 4096, 64), device='cuda')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.t2v_gemm_f32_grouped_group_offset(arr, 2, 4096, 64, 0) == 0
    assert lib.t2v_gemm_f32_grouped_group_offset(arr, 2, 4096, 64, 1) == lib.t2v_gemm_f32_grouped_scratch_floats(arr, 1, 4096, 64)
    assert lib.t2v_gemm_f32_grouped_group_offset(arr, 2, 4096, 64, 2) == -1
    assert lib.t2v_gemm_f32_grouped_group_offset(arr, 2, 4096, 16, 1) == -1          # K < 32: no plane form
    assert lib.t2v_gemm_f32_grouped_handed(arr, 2, 4096, 64, 0, p(scr), 1, None, 0, st) != 0      # no counter
    assert lib.t2v_gemm_f32_grouped_handed(arr, 2, 4096, 64, 0, None, 1, p(ctr), 0, st) != 0      # no scratch
    assert lib.t2v_gemm_f32_grouped_handed(arr, 2, 4096, 64, 0, p(scr), 2, p(ctr), 0, st) != 0    # no such group
    assert lib.t2v_gemm_f32_grouped_handed(arr, 2, 4096, 64, 0, p(scr), -1, p(ctr), 0, st) != 0
    assert lib.t2v_gemm_f32_grouped_handed(arr, 2, 4096, 16, 0, p(scr), 1, p(ctr), 0, st) != 0    # K < 32
    torch.cuda.synchronize()
