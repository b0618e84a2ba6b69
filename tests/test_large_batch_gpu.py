"""Batches above 16 — the reference trains at batch_size = 64 (hparams.py) — where the product takes paths that the B <= 16 tests
never reach: the recurrent modules run in chunks of MAX_DEC_B = 16 items (BiLSTM, GRULast, DecoderCore, whose chunks pick their
engines one by one), the encoder conv bank goes to the x3 Conv1d, and the Postnet's x3 scratch outgrows its ring at long T.

Every test compares with a plain high-precision reference — fp64 torch (on the CPU, or for the B = 64 convolutions fp64
F.pad + unfold + matmul on the GPU) or the CPU oracle — and asserts the dispatch path it was written for (chunk count, per-chunk
engine, x3 or tiled conv), so that a change of dispatch cannot turn it into a test of something else."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _conv1d_f64(x, w, b=None):
    """fp64 'same' Conv1d on the GPU without the project's kernels: F.pad + unfold + one float64 matmul"""
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    cols = F.pad(x, (K // 2, K // 2)).unfold(2, K, 1)                       # (B, Cin, T, K)
    y = cols.permute(0, 2, 1, 3).reshape(B * T, Cin * K) @ w.reshape(Cout, Cin * K).t()
    y = y.view(B, T, Cout).permute(0, 2, 1)
    return y if b is None else y + b[None, :, None]


# ------------------------------------------------------------------------------------------------------------ Conv1d at B = 64
CONV_SHAPES = [(80, 512, 400), (80, 512, 1153), (80, 512, 1300), (512, 512, 400), (512, 512, 1153), (512, 512, 1300),
               (512, 80, 400), (512, 80, 1153), (512, 80, 1300), (512, 512, 84)]


def _conv_inputs(B, Cin, Cout, T, dc):
    g = torch.Generator().manual_seed(Cin * 7 + Cout * 3 + T)
    x = torch.randn(B, Cin, T, generator=g) * (2.5 if dc else 1.0) + (-6.0 if dc else 0.0)      # dc: log-mel-like input
    w = torch.randn(Cout, Cin, 5, generator=g) / (Cin * 5) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    rm, rv = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    wo = torch.randn(B, Cout, T, generator=g)
    return x, w, bias, gamma, beta, rm, rv, wo


@pytest.mark.parametrize("Cin,Cout,T,dc", [s + (False,) for s in CONV_SHAPES] + [(80, 512, 1153, True)])
def test_conv_bn_act_b64_default_dispatch_fp32(Cin, Cout, T, dc):
    """ConvBNAct1d (Conv1d k = 5 + training BatchNorm + tanh) at B = 64 in the DEFAULT dispatch mode, the Postnet shapes at
    T = 400 / 1153 / 1300 and the encoder's 512 -> 512 at T = 84 (256 tiles: the x3 path); dc: input with a log-mel-like offset
    (mean -6, std 2.5), the case where the one-pass q/n - mu^2 variance cancels.
    Reference: fp64 on the GPU (unfold + float64 matmul; BatchNorm, tanh and autograd in float64).
    Bounds: the raw convolution and its data gradient through the C ABI are held to test_conv1d_x3_is_fp32_class's
    2e-7 * max(4, sqrt(5 Cin)) of sum |w||x| per element, its BatchNorm partial sums (prefilled with NaN: every row written) to
    1e-5; through ConvBNAct1d the output may move by that conv bound carried through the normalisation (gamma * rstd, the
    mean's and the variance's share) plus fp32 round-off, and dX, dW, dgamma,
    dbeta — fp32 sums over B*T = 25 600 .. 83 200 products, random-walk error ~sqrt(N) * 2^-24 < 2e-5 — by 1e-4 of each
    tensor's largest entry.  The running statistics: 0.9 * init + 0.1 * batch statistic (unbiased variance for running_var),
    within 1e-6 of the channel's second moment mu^2 + var (what the fp32 partial sums carry) + fp32 round-off of the update.
    Path: whether t2v_conv1d_takes_x3 says x3 follows the tile count and the scratch cap, and is asserted
    (512 -> 512 at T = 1153 / 1300 need more than the ring's 64 M-float cap per call: the tiled kernels run them)."""
    import t2v_hip
    lib = t2v_hip.load_library()
    B = 64
    x, w, bias, gamma, beta, rm, rv, wo = _conv_inputs(B, Cin, Cout, T, dc)
    dev = 'cuda'
    # ---- ConvBNAct1d (the product's entry) first, then its fp64 graph
    gi = [t.to(dev).clone().requires_grad_(True) for t in (x, w, bias, gamma, beta)]
    grm, grv = rm.to(dev).clone(), rv.to(dev).clone()
    out = t2v_hip.ConvBNAct1d.apply(gi[0], gi[1], gi[2], gi[3], gi[4], grm, grv, True, 1, 0.0, 1, 1, 1)
    (out * wo.to(dev)).sum().backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    # ---- the path: x3 at >= 192 tiles (default mode 2) when the call's scratch fits the ring's cap (64 M floats)
    tiles = B * ((T + 127) // 128) * ((Cout + 127) // 128)
    w_slots = 5 * 3 * ((Cin + 15) // 16 * 2) * ((Cout + 127) // 128 * 128)
    x_slots = B * 3 * ((Cin + 15) // 16 * 2) * (((T + 127) // 128 * 128 + 8 + 63) // 64 * 64)
    fits = 4 * (w_slots + x_slots) <= (64 << 20)
    assert lib.t2v_conv1d_x3_set_mode(-1) == 2 and lib.t2v_gemm_f32_set_mode(-1) == 1
    exp_x3 = tiles >= 192 and fits
    assert lib.t2v_conv1d_takes_x3(B, Cin, T, Cout, 5, 0) == int(exp_x3), (tiles, fits)
    if (Cin, Cout, T) == (512, 512, 84):
        assert exp_x3                                       # the encoder conv bank at B = 64 is on the x3 kernels
    if (Cin, Cout, T) == (512, 512, 1153):
        assert not fits                                     # the shape the unchecked scratch used to fail with T2V_ERR_LAUNCH

    r = [t.to(dev).double().requires_grad_(True) for t in (x, w, bias, gamma, beta)]
    yr = _conv1d_f64(r[0], r[1], r[2])
    mu, var_b = yr.mean((0, 2)), yr.var((0, 2), unbiased=False)
    rstd = torch.rsqrt(var_b + 1e-5)
    z = (yr - mu[None, :, None]) * rstd[None, :, None]
    ref = torch.tanh(z * r[3][None, :, None] + r[4][None, :, None])
    (ref * wo.to(dev).double()).sum().backward()
    n = B * T
    x64, w64, b64 = r[0].detach(), r[1].detach(), r[2].detach()
    ref_y = yr.detach()
    aref = _conv1d_f64(x64.abs(), w64.abs(), b64.abs())
    bound = 2e-7 * max(4.0, (5 * Cin) ** 0.5)
    with torch.no_grad():
        # the statistics are sums of y and y^2 in fp32 partials: their error is relative to the second moment mu^2 + var
        m2 = mu * mu + var_b
        ga, rs, zd = r[3].detach().abs()[None, :, None], rstd[None, :, None], z.detach().abs()
        abar = aref.mean((0, 2))[None, :, None]
        tol = (bound * ga * rs * (aref + abar * (2.0 + zd)) + ga * zd * (1e-5 * m2 / (2 * var_b))[None, :, None]
               + 4e-6 * (1.0 + ref.detach().abs()))
        err = (out.double() - ref.detach()).abs()
        assert (err <= tol).all(), ('output', (err / tol).max().item())
        exp_rm = 0.9 * rm.to(dev).double() + 0.1 * mu
        exp_rv = 0.9 * rv.to(dev).double() + 0.1 * var_b * n / (n - 1)
        e_rm = ((grm.double() - exp_rm).abs() / (1e-6 * m2.sqrt() + 2e-7 * exp_rm.abs() + 1e-9)).max().item()
        e_rv = ((grv.double() - exp_rv).abs() / (1e-6 * m2 + 2e-7 * exp_rv)).max().item()
        assert e_rm < 1.0 and e_rv < 1.0, (e_rm, e_rv)
        for name, a, b in (('dx', gi[0].grad, r[0].grad), ('dw', gi[1].grad, r[1].grad), ('dgamma', gi[3].grad, r[3].grad),
                           ('dbeta', gi[4].grad, r[4].grad)):
            d = (a.double() - b).abs().max().item()
            assert d < 1e-4 * b.abs().max().item(), (name, d, b.abs().max().item())
    del r, yr, z, ref, gi, out

    # ---- the raw convolution through the C ABI: output, every BatchNorm partial row (NaN-prefilled), data gradient
    gx, gw, gb = x.to(dev), w.to(dev), bias.to(dev)
    nblk = lib.t2v_conv1d_stat_blocks(B, T, Cin, Cout, 5)
    if exp_x3:
        assert nblk == B * ((T + 127) // 128)
    y = torch.full((B, Cout, T), float('nan'), device=dev)
    part = torch.full((nblk, Cout, 2), float('nan'), device=dev)
    assert lib.t2v_conv1d_fwd(_p(gw), _p(gx), _p(gb), _p(y), _p(part), B, Cin, T, Cout, 5, _st()) == 0
    dyr = wo.to(dev)
    dx = torch.full((B, Cin, T), float('nan'), device=dev)
    wt = torch.empty_like(gw)
    assert lib.t2v_conv1d_bwd(_p(gw), _p(gx), _p(dyr), _p(dx), None, _p(wt), None, B, Cin, T, Cout, 5, _st()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(part).any() and not torch.isnan(dx).any()
    e_y = ((y.double() - ref_y).abs() / aref).max().item()
    wf = w64.flip(2).transpose(0, 1).contiguous()
    ref_dx = _conv1d_f64(dyr.double(), wf)
    aref_dx = _conv1d_f64(dyr.double().abs(), wf.abs())
    e_dx = ((dx.double() - ref_dx).abs() / (aref_dx + 1e-30)).max().item()
    s = part.double().sum(0)
    e_s = (s[:, 0] - ref_y.sum((0, 2))).abs().max().item() / ref_y.abs().sum((0, 2)).max().item()
    e_q = (s[:, 1] - (ref_y * ref_y).sum((0, 2))).abs().max().item() / (ref_y * ref_y).sum((0, 2)).max().item()
    assert e_y < bound and e_dx < 2e-7 * max(4.0, (5 * Cout) ** 0.5), (e_y, e_dx)
    assert e_s < 1e-5 and e_q < 1e-5, (e_s, e_q)


@pytest.mark.parametrize("Cin,Cout,T", CONV_SHAPES)
def test_conv_b64_bf16_plane_kernels_match_the_rounded_product(Cin, Cout, T):
    """bf16_run's Conv1d forward / data gradient (t2v_conv1d_fwd_bf16 / t2v_conv1d_bwd_bf16) at B = 64 in the default dispatch
    mode.  Reference: the fp64 convolution of the bf16-ROUNDED operands on the GPU (unfold + float64 matmul), as in
    test_conv_bf16_plane_kernels_match_the_rounded_product: output and data gradient within 2e-5 of the largest reference
    entry, the BatchNorm partial sums (prefilled with NaN: every row written) within 1e-5.  Path: one-plane kernels where
    t2v_conv1d_takes_x3(.., bf16 = 1) says so (>= 192 tiles and the scratch within the cap), asserted for the encoder shape."""
    import t2v_hip
    lib = t2v_hip.load_library()
    B = 64
    g = torch.Generator().manual_seed(Cin + Cout + T)
    dev = 'cuda'
    x = torch.randn(B, Cin, T, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 5, generator=g) / (Cin * 5) ** 0.5).to(dev)
    bias = (torch.randn(Cout, generator=g) * 0.1).to(dev)
    dy = torch.randn(B, Cout, T, generator=g).to(dev)
    tiles = B * ((T + 127) // 128) * ((Cout + 127) // 128)
    w_slots = 5 * ((Cin + 31) // 32 * 4) * ((Cout + 127) // 128 * 128)
    x_slots = B * ((Cin + 31) // 32 * 4) * (((T + 127) // 128 * 128 + 8 + 63) // 64 * 64)
    exp_x3 = tiles >= 192 and 4 * (w_slots + x_slots) <= (64 << 20)
    assert lib.t2v_conv1d_takes_x3(B, Cin, T, Cout, 5, 1) == int(exp_x3)
    if (Cin, Cout, T) == (512, 512, 84):
        assert exp_x3
    xr, wr, dyr = x.bfloat16().double(), w.bfloat16().double(), dy.bfloat16().double()
    ref = _conv1d_f64(xr, wr, bias.double())
    ref_dx = _conv1d_f64(dyr, wr.flip(2).transpose(0, 1).contiguous())
    nblk = lib.t2v_conv1d_stat_blocks_bf16(B, T, Cin, Cout, 5)
    wp = torch.empty(w.numel(), device=dev, dtype=torch.bfloat16)
    y = torch.full((B, Cout, T), float('nan'), device=dev)
    part = torch.full((nblk, Cout, 2), float('nan'), device=dev)
    assert lib.t2v_conv1d_fwd_bf16(_p(w), _p(x), _p(bias), _p(y), _p(part), _p(wp), B, Cin, T, Cout, 5, _st()) == 0
    dx = torch.full((B, Cin, T), float('nan'), device=dev)
    assert lib.t2v_conv1d_bwd_bf16(_p(w), _p(x), _p(dy), _p(dx), None, _p(wp), None, B, Cin, T, Cout, 5, _st()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(part).any() and not torch.isnan(dx).any()
    s = part.double().sum(0)
    res = ((y.double() - ref).abs().max().item() / ref.abs().max().item(),
           (dx.double() - ref_dx).abs().max().item() / ref_dx.abs().max().item(),
           (s[:, 0] - ref.sum((0, 2))).abs().max().item() / ref.abs().sum((0, 2)).max().item(),
           (s[:, 1] - (ref * ref).sum((0, 2))).abs().max().item() / (ref * ref).sum((0, 2)).max().item())
    assert res[0] < 2e-5 and res[1] < 2e-5 and res[2] < 1e-5 and res[3] < 1e-5, res


# ------------------------------------------------------------------------------------------------------- BiLSTM / GRU chunks
def _bilstm_lengths(B, T):
    """descending, ragged: every later chunk's longest item is well short of T; the tail has items of length 1"""
    return [max(1, int(round(T * (1.0 - i / B) ** 2))) for i in range(B)]


@pytest.mark.parametrize("B", [17, 33, 64])
def test_bilstm_chunks_match_packed_lstm_fp64(B):
    """BiLSTM above 16 items: ceil(B / 16) chunks in both passes (per-chunk dg joined by torch.cat in the backward).
    Reference: packed nn.LSTM in float64 on the CPU, output and all gradients.  Bounds of test_bilstm_matches_packed_lstm:
    output 2e-5 absolute, gradients 2e-3 of each tensor's largest entry; padded rows exactly zero; bit-reproducible.
    Path: the number of chunks the forward recorded."""
    import t2v_hip
    T = 84
    lens = _bilstm_lengths(B, T)
    torch.manual_seed(B)
    lstm = nn.LSTM(512, 256, 1, batch_first=True, bidirectional=True).double()
    g = torch.Generator().manual_seed(B + 1)
    x = torch.randn(B, T, 512, generator=g)
    wo = torch.randn(B, T, 512, generator=g)
    lengths = torch.tensor(lens)
    cx = x.double().clone().requires_grad_(True)
    out, _ = lstm(nn.utils.rnn.pack_padded_sequence(cx, lengths, batch_first=True))
    ref, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    (ref * wo.double()).sum().backward()
    runs = []
    for rep in range(2):
        P = {k: v.detach().float().clone().cuda().requires_grad_(True) for k, v in lstm.named_parameters()}
        gx = x.clone().cuda().requires_grad_(True)
        y = t2v_hip.BiLSTM.apply(gx, lengths.cuda().int(), P['weight_ih_l0'], P['weight_hh_l0'], P['bias_ih_l0'],
                                 P['bias_hh_l0'], P['weight_ih_l0_reverse'], P['weight_hh_l0_reverse'],
                                 P['bias_ih_l0_reverse'], P['bias_hh_l0_reverse'], True)
        assert len(y.grad_fn.keep[6]) == (B + 15) // 16        # chunks of MAX_DEC_B = 16
        (y * wo.cuda()).sum().backward()
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
        runs.append((y.detach(), gx.grad, {k: p.grad for k, p in P.items()}))
    y, dxg, grads = runs[0]
    assert torch.equal(y, runs[1][0]) and torch.equal(dxg, runs[1][1])
    assert all(torch.equal(grads[k], runs[1][2][k]) for k in grads), 'not reproducible'
    assert (y.cpu().double() - ref).abs().max().item() < 2e-5
    for b, n in enumerate(lens):
        if n < T:
            assert float(y[b, n:].abs().max()) == 0.0, b
    assert (dxg.cpu().double() - cx.grad).abs().max().item() < 2e-3 * cx.grad.abs().max().item() + 1e-6
    for k, p in lstm.named_parameters():
        d = (grads[k].cpu().double() - p.grad).abs().max().item()
        assert d < 2e-3 * p.grad.abs().max().item() + 1e-6, (k, d)


@pytest.mark.parametrize("T", [1, 16, 19, 25])
@pytest.mark.parametrize("B", [17, 64])
def test_gru_last_chunks_match_torch_fp64(B, T):
    """GRULast above 16 items (chunks share one exchange buffer; the backward reuses the forward's sync words) and beyond the
    T <= 16 steps of the reference encoder's comment (T_out = 1200 frames give 19).  Reference: nn.GRU in float64 on the CPU,
    last hidden state and all gradients.  Bounds of test_gru_last_matches_torch: 2e-5 absolute on the state, 2e-4 of each
    gradient's largest entry; bit-reproducible.  Path: one sync record per chunk of 16."""
    import t2v_hip
    torch.manual_seed(B * 10 + T)
    gru = torch.nn.GRU(256, 256, batch_first=True).double()
    g = torch.Generator().manual_seed(B + T)
    x = torch.randn(B, T, 256, generator=g)
    wo = torch.randn(B, 256, generator=g)
    xr = x.double().clone().requires_grad_(True)
    _, h = gru(xr)
    (h[0] * wo.double()).sum().backward()
    refs = [xr.grad, gru.weight_ih_l0.grad, gru.weight_hh_l0.grad, gru.bias_ih_l0.grad, gru.bias_hh_l0.grad]
    runs = []
    for rep in range(2):
        params = [p.detach().float().clone().cuda().requires_grad_(True) for p in
                  (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
        xg = x.clone().cuda().requires_grad_(True)
        out = t2v_hip.GRULast.apply(xg, *params)
        assert len(out.grad_fn.keep[6]) == (B + 15) // 16
        (out * wo.cuda()).sum().backward()
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
        runs.append([out.detach()] + [xg.grad] + [p.grad for p in params])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), 'not reproducible'
    assert (runs[0][0].cpu().double() - h[0]).abs().max().item() < 2e-5
    for name, got, ref in zip(('dx', 'dw_ih', 'dw_hh', 'db_ih', 'db_hh'), runs[0][1:], refs):
        scale = ref.abs().max().item() + 1e-6
        assert (got.cpu().double() - ref).abs().max().item() < 2e-4 * scale + 1e-6, name


# ------------------------------------------------------------------------------------ DecoderCore, bf16_run, default engines
def _dec_run(dec, mem0, mels, lens, mode):
    import t2v_hip as H
    if mode == 'default':
        H.DecoderCore.persistent = H.DecoderCore.persistent16 = H.DecoderCore.persistent_bwd = None
    else:
        H.DecoderCore.persistent = H.DecoderCore.persistent16 = H.DecoderCore.persistent_bwd = False
    dec._calls = 0
    for q in dec.parameters():
        q.grad = None
    mem = mem0.clone().requires_grad_(True)
    mel, gate, al = dec(mem, mels, lens)
    kf = list(H.DecoderCore.chunk_kernels)
    (mel.sum() + 0.3 * gate.sum() + 0.01 * (mel * mel).sum()).backward()
    torch.cuda.synchronize()
    H.check_async_errors()
    grads = {n: q.grad.clone() for n, q in dec.named_parameters() if q.grad is not None}
    grads['memory'] = mem.grad.clone()
    return kf, list(H.DecoderCore.chunk_bwd_kernels), mel.detach(), gate.detach(), al.detach(), grads


@pytest.mark.parametrize("B,T_in,T", [(20, 84, 12), (22, 60, 10), (64, 84, 8)])
def test_decoder_bf16_default_engines_match_launch_per_step(B, T_in, T):
    """bf16_run, B = 20 / 22 / 64 under the DEFAULT engine selection: every 16-item chunk takes k_dec_train_persist16 and
    k_bwd_persist16, a 4- or 6-item tail chunk the fp32-weight persistent kernels (k_dec_train_persist, k_achain_bwd) — both
    kinds in one forward and one reverse pass (asserted per chunk).  Reference: the launch-per-step bf16 loop on the same inputs
    and weights (state dropout on, same masks), at the bounds of test_decoder_persist16_gpu.py: outputs within 1e-2 of their
    scale (max) and 3e-4 (mean); gradients within 3e-2 of each tensor's scale + 1e-3 of the largest.  The items of a tail chunk
    run on fp32 weights: they are held to the same bounds (the bf16 loop's rounding is what separates them)."""
    import hparams as HP
    import model as M
    import t2v_hip as H
    old = (M.drop_rate, H.DecoderCore.persistent, H.DecoderCore.persistent16, H.DecoderCore.persistent_bwd, H.bf16_enabled())
    M.drop_rate = 0.0
    H.set_bf16(True)
    try:
        torch.manual_seed(0)
        dec = M.Decoder(HP.create_hparams("bf16_run=True")).cuda().train()
        dec.p_attention_dropout = dec.p_decoder_dropout = 0.1
        g = torch.Generator().manual_seed(B)
        mem0 = (torch.randn(B, T_in, 512, generator=g) * 0.5).cuda()
        mels = torch.randn(B, 80, T, generator=g).cuda()
        lens = torch.tensor(_bilstm_lengths(B, T_in)).cuda()
        a = _dec_run(dec, mem0, mels, lens, 'launch-per-step')
        b = _dec_run(dec, mem0, mels, lens, 'default')
        nfull, tail = B // 16, B % 16
        assert a[0] == ['k_lstm_fwd256 + k_attn_fwd'] * ((B + 15) // 16), a[0]
        assert a[1] == ['k_lstm_bwd256 + k_attn_cell_bwd'] * ((B + 15) // 16), a[1]
        exp_f = ['k_dec_train_persist16'] * nfull + (['k_dec_train_persist'] if 0 < tail <= 6 else [])
        exp_b = ['k_bwd_persist16'] * nfull + (['k_achain_bwd'] if 0 < tail <= 6 else [])
        assert b[0] == exp_f and b[1] == exp_b, (b[0], b[1])
        for i, name in ((2, 'mel'), (3, 'gate'), (4, 'alignments')):
            d = (a[i] - b[i]).abs()
            assert d.max().item() < 1e-2 * max(1.0, a[i].abs().max().item()) and d.mean().item() < 3e-4, (name, d.max().item(), d.mean().item())
        gmax = max(v.abs().max().item() for v in a[5].values())
        for n in a[5]:
            scale = a[5][n].abs().max().item()
            d = (a[5][n] - b[5][n]).abs().max().item()
            assert d < 3e-2 * scale + 1e-3 * gmax + 1e-7, (n, d, scale, gmax)
    finally:
        M.drop_rate, H.DecoderCore.persistent, H.DecoderCore.persistent16, H.DecoderCore.persistent_bwd = old[:4]
        H.set_bf16(old[4])


# ---------------------------------------------------------------------------------------------------- whole step at B = 64
def _b64_lengths():
    B, T_in, T = 64, 84, 160
    lens_in = [max(1, int(round(T_in * (1.0 - i / B) ** 2))) for i in range(B)]       # 84 .. 47 | 46 .. 21 | .. | 1
    lens_out = [max(2, T - 2 * i - (i % 3)) for i in range(B)]
    return B, T_in, T, lens_in, lens_out


def test_whole_step_b64_both_builds_against_the_cpu_oracle():
    """The reference's batch_size = 64 at T_in = 84, T_out = 160, ragged descending lengths (text lengths 84 .. 1, items of
    length 1; the later chunks' longest items far below the padded length), dropout off, injected eps: ONE run of the CPU oracle
    (<= 16 threads) and BOTH builds compared with it directly.
    fp32 build — the encoder conv bank on the x3 kernels (256 tiles), four launch-per-step decoder chunks in both passes, four
    GRU / BiLSTM chunks: the koemo bounds (mel-L1 < 1e-4, alignments 5e-5, gradients within 3e-3 of each tensor's norm).
    bf16_run build — four k_dec_train_persist16 / k_bwd_persist16 chunks: the bounds and error model of
    test_config5_shape_both_builds_against_the_cpu_oracle (mel-L1 < 2e-2; decoder tensors norm within 1 %, cosine >= 0.999;
    other tensors 3 % / 0.995, 0.99 upstream of the encoder's BatchNorm layers).
    Both builds: every BatchNorm layer's running mean / variance after the step == 0.9 * init + 0.1 * the oracle's batch
    statistic (unbiased variance), within 8e-4 (fp32) or 2e-2 (bf16, the products' 2^-8) of the channel's scale sqrt(mu^2 + var)
    resp. its second moment mu^2 + var.  fp32 error model: a BatchNorm input element may be off by the fp32-class conv bound,
    2e-7 * sqrt(5 * 512) = 1e-5 of sum |w||x|, which is ~40 times the channel's spread here, so 4e-4 of the scale; where those
    errors are all alike — the padded text positions, two thirds of the batch, all hold the same symbol and so the same conv
    output — they do not average out, and the variance moves by up to twice that (measured: 2.5e-4 on the first encoder layer,
    <= 1e-5 on every other layer)."""
    import hparams as HP
    import model as M
    import t2v_hip
    import t2v_oracle as O
    import train as TR
    sys.path.insert(0, ROOT)
    from bench import synthetic_batch
    B, T_in, T, lens_in, lens_out = _b64_lengths()
    batch = synthetic_batch(B, T_in, T, 77, lens_in=lens_in, lens_out=lens_out)
    eps = torch.randn(B, 32, generator=torch.Generator().manual_seed(5))
    lib = t2v_hip.load_library()
    old = M.drop_rate
    M.drop_rate = 0.0
    try:
        res = {}
        sd = None
        for mode in ('fp32', 'bf16'):
            hp = HP.create_hparams("batch_size=64,anneal_function=constant,p_attention_dropout=0.0,p_decoder_dropout=0.0,"
                                   "bf16_run=%s" % (mode == 'bf16'))
            torch.manual_seed(hp.seed)
            eng = TR.TrainEngine(hp, graph=False)
            eng.model.vae_gst.eps_override = eps.cuda()
            if sd is None:
                sd = {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}
            eng.optimizer.zero_grad()
            x, y = eng.model.parse_batch(batch)
            y_pred = eng.model(x)
            fwd_k = list(t2v_hip.DecoderCore.chunk_kernels)
            loss = eng.criterion(y_pred, y, 0)[0]
            loss.backward()
            torch.cuda.synchronize()
            t2v_hip.check_async_errors()
            res[mode] = dict(loss=float(loss), out=[t.detach().float().cpu() for t in y_pred[:4]],
                             grads={n: p.grad.detach().float().cpu().clone() for n, p in eng.model.named_parameters() if p.grad is not None},
                             kernels=(fwd_k, list(t2v_hip.DecoderCore.chunk_bwd_kernels)),
                             x3=lib.t2v_conv1d_takes_x3(B, 512, T_in, 512, 5, int(mode == 'bf16')),
                             running={k: v.detach().double().cpu() for k, v in eng.model.state_dict().items() if 'running_' in k})
            eng.close()
            del eng, y_pred, loss
        assert res['fp32']['kernels'] == (['k_lstm_fwd256 + k_attn_fwd'] * 4, ['k_lstm_bwd256 + k_attn_cell_bwd'] * 4), res['fp32']['kernels']
        assert res['bf16']['kernels'] == (['k_dec_train_persist16'] * 4, ['k_bwd_persist16'] * 4), res['bf16']['kernels']
        assert res['fp32']['x3'] == 1 and res['bf16']['x3'] == 1
        # ---- the oracle, once
        nthreads = torch.get_num_threads()
        torch.set_num_threads(max(1, min(16, nthreads)))
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and 'running_' not in k}
        osd = dict(sd)
        osd.update(leaves)
        text, lin, mel, gate, lout = batch[0].long(), batch[1].long(), batch[2].float(), batch[3].float(), batch[4].long()
        stats = {}
        o = O.tacotron2_forward(osd, text, lin, mel, lout, training=True, eps=eps, bn_stats=stats)
        o_loss = O.loss_forward(o, mel, gate, 0, anneal_function='constant')[0]
        o_loss.backward()
        torch.set_num_threads(nthreads)
        ref = {k: v.grad for k, v in leaves.items() if v.grad is not None}
        gmax = max(float(v.norm()) for v in ref.values())
        # ---- BatchNorm running statistics, both builds
        assert len(stats) == 3 + 6 + 5
        bad = []
        for mode, tol in (('fp32', 8e-4), ('bf16', 2e-2)):
            run = res[mode]['running']
            for prefix, (mu, var) in stats.items():
                mu, var = mu.double(), var.double()
                m2 = mu * mu + var
                exp_m = 0.9 * sd[prefix + '.running_mean'].double() + 0.1 * mu
                exp_v = 0.9 * sd[prefix + '.running_var'].double() + 0.1 * var
                dv = run[prefix + '.running_var'] - exp_v
                e_m = ((run[prefix + '.running_mean'] - exp_m).abs() / (0.1 * m2.sqrt() + 1e-12)).max().item()
                e_v = (dv.abs() / (0.1 * m2 + 1e-12)).max().item()
                print('%s %s running mean / var error %.2e / %.2e (var: mean ratio to 0.1*var %.2e, std %.2e)' % (
                    mode, prefix, e_m, e_v, (dv / (0.1 * var)).mean().item(), (dv / (0.1 * var)).std().item()))
                if not (e_m < tol and e_v < tol):
                    bad.append((mode, prefix, e_m, e_v))
        assert not bad, bad
        # ---- fp32 build: the fp32 bounds
        r = res['fp32']
        assert abs(r['loss'] - float(o_loss)) < 1e-4 * abs(float(o_loss))
        assert (r['out'][0] - o[0].detach()).abs().mean().item() < 1e-4           # mel-L1 (BASELINE.json)
        assert (r['out'][1] - o[1].detach()).abs().mean().item() < 1e-4
        assert (r['out'][3] - o[3].detach()).abs().max().item() < 5e-5            # alignments
        checked = 0
        for n, g in r['grads'].items():
            if n not in ref:
                continue
            if n.endswith('conv.bias') and 'convolutions' in n:
                # a conv bias in front of a training-mode BatchNorm has an exactly zero gradient: the kernels write zeros, the
                # oracle's fp32 autograd leaves round-off (at B = 64: a norm of ~2e-6 of the largest gradient norm)
                assert float(g.abs().max()) == 0.0 and float(ref[n].norm()) < 1e-5 * gmax, ('fp32 build', n)
                checked += 1
                continue
            scale = max(float(ref[n].norm()), 1e-4 * gmax)
            assert float((g - ref[n]).norm()) < 3e-3 * scale, ('fp32 build', n)
            checked += 1
        assert checked >= 90
        # ---- bf16 build: the stated bf16 bounds, against the oracle
        r = res['bf16']
        d_mel = (r['out'][0] - o[0].detach()).abs().mean().item()
        d_post = (r['out'][1] - o[1].detach()).abs().mean().item()
        assert d_mel < 2e-2 and d_post < 2e-2, (d_mel, d_post)
        assert (r['out'][3] - o[3].detach()).abs().max().item() < 2e-2
        assert abs(r['loss'] - float(o_loss)) < 2e-2 * abs(float(o_loss))
        for n, g in r['grads'].items():
            if n not in ref or float(ref[n].norm()) < 1e-4 * gmax:
                continue
            g64, r64 = g.double(), ref[n].double()
            rel = abs(float(g64.norm() / r64.norm()) - 1.0)
            cos = float((g64 * r64).sum() / (g64.norm() * r64.norm()))
            if n.startswith('decoder.'):
                assert rel < 1e-2 and cos > 0.999, ('bf16 build, decoder tensor', n, rel, cos)
            else:
                assert rel < 3e-2, ('bf16 build', n, rel)
                upstream = n.startswith('transcript_embedding') or ('convolutions' in n and n.startswith('encoder.'))
                assert cos > (0.99 if upstream or ('.bias' in n and 'convolutions' in n) else 0.995), ('bf16 build', n, cos)
    finally:
        M.drop_rate = old
        t2v_hip.set_bf16(False)


# ------------------------------------------------------------------------------------------------- remaining large-batch edges
def _coord_channels(B, H, W):
    """CoordConv.py (with_r): xx along H, yy along W in [-1, 1], rr = sqrt((xx-.5)^2 + (yy-.5)^2)"""
    xx = (torch.arange(H, dtype=torch.float32) / (H - 1) * 2 - 1).view(1, 1, H, 1).expand(B, 1, H, W)
    yy = (torch.arange(W, dtype=torch.float32) / (W - 1) * 2 - 1).view(1, 1, 1, W).expand(B, 1, H, W)
    rr = torch.sqrt((xx - 0.5) ** 2 + (yy - 0.5) ** 2)
    return torch.cat([xx, yy, rr], 1)


@pytest.mark.parametrize("gemm_form", [True, False])
@pytest.mark.parametrize("B,Cx,H,W,Cout,coord", [(64, 1, 800, 80, 32, True), (64, 32, 400, 40, 32, False)])
def test_conv2d_s2_bn_relu_b64_matches_fp64(B, Cx, H, W, Cout, coord, gemm_form):
    """The reference encoder's first two layers at B = 64 (T_out = 800 frames), both forms (im2col + batched GEMM / direct).
    Reference: fp64 torch on the CPU.  Bounds of test_conv2d_s2_bn_relu_matches_torch: output 2e-5 of its scale, running
    statistics 1e-5 / 1e-4, gradients 3e-4 of each tensor's largest entry (+ 2e-7); the reference's ReLU takes the kernel's
    side only where z is within round-off of 0.  Path: t2v_hip.CONV2D_GEMM as set."""
    import t2v_hip
    g = torch.Generator().manual_seed(B * 1000 + H + Cout)
    Cin = Cx + (3 if coord else 0)
    x = torch.randn(B, Cx, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (Cin * 9) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    wo = torch.randn(B, Cout, Ho, Wo, generator=g)
    old = t2v_hip.CONV2D_GEMM
    t2v_hip.CONV2D_GEMM = gemm_form
    try:
        dev = [t.clone().cuda().requires_grad_(True) for t in (x, w, b, gamma, beta)]
        drm, drv = torch.zeros(Cout, device='cuda'), torch.ones(Cout, device='cuda')
        out = t2v_hip.Conv2dBNReLU.apply(dev[0], dev[1], dev[2], dev[3], dev[4], drm, drv, True, coord)
        assert t2v_hip.CONV2D_GEMM == gemm_form
        (out * wo.cuda()).sum().backward()
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
    finally:
        t2v_hip.CONV2D_GEMM = old
    ref = [t.clone().double().requires_grad_(True) for t in (x, w, b, gamma, beta)]
    xin = torch.cat([ref[0], _coord_channels(B, H, W).double()], 1) if coord else ref[0]
    rm, rv = torch.zeros(Cout, dtype=torch.float64), torch.ones(Cout, dtype=torch.float64)
    zr = F.batch_norm(F.conv2d(xin, ref[1], ref[2], stride=2, padding=1), rm, rv, ref[3], ref[4], True, 0.1, 1e-5)
    # ReLU'(z) at z = 0 is a coin toss between fp32 and fp64: among 8 M values a few land within round-off of 0 and take the other
    # side (measured: one element's whole dout moved into dbeta and its 3x3 footprint of dX).  The reference takes the kernel's
    # side there — and only there: a disagreement is allowed where |z| is within fp32 round-off of 0
    keep = out.detach().cpu() > 0
    flip = keep != (zr.detach() > 0)
    assert (zr.detach().abs()[flip] < 1e-5 * max(1.0, zr.detach().abs().max().item())).all()
    y = zr * keep.double()
    (y * wo.double()).sum().backward()
    assert (out.cpu().double() - y).abs().max().item() < 2e-5 * max(1.0, y.abs().max().item())
    assert (drm.cpu().double() - rm).abs().max().item() < 1e-5 and (drv.cpu().double() - rv).abs().max().item() < 1e-4
    for name, r, d in zip(('x', 'weight', 'bias', 'gamma', 'beta'), ref, dev):
        if name == 'bias':
            continue
        scale = max(r.grad.abs().max().item(), 1e-6)
        assert (d.grad.cpu().double() - r.grad).abs().max().item() < 3e-4 * scale + 2e-7, name


def test_fused_loss_and_mask_outputs_b64_t1200():
    """VAELoss (one launch: both MSEs, the gate BCE, KL) and mask_outputs at B = 64, T = 1200 (6.1 M mel values per tensor).
    Reference: the oracle's loss_forward in float64 on the CPU and masked_fill; bounds of test_fused_loss_matches_oracle
    (values 1e-5 relative, gradients 1e-5 of the largest entry) and bit-equality for the masks."""
    import hparams as HP
    import t2v_hip as H
    import t2v_oracle as O
    from loss_function import Tacotron2Loss_VAE
    g = torch.Generator().manual_seed(64)
    B, T = 64, 1200
    lens = torch.tensor([max(1, T - 19 * i) for i in range(B)])
    mel, post = torch.randn(B, 80, T, generator=g), torch.randn(B, 80, T, generator=g)
    gate = torch.randn(B, T, generator=g) * 3
    pad = torch.arange(T)[None, :] >= lens[:, None]
    m_ref = (mel.masked_fill(pad[:, None, :], 0.0), post.masked_fill(pad[:, None, :], 0.0), gate.masked_fill(pad, 1e3))
    dm, dp, dg = mel.cuda(), post.cuda(), gate.cuda()
    H.mask_outputs(dm, dp, dg, lens.to(device='cuda', dtype=torch.int32))
    torch.cuda.synchronize()
    for a, r in zip((dm, dp, dg), m_ref):
        assert torch.equal(a.cpu(), r)
    mu, logvar = torch.randn(B, 32, generator=g), torch.randn(B, 32, generator=g) * 0.3
    mel_t, gate_t = torch.randn(B, 80, T, generator=g), (torch.rand(B, T, generator=g) > 0.9).float()
    cpu = [t.clone().double().requires_grad_(True) for t in (m_ref[0], m_ref[1], m_ref[2], mu, logvar)]
    ref = O.loss_forward([cpu[0], cpu[1], cpu[2], None, cpu[3], cpu[4]], mel_t.double(), gate_t.double(), 20000, 'logistic')
    ref[0].backward()
    dev = [t.clone().cuda().requires_grad_(True) for t in (m_ref[0], m_ref[1], m_ref[2], mu, logvar)]
    crit = Tacotron2Loss_VAE(HP.create_hparams("anneal_function=logistic"))
    out = crit([dev[0], dev[1], dev[2], None, dev[3], dev[4]], (mel_t.cuda(), gate_t.cuda()), 20000)
    out[0].backward()
    torch.cuda.synchronize()
    for a, b in zip(out[:3], ref[:3]):
        assert abs(float(a) - float(b)) < 1e-5 * abs(float(b)) + 1e-6
    for d, c in zip(dev, cpu):
        assert (d.grad.cpu().double() - c.grad).abs().max().item() < 1e-5 * c.grad.abs().max().item() + 1e-9


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M,N,K", [(76800, 256, 80), (76800, 80, 1536), (256, 80, 76800), (80, 1536, 76800)])
def test_gemm_at_b64_row_counts(M, N, K, bf16):
    """gemm at the B*T = 64 * 1200 = 76 800 rows of the Prenet (80 -> 256), the projection (1536 -> 80) and their weight
    gradients (K = 76 800), past the fuzz slice's 6 400.  Reference: the float64 product on the GPU.  fp32 (x3 products): the
    bound of test_gemm_forms, 2e-5 * sqrt(K) of the largest entry; bf16_run: the fp64 product of the bf16-rounded operands
    within 2e-3 (test_gemm_bf16) — or, where the skinny deep-K product stays on the fp32 split-K kernel, the fp32 bound.
    Path: t2v_gemm_f32_set_mode(-1) == 1 (x3) for fp32, bf16_enabled() for bf16."""
    import t2v_hip
    lib = t2v_hip.load_library()
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).cuda()
    Bm = torch.randn(N, K, generator=g).cuda()
    if K == 76800:              # weight gradients: dY^T . X — both operands given as transposed views
        A = torch.randn(K, M, generator=g).cuda().t()
        Bm = torch.randn(K, N, generator=g).cuda().t()
    bias = torch.randn(N, generator=g).cuda()
    t2v_hip.set_bf16(bf16)
    try:
        assert t2v_hip.bf16_enabled() == bf16
        if not bf16:
            assert lib.t2v_gemm_f32_set_mode(-1) == 1
        out = t2v_hip.gemm(A, Bm, bias)
        torch.cuda.synchronize()
    finally:
        t2v_hip.set_bf16(False)
    full = A.double() @ Bm.double().t() + bias.double()
    skinny = lib.t2v_gemm_splitk_scratch_floats(M, N, K) > 0 and ((M + 63) // 64) * ((N + 63) // 64) < 64
    if bf16 and not skinny:
        ref = A.bfloat16().double() @ Bm.bfloat16().double().t() + bias.double()
        assert (out.double() - ref).abs().max().item() < 2e-3 * ref.abs().max().item()
    else:
        assert (out.double() - full).abs().max().item() < 2e-5 * K ** 0.5 * full.abs().max().item()
