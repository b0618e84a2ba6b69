"""Guided attention loss on the GPU: the kernel against tests/guided_ref.py, the criterion switch, one full training step against
the CPU oracle with the term in the loss, and the captured step against the eager one.

Bounds of the kernel test.  G * D against W_ref: expf costs about 2 ulp of a value <= 1, the subtraction from 1 half an ulp, the
fp32 argument x contributes at most x e^-x (<= 0.37) times a few ulp, the scaling by D half an ulp: 8 * 2^-24 elementwise.  L: the
rows of A sum to 1, so sum_b T_b / D bounds L, and its terms carry the relative error of W: 16 * 2^-24 * sum_b T_b / D (the fp64
accumulation adds nothing visible)."""
import os
import sys

import pytest
import torch

import guided_ref as G

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24


def _align(B, T, T_in, in_lengths, seed, layout):
    """random row-stochastic alignments, masked like the decoder's (0 past an item's length); layout 'contiguous' or 'arena':
    the (B, T, T_in) view of rows 1.. of a (T + 1, B, T_in) arena that model(x)[3] is"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(B, T, T_in, generator=g)
    for b, n in enumerate(in_lengths):
        e[b, :, n:] = float('-inf')
    a = torch.softmax(e, -1)
    if layout == 'contiguous':
        return a.cuda()
    arena = torch.full((T + 1, B, T_in), 9.0, device='cuda')
    arena[1:] = a.permute(1, 0, 2).cuda()
    view = arena[1:].permute(1, 0, 2)
    assert not view.is_contiguous() and torch.equal(view.cpu(), a)
    return view


KERNEL_CASES = [(3, 7, 21, (21, 10, 1), (7, 4, 1), 'contiguous'),
                (2, 5, 225, (225, 130), (5, 3), 'contiguous'),              # rows wider than a workgroup
                (3, 7, 21, (21, 10, 1), (7, 4, 1), 'arena')]


@pytest.mark.parametrize("B,T,T_in,n_in,n_out,layout", KERNEL_CASES, ids=['B3-T7-Tin21', 'B2-T5-Tin225', 'B3-T7-Tin21-arena'])
@pytest.mark.parametrize("sigma", [0.4, 0.2])
def test_kernel_matches_reference(B, T, T_in, n_in, n_out, layout, sigma):
    import t2v_hip
    a = _align(B, T, T_in, n_in, 3, layout)
    lin, lout = torch.tensor(n_in).cuda(), torch.tensor(n_out).cuda()
    L, Gd = t2v_hip.guided_attention(a, lin, lout, sigma)
    L2, Gd2 = t2v_hip.guided_attention(a, lin, lout, sigma)
    torch.cuda.synchronize()
    assert Gd.shape == (B, T, T_in) and Gd.permute(1, 0, 2).is_contiguous() and L.shape == ()
    D = G.denominator(n_in, n_out)
    w_ref = G.weights(n_in, n_out, T, T_in, sigma)
    err_g = (Gd.cpu().double() * D - w_ref).abs().max().item()
    l_ref = G.loss(a.cpu(), n_in, n_out, sigma).item()
    err_l, bound_l = abs(L.item() - l_ref), 16 * ULP * sum(n_out) / D
    print('guided kernel B%d T%d Tin%d sigma %.1f %s: |G D - W| %.2e bound %.2e   |L - L_ref| %.2e bound %.2e   L %.6f'
          % (B, T, T_in, sigma, layout, err_g, 8 * ULP, err_l, bound_l, l_ref))
    assert err_g <= 8 * ULP
    for b in range(B):
        assert Gd[b, n_out[b]:].abs().max().item() == 0.0 if n_out[b] < T else True
        assert Gd[b, :, n_in[b]:].abs().max().item() == 0.0 if n_in[b] < T_in else True
    assert (w_ref == 0).sum() == (Gd == 0).sum().item()
    assert err_l <= bound_l
    assert torch.equal(L, L2) and torch.equal(Gd, Gd2)                  # the same bits from call to call


def test_autograd_function_scales_the_gradient():
    import t2v_hip
    n_in, n_out = (21, 10, 1), (7, 4, 1)
    a = _align(3, 7, 21, n_in, 4, 'arena').requires_grad_(True)
    lin, lout = torch.tensor(n_in).cuda(), torch.tensor(n_out).cuda()
    L = t2v_hip.GuidedAttention.apply(a, lin, lout, 0.4)
    g, = torch.autograd.grad(2.5 * L, a)
    _, Gd = t2v_hip.guided_attention(a.detach(), lin, lout, 0.4)
    assert torch.equal(g, 2.5 * Gd) and g.permute(1, 0, 2).is_contiguous()


# ------------------------------------------------------------------------------------------------ criterion
def _model_output(seed=0):
    g = torch.Generator().manual_seed(seed)
    B, T, T_in = 3, 7, 21
    mel, post = torch.randn(B, 80, T, generator=g).cuda(), torch.randn(B, 80, T, generator=g).cuda()
    gate, mu, logvar = torch.randn(B, T, generator=g).cuda(), torch.randn(B, 32, generator=g).cuda(), torch.randn(B, 32, generator=g).cuda()
    align = _align(B, T, T_in, (21, 10, 1), 5, 'arena')
    targets = (torch.randn(B, 80, T, generator=g).cuda(), torch.rand(B, T, generator=g).round().cuda())
    lengths = (torch.tensor([21, 10, 1]).cuda(), torch.tensor([7, 4, 1]).cuda())
    return [mel, post, gate, align, mu, logvar], targets, lengths


def test_criterion_weight_zero_launches_nothing_new(monkeypatch):
    import hparams as HP
    import loss_function as LF
    import t2v_hip
    calls = []
    lib = t2v_hip.load_library()
    real = lib.t2v_guided_attention
    monkeypatch.setattr(lib, 't2v_guided_attention', lambda *a: calls.append(1) or real(*a))
    out, targets, lengths = _model_output()

    class ReferenceHParams(object):         # the reference's own set: no guided_attention_* at all
        pass
    ref_hp = ReferenceHParams()
    for k, v in HP.create_hparams("anneal_function=constant").values().items():
        setattr(ref_hp, k, v)
    assert not hasattr(ref_hp, 'guided_attention_weight')
    base = LF.Tacotron2Loss_VAE(ref_hp)(out, targets, 0)
    off = LF.Tacotron2Loss_VAE(HP.create_hparams("anneal_function=constant"))
    for got in (off(out, targets, 0), off(out, targets, 0, lengths=lengths)):
        assert len(got) == 4 and all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(got, base))
    assert not calls and off.guided is None
    on = LF.Tacotron2Loss_VAE(HP.create_hparams("anneal_function=constant,guided_attention_weight=1.5"))
    total, recon, kl, w = on(out, targets, 0, lengths=lengths)
    torch.cuda.synchronize()
    assert len(calls) == 1 and on.guided is not None and not on.guided.requires_grad
    want = base[0].double().item() + 1.5 * on.guided.double().item()
    assert abs(total.item() - want) <= ULP * 2 * abs(want), (total.item(), want)            # one fp32 rounding
    assert torch.equal(recon, base[1]) and torch.equal(kl, base[2]) and w == base[3]
    assert abs(on.guided.item() - G.loss(out[3].cpu(), (21, 10, 1), (7, 4, 1)).item()) <= 16 * ULP * 12 / 248
    with pytest.raises(ValueError):
        on(out, targets, 0)
    # validation: under no_grad the term is left out, lengths given or not needed for nothing
    with torch.no_grad():
        val = on(out, targets, 0, lengths=lengths)
    assert len(calls) == 1 and torch.equal(val[0], base[0])


# ------------------------------------------------------------------------------------------------ full step against the oracle
def test_full_step_with_guided_attention_matches_oracle():
    """test_koemo_shape_parity_against_oracle's procedure and tolerances at B = 3, (T_in, T_out) = (30, 48), (22, 40), (17, 31),
    guided_attention_weight = 1.0; the oracle's loss is extended by guided_ref on its alignments"""
    import hparams as HP
    import model as M
    import t2v_oracle as O
    import train as TR
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synthetic_batch
    lens_in, lens_out = [30, 22, 17], [48, 40, 31]
    old = M.drop_rate
    M.drop_rate = 0.0
    try:
        hp = HP.create_hparams("batch_size=3,anneal_function=constant,p_attention_dropout=0.0,p_decoder_dropout=0.0,"
                               "guided_attention_weight=1.0")
        torch.manual_seed(hp.seed)
        eng = TR.TrainEngine(hp)
        batch = synthetic_batch(3, 30, 48, 77, lens_in=lens_in, lens_out=lens_out)
        eps = torch.randn(3, hp.z_latent_dim, generator=torch.Generator().manual_seed(5))
        eng.model.vae_gst.eps_override = eps.cuda()
        sd = {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}
        eng.optimizer.zero_grad()
        x, y = eng.model.parse_batch(batch)
        y_pred = eng.model(x)
        loss = eng.criterion(y_pred, y, 0, lengths=(x[1], x[4]))[0]
        loss.backward()
        torch.cuda.synchronize()
        import t2v_hip
        t2v_hip.check_async_errors()
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and 'running_' not in k}
        osd = dict(sd)
        osd.update(leaves)
        text, lin, mel, gate, lout = batch[0].long(), batch[1].long(), batch[2].float(), batch[3].float(), batch[4].long()
        o = O.tacotron2_forward(osd, text, lin, mel, lout, training=True, eps=eps)
        o_guided = G.loss(o[3], lens_in, lens_out, 0.4)
        o_loss = O.loss_forward(o, mel, gate, 0, anneal_function='constant')[0] + 1.0 * o_guided
        o_loss.backward()
        print('full step with guided attention: loss %.6f oracle %.6f, guided %.6f oracle %.6f'
              % (float(loss), float(o_loss), float(eng.criterion.guided), float(o_guided)))
        assert abs(float(loss) - float(o_loss)) < 1e-4 * abs(float(o_loss))
        assert abs(float(eng.criterion.guided) - float(o_guided)) < 1e-4 * abs(float(o_guided))
        assert (y_pred[3].detach().cpu() - o[3].detach()).abs().max().item() < 5e-5           # alignments
        gmax = max(float(v.grad.norm()) for v in leaves.values() if v.grad is not None)
        checked = 0
        for name, p in eng.model.named_parameters():
            ref = leaves[name].grad if name in leaves else None
            if ref is None or p.grad is None:
                continue
            scale = max(float(ref.norm()), 1e-4 * gmax)
            assert float((p.grad.cpu() - ref).norm()) < 3e-3 * scale, name
            checked += 1
        assert checked >= 90
    finally:
        M.drop_rate = old


# ------------------------------------------------------------------------------------------------ graph equals eager
def test_graph_replay_equals_eager_training_with_guided_attention():
    """test_graph_replay_equals_eager_training's procedure with guided_attention_weight = 1.0: losses, gradient norms, the guided
    term and the arena after six steps are the same bits, one graph in graph mode, and the guided term differs from step to step"""
    import hparams as HP
    import train as TR
    import t2v_hip
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from bench import synthetic_batch
    batches = [synthetic_batch(3, 30, 48, 5, lens_in=[30, 22, 17], lens_out=[48, 40, 31]),
               synthetic_batch(3, 30, 48, 6, lens_in=[30, 25, 11], lens_out=[48, 37, 20])]
    runs = {}
    for mode in ('eager', 'graph'):
        hp = HP.create_hparams("batch_size=3,anneal_function=logistic,graph_step=%s,guided_attention_weight=1.0" % (mode == 'graph'))
        torch.manual_seed(hp.seed)
        torch.cuda.manual_seed(hp.seed)
        eng = TR.TrainEngine(hp)
        eng.model.overlap_branches = False
        eng.model.vae_gst.eps_override = torch.full((3, 32), 0.25, device='cuda')
        vals = []
        for it in range(6):
            loss, recon, kl, w, gn = eng.step(batches[it % 2], 1000 * it)
            vals.append((float(loss), float(kl), float(w), float(gn), float(eng.criterion.guided)))
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
        assert (mode == 'graph') == (len(eng._graphs) == 1)
        runs[mode] = (vals, eng.optimizer.params.clone(), eng.optimizer.step_count)
    assert runs['eager'][2] == runs['graph'][2] == 6
    assert runs['eager'][0] == runs['graph'][0], (runs['eager'][0], runs['graph'][0])
    assert torch.equal(runs['eager'][1], runs['graph'][1])
    gs = [v[4] for v in runs['graph'][0]]
    assert len(set(gs)) == 6 and all(0.0 < g < 1.0 for g in gs), gs
