"""Decoder attention on steered alignments against the fp64 oracle, at round-off scale.

tests/steer_ref.py puts probability mass on both sides of every position at which a kernel cuts T_in (16, 32, 96, 128, 192, 288,
384, 480, 512) and multiplies the location term by 60, so that the halo of the 31-tap location filter carries weight across
every cut; tests/test_steer_ref.py shows on the reference alone that one halo tap lost at a cut then stands thousands of fp32
round-offs above the fp32 round-off.  Here the HIP decoder runs on those inputs:

(a) teacher-forced forward and every gradient, on each engine pair a shape qualifies for (persistent forward + one-launch reverse
    pass; launch-per-step forward + launch-per-step reverse; launch-per-step forward + one-launch reverse pass at 561..576);
(b) the comparison of (a) against an oracle that loses one halo tap at a cut, in the forward pass or in the reverse pass alone,
    must FAIL — nothing in the kernels is altered, the device results of (a) are reused;
(c) free-running decode, 6 frames, launch-per-stage and default (persistent for B <= 4, T_in <= 224) paths.

Bounds.  floor = fp32 oracle minus fp64 oracle, per case and quantity (steer_ref.floor).  A quantity passes below
K * max(floor, 4 * 2^-24 * scale): scale = max |reference| for mel / gate / align; 1 for parameter gradients (each relative to its
tensor's largest reference entry) and d memory (each item relative to its largest entry), whose floors are relative already.  The
second leg keeps a floor that happens to cancel from setting the bound.  K = 16 for every quantity: the kernels' sigmoid / tanh
carry ~1e-7 absolute error (csrc/t2v_common.h) where libm carries half an ulp, and the fused 64-tap filter and the sliced softmax
sum in another order than the oracle.

Every case prints its worst values next to floor, K and bound before it asserts (pytest -s); profiles/steered_attention_parity.txt
is that table from an MI355X.  The bf16 engines are not covered here: the oracle has no bf16 form — they meet a step-by-step
rounding oracle (tests/bf16_ref.py) in test_decoder_bf16_stepwise_gpu.py.
"""
import pytest
import torch

import steer_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K = 16.0

# forward engine / reverse engine pairs (DecoderCore.persistent, .persistent_bwd, expected last_mode, last_bwd_mode)
ENGINES = {'persistent+achain': (True, True, 'persistent', 'persistent'),
           'launch-per-step+steps': (False, False, 'launch-per-step', 'launch-per-step'),
           'launch-per-step+achain': (False, True, 'launch-per-step', 'persistent')}


def _engines(case):
    B, T_in = case[:2]
    out = ['launch-per-step+steps']
    if B <= 6 and T_in <= 560:
        out.append('persistent+achain')             # the one-launch kernels' range
    if B <= 6 and 560 < T_in <= 576:
        out.append('launch-per-step+achain')        # the reverse pass reaches 16 positions further than the forward one
    return sorted(out)


PARITY = [(c, e) for c in S.CASES for e in _engines(c)]
MUTATIONS = [(kind, b, c, e) for b, c in S.MUTATION_CUTS for kind in ('fwd', 'bwd') for e in _engines(c)]
_MUTATED_CASES = {c for _, c in S.MUTATION_CUTS}


def _id(case):
    return 'B%d-Tin%d-T%d' % case[:3]


_DEVICE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    S.oracle.cache_clear()


def _device(case, engine, monkeypatch):
    """the HIP decoder on the steered inputs: (mel, gate, align, {parameter: gradient}, d memory) on the host.  Kept per
    (case, engine) for the cases that (b) looks at again."""
    if (case, engine) in _DEVICE:
        return _DEVICE[case, engine]
    import model as M
    import t2v_hip
    fwd, bwd, fwd_mode, bwd_mode = ENGINES[engine]
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent', fwd)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent_bwd', bwd)
    dec, memory, mels, lengths, wm, wg = S.inputs(case)
    dev = torch.device('cuda:0')
    dec = dec.to(dev).train()
    dec.p_attention_dropout = dec.p_decoder_dropout = 0.0
    dec._calls = 0
    mem = memory.to(dev).requires_grad_(True)
    mel, gate, align = dec(mem, mels.to(dev), lengths.to(dev))
    assert t2v_hip.DecoderCore.last_mode == fwd_mode
    ((mel * wm.to(dev)).sum() + (gate * wg.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert t2v_hip.DecoderCore.last_bwd_mode == bwd_mode
    assert all(p.grad is not None for p in dec.parameters())
    grads = {n: p.grad.cpu() for n, p in dec.named_parameters()}
    res = (mel.detach().cpu(), gate.detach().cpu(), align.detach().cpu(), grads, mem.grad.cpu())
    if case in _MUTATED_CASES:
        _DEVICE[case, engine] = res
    return res


def _judge(title, res, ref, floors):
    """prints one row per quantity; returns ({quantity: error / bound}, the rows over their bound)"""
    err, bound = S.compare(res, ref), S.bounds(floors, ref, K)
    ratio, failed = {}, []
    for q in S.QUANTITIES:
        if q not in err:
            continue
        e, where = err[q]
        row = '%s %-8s err %.2e floor %.2e K %g bound %.2e at %s' % (title, q, e, floors[q], K, bound[q], where)
        print(row)
        ratio[q] = e / bound[q]
        if not e < bound[q]:
            failed.append(row)
    return ratio, failed


# ------------------------------------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("case,engine", PARITY, ids=['%s-%s' % (_id(c), e) for c, e in PARITY])
def test_steered_decoder_matches_oracle(case, engine, monkeypatch):
    """mel, gate, align absolutely, every parameter gradient relative to its tensor's largest reference entry, d memory per item
    relative to the item's largest entry: each within 16 * max(floor, 4 * 2^-24 * scale) of the fp64 oracle"""
    ref = S.oracle(case, F64)
    floors = S.floor(case)
    res = _device(case, engine, monkeypatch)
    _, failed = _judge('steered parity %s %s' % (_id(case), engine), res, ref, floors)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ (b) the test sees a lost tap
@pytest.mark.parametrize("kind,b,case,engine", MUTATIONS, ids=['%s%d-%s-%s' % (k, b, _id(c), e) for k, b, c, e in MUTATIONS])
def test_a_lost_halo_tap_in_the_oracle_is_seen(kind, b, case, engine, monkeypatch):
    """CPU-side mutations of the REFERENCE: against an oracle in which input position b - 1 no longer reaches the location-conv
    outputs b .. b + 14 the unmutated kernels' alignments are over the bound of the parity test; against one that loses the same
    tap in the reverse pass alone the forward quantities still pass and the gradients are over the bound"""
    floors = S.floor(case)
    res = _device(case, engine, monkeypatch)
    ref = S.oracle(case, F64, (kind, b))
    ratio, _ = _judge('lost tap %s at %d, %s %s' % (kind, b, _id(case), engine), res, ref, floors)
    if kind == 'fwd':
        assert ratio['align'] > 1, ratio
    else:
        assert max(ratio['mel'], ratio['gate'], ratio['align']) < 1, ratio
        assert max(ratio['grad'], ratio['d_memory']) > 1, ratio


# ------------------------------------------------------------------------------------------------ (c) free-running decode
@pytest.mark.parametrize("T_in,B", S.DECODE_CASES)
def test_steered_decode_matches_oracle(T_in, B, monkeypatch):
    """Decoder.inference, gate ignored, 6 frames, on the launch-per-stage path and on the default one (one persistent launch
    for B <= 4, T_in <= 224): mel, gate, align within 16 * max(floor, 4 * 2^-24 * scale) of the fp64 oracle's free run"""
    import model as M
    import t2v_hip
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    calls = {'persistent': 0, 'stages': 0}
    for name, attr in (('persistent', 'run_persistent'), ('stages', 'run')):
        def counted(self, *a, _f=getattr(t2v_hip.InferenceSession, attr), _n=name, **kw):
            calls[_n] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(t2v_hip.InferenceSession, attr, counted)
    dec, memory = S.decode_inputs(T_in, B)
    dec = dec.cuda().eval()
    dec.gate_threshold = 1.0                                        # never stop: all 6 frames
    dec.max_decoder_steps = S.DECODE_FRAMES
    ref, floors = S.decode_oracle(T_in, B, F64), S.decode_floor(T_in, B)
    failed = []
    for path, persistent in (('launch-per-stage', False), ('default', None)):
        calls.update(persistent=0, stages=0)
        with torch.no_grad():
            mel, gate, align = dec.inference(memory.cuda(), persistent=persistent)
        torch.cuda.synchronize()
        t2v_hip.check_async_errors()
        one_launch = persistent is None and B <= 4 and T_in <= 224
        assert calls == ({'persistent': 1, 'stages': 0} if one_launch else {'persistent': 0, 'stages': 1}), (path, calls)
        assert mel.shape == (B, 80, S.DECODE_FRAMES)
        res = (mel.cpu(), gate.squeeze(-1).cpu(), align.cpu())
        title = 'steered decode T_in=%d B=%d %s path (%s)' % (T_in, B, path, 'one launch' if one_launch else 'launch per stage')
        failed += _judge(title, res, ref, floors)[1]
    assert not failed, failed
