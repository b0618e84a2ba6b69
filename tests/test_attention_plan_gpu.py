"""The planned free-running decode (Decoder.inference(plan=, n_plan=)) on the device against the planned fp64
reference of tests/plan_ref.py, on the steered inputs of tests/steer_ref.py, with plans that put the window on both sides of
every tile and chunk cut of the kernels.

Bounds: the rule of test_decoder_steered_gpu.py::test_steered_decode_matches_oracle.  floor = planned fp32 reference minus
planned fp64 reference per case and quantity; a quantity passes below 16 * max(floor, 4 * 2^-24 * max |reference|).  A plan is
data, so round-off cannot move a window and the rule carries over as it stands.  tests/test_attention_plan.py asserts, on the
reference alone, that a plan shifted by one frame or one symbol, or a window one position wider, moves `align` by at least
1000 such bounds on every case.

Both decode paths, as in test_attention_window_gpu.py: the T_in = 224, B = 4 group does not fit the persistent launch and runs
the launch-per-stage loop on both.  Every case prints its figures before it asserts (pytest -s).
"""
import copy

import pytest
import torch

import plan_ref as P
import steer_ref as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K = 16.0
PATHS = (('launch-per-stage', False), ('default', None))
IDS = [P.case_id(c) for c in P.CASES]
_DEVICE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    P.reference.cache_clear()
    P.inputs.cache_clear()


@pytest.fixture()
def calls(monkeypatch):
    """Prenet dropout off; counts InferenceSession.run_persistent / .run calls"""
    import model as M
    import t2v_hip
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    n = {'persistent': 0, 'stages': 0}
    for name, attr in (('persistent', 'run_persistent'), ('stages', 'run')):
        def counted(self, *a, _f=getattr(t2v_hip.InferenceSession, attr), _n=name, **kw):
            n[_n] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(t2v_hip.InferenceSession, attr, counted)
    return n


def _decoder(case, frames=None):
    T_in, lens = case[0], case[1]
    dec, memory = P.inputs(T_in, lens)
    dec = copy.deepcopy(dec).cuda().eval()                 # (the cached CPU decoder stays where the references read it)
    dec.gate_threshold = 1.0                               # never stop: all frames
    dec.max_decoder_steps = case[3] if frames is None else frames
    return dec, memory.cuda()


def _plan(case):
    return torch.tensor(case[4], dtype=torch.int32).cuda(), torch.tensor(case[5], dtype=torch.int32).cuda()


def _decode(case, persistent, calls, chunk=32):
    """(mel (B, 80, frames), gate (B, frames), align (B, frames, T_in)) on the host under the case's plan and window, with
    plan_stop = 'gate' and a gate that never fires: all `frames` frames, past n_plan too (the plan holds its last symbol).
    inference_batch for ragged lengths, inference for full-length items; asserts which decode loop ran."""
    import t2v_hip
    T_in, lens, win, frames = case[:4]
    dec, memory = _decoder(case)
    plan, n_plan = _plan(case)
    calls.update(persistent=0, stages=0)
    kw = dict(plan=plan, n_plan=n_plan, plan_window=win, plan_stop='gate', persistent=persistent, chunk=chunk)
    with torch.no_grad():
        if any(n != T_in for n in lens):
            mel, gate, align, n_frames = dec.inference_batch(memory, lens, **kw)
            assert n_frames.tolist() == [frames] * len(lens)
        else:
            mel, gate, align = dec.inference(memory, **kw)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    one_launch = persistent is None and P.persistent_fits(len(lens), T_in)
    n_runs = (frames + chunk - 1) // chunk
    assert calls == ({'persistent': 1, 'stages': 0} if one_launch else {'persistent': 0, 'stages': n_runs}), (P.case_id(case), calls)
    assert mel.shape == (len(lens), 80, frames) and align.shape == (len(lens), frames, T_in)
    return mel.cpu(), gate.squeeze(-1).cpu(), align.cpu()


def _device(case, path, calls):
    """the planned device result of (case, path), decoded once per module"""
    if (case, path) not in _DEVICE:
        _DEVICE[case, path] = _decode(case, dict(PATHS)[path], calls)
    return _DEVICE[case, path]


def _judge(title, res, ref, floors):
    """prints one row per quantity; returns ({quantity: error / bound}, the rows over their bound)"""
    err, bound = S.compare(res, ref), S.bounds(floors, ref, K)
    ratio, failed = {}, []
    for q in ('mel', 'gate', 'align'):
        e, where = err[q]
        row = '%s %-5s err %.2e floor %.2e K %g bound %.2e at %s' % (title, q, e, floors[q], K, bound[q], where)
        print(row)
        ratio[q] = e / bound[q]
        if not e < bound[q]:
            failed.append(row)
    return ratio, failed


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_planned_decode_matches_the_planned_oracle(case, calls):
    """mel, gate and align of both decode paths within 16 * max(floor, 4 * 2^-24 * scale) of the planned fp64 reference"""
    ref, floors = P.reference(case, F64)[:3], P.floors(case)
    failed = []
    for path, _ in PATHS:
        failed += _judge('plan parity %s %s' % (P.case_id(case), path), _device(case, path, calls), ref, floors)[1]
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 2. exact zeros, one-hot rows
@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_weights_outside_the_window_are_exactly_zero(case, calls):
    """every device weight outside [p - back, p + ahead] ∩ [0, len) is == 0.0, p from the plan alone (held behind n_plan,
    clamped to the item); the weights inside sum to 1; with (0, 0) every alignment row is exactly one-hot at the plan"""
    T_in, lens, win, frames, plan, n_plan = case
    p = P.centres(plan, n_plan, lens, frames)
    out = P.outside(p, lens, win, T_in)
    for path, _ in PATHS:
        align = _device(case, path, calls)[2]
        print('exact zeros %s %s: p of the last item %s, largest weight outside %.3e'
              % (P.case_id(case), path, p[-1].tolist(), align[out].abs().max().item()))
        assert (align[out] == 0.0).all()
        assert (align.double().sum(2) - 1).abs().max() < 1e-5
        if win == (0, 0):
            assert torch.equal(align, torch.nn.functional.one_hot(p, T_in).to(F32))


# ------------------------------------------------------------------------------------------------ 3. a shifted plan is seen
@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_a_shifted_plan_or_a_wider_window_in_the_oracle_is_seen(case, calls):
    """against a reference whose plan is shifted by one frame or by one symbol, or whose window is one position wider in front
    or behind, the unaltered device result is over the parity bound on align.  The device results are reused."""
    back, ahead = case[2]
    floors = P.floors(case)
    for path, _ in PATHS:
        res = _device(case, path, calls)
        others = [(how, P.reference(case, F64, how)) for how in ('frame', 'symbol')]
        others += [(w, P.reference(case, F64, None, w)) for w in ((back, ahead + 1), (back + 1, ahead))]
        for what, ref in others:
            ratio, _ = _judge('plan against %s, %s %s' % (what, P.case_id(case), path), res, ref[:3], floors)
            assert ratio['align'] > 1, (what, ratio)


# ------------------------------------------------------------------------------------------------ 4. stepwise and chunked runs
@pytest.mark.parametrize("case", [P.CASES[6], P.CASES[7], P.CASES[1]], ids=[IDS[6], IDS[7], IDS[1]])
def test_a_chunked_run_continues_the_plan(case, calls):
    """the launch-per-stage loop in chunks of 3 frames (calls with t_begin = 3, 6, ...: t is the absolute frame) gives the bits
    of the one-call run"""
    whole = _device(case, 'launch-per-stage', calls)
    parts = _decode(case, False, calls, chunk=3)
    for q, a, b in zip(('mel', 'gate', 'align'), parts, whole):
        assert torch.equal(a, b), q


@pytest.mark.parametrize("case", [P.CASES[3], P.CASES[6]], ids=[IDS[3], IDS[6]])
def test_stepwise_decode_api_honours_the_plan(case, calls):
    """initialize_decoder_states(plan=...) + decode() frame by frame equals inference() under the plan: within the parity bound
    of the planned reference, and within twice that bound of inference() (two results inside one bound are at most two bounds
    apart)"""
    T_in, lens, win, frames = case[:4]
    ref, floors = P.reference(case, F64)[:3], P.floors(case)
    inf = _device(case, 'default', calls)
    dec, memory = _decoder(case)
    plan, n_plan = _plan(case)
    with torch.no_grad():
        x = dec.get_go_frame(memory)
        dec.initialize_decoder_states(memory, mask=None, plan=plan, n_plan=n_plan, plan_window=win)
        mels, gates, als = [], [], []
        for _ in range(frames):
            m, gt, al = dec.decode(dec.prenet(x))
            mels.append(m.clone()), gates.append(gt.clone()), als.append(al.clone())
            x = m
        mel, gate, align = dec.parse_decoder_outputs(mels, gates, als)
    torch.cuda.synchronize()
    res = (mel.cpu(), gate.squeeze(-1).cpu(), align.cpu())
    _, failed = _judge('stepwise plan %s' % P.case_id(case), res, ref, floors)
    assert not failed, failed
    bound = S.bounds(floors, ref, K)
    for i, q in enumerate(('mel', 'gate', 'align')):
        d = (res[i] - inf[i]).abs().max().item()
        print('stepwise against inference %s %-5s %.2e (2 x bound %.2e)' % (P.case_id(case), q, d, 2 * bound[q]))
        assert d < 2 * bound[q], q
    assert (dec.attention_weights_cum.cpu() - align.cpu().sum(1)).abs().max() < 1e-5      # the planned weights accumulate


# ------------------------------------------------------------------------------------------------ 5. who ends the decode
@pytest.mark.parametrize("case", [P.CASES[2], P.CASES[5], P.CASES[3]], ids=[IDS[2], IDS[5], IDS[3]])
def test_plan_stop(case, calls, capsys):
    """plan_stop = 'plan': item b has exactly n_plan[b] frames, equal to the first n_plan[b] frames of the run that went on, and
    a gate that fires on frame 0 ends nothing; nothing warns about max decoder steps.  'gate': that gate ends the decode."""
    T_in, lens, win, frames, _, n_plan = case
    long_run = _device(case, 'default', calls)
    plan, n_plan_d = _plan(case)
    ragged = any(n != T_in for n in lens)
    for bias, stop, want in ((-1e3, 'plan', list(n_plan)), (1e3, 'plan', list(n_plan)), (1e3, 'gate', [1] * len(lens))):
        dec, memory = _decoder(case, frames=frames + 5)
        dec.gate_threshold = 0.5
        with torch.no_grad():
            dec.gate_layer.bias.fill_(bias)
            kw = dict(plan=plan, n_plan=n_plan_d, plan_window=win, plan_stop=stop)
            if ragged:
                mel, gate, align, n_frames = dec.inference_batch(memory, lens, **kw)
                assert n_frames.tolist() == want, (stop, bias)
            else:
                mel, gate, align = dec.inference(memory, **kw)
        torch.cuda.synchronize()
        assert mel.shape == (len(lens), 80, max(want)) and align.shape == (len(lens), max(want), T_in), (stop, bias)
        for b, n in enumerate(want):
            assert torch.equal(align[b, :n].cpu(), long_run[2][b, :n]) and torch.equal(mel[b, :, :n].cpu(), long_run[0][b, :, :n])
            assert not align[b, n:].any() and not mel[b, :, n:].any() and (gate[b, n:] == 1e3).all()
    assert 'max decoder steps' not in capsys.readouterr().out


def test_a_session_without_a_plan_launches_what_it_launched(calls, monkeypatch):
    """off by default: without the new arguments the entry points are the parent's (plain, _items, _window)"""
    import t2v_hip
    names = []
    real = t2v_hip.InferenceSession._constrained
    monkeypatch.setattr(t2v_hip.InferenceSession, '_constrained',
                        lambda self, name, args: names.append(real(self, name, args)[0]) or real(self, name, args))
    case = P.CASES[0]
    dec, memory = _decoder(case)
    with torch.no_grad():
        dec.inference(memory)
        dec.inference_batch(memory, case[1])
        dec.attention_window = (1, 3)
        dec.inference(memory)
        dec.inference(memory, plan=_plan(case)[0], n_plan=_plan(case)[1])
        assert dec.attention_window == (1, 3)
    torch.cuda.synchronize()
    assert names == ['t2v_decoder_infer_persistent', 't2v_decoder_infer_persistent_items', 't2v_decoder_infer_persistent_window',
                     't2v_decoder_infer_persistent_plan'], names


def test_inference_ends_every_item_with_its_own_plan(calls):
    """inference() (no lengths) on a batch whose plans differ in length, plan_stop = 'plan': the output has max(n_plan) frames,
    item b is padded behind n_plan[b] (mel 0, gate logit 1e3, weights 0) and equals, before it, the run whose plans all go on;
    more than 8 items are decoded 8 at a time with their plan rows"""
    case = P.CASES[0]
    T_in, win, frames = case[0], case[2], case[3]
    dec, memory = _decoder(case)
    plan, _ = _plan(case)
    with torch.no_grad():
        full = dec.inference(memory, plan=plan, n_plan=torch.tensor([8, 8], dtype=torch.int32).cuda(), plan_window=win)
        n = torch.tensor([8, 5], dtype=torch.int32).cuda()
        mel, gate, al = dec.inference(memory, plan=plan, n_plan=n, plan_window=win)
        assert mel.shape == (2, 80, 8) and gate.shape == (2, 8, 1) and al.shape == (2, 8, T_in)
        assert torch.equal(mel[0], full[0][0]) and torch.equal(al[0], full[2][0])
        assert torch.equal(mel[1, :, :5], full[0][1, :, :5]) and torch.equal(al[1, :5], full[2][1, :5])
        assert not mel[1, :, 5:].any() and not al[1, 5:].any() and (gate[1, 5:] == 1e3).all()
        # nine items: a group of 8 on the launch-per-stage loop and a group of 1, each with its rows of the plan
        idx = [0, 1, 0, 1, 0, 1, 0, 1, 1]
        n9 = [8, 8, 7, 6, 5, 4, 3, 2, 6]
        mel9, gate9, al9 = dec.inference(memory[idx], plan=plan[idx], n_plan=torch.tensor(n9, dtype=torch.int32).cuda(),
                                         plan_window=win)
    torch.cuda.synchronize()
    assert mel9.shape == (9, 80, 8) and al9.shape == (9, 8, T_in)
    for b, (i, k) in enumerate(zip(idx, n9)):
        assert (al9[b, :k] - full[2][i, :k]).abs().max() < 1e-5 and (mel9[b, :, :k] - full[0][i, :, :k]).abs().max() < 1e-4, b
        assert not al9[b, k:].any() and not mel9[b, :, k:].any() and (gate9[b, k:] == 1e3).all(), b
