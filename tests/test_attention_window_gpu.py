"""The attention window of the free-running decode (Decoder.attention_window) on the device against the windowed fp64
reference of tests/window_ref.py, on the ramped, steered inputs on which the window marches across every tile and chunk cut of
the kernels while the unconstrained decoder puts 74 to 99 % of its mass elsewhere.

Bounds: the rule of test_decoder_steered_gpu.py::test_steered_decode_matches_oracle.  floor = windowed fp32 reference minus
windowed fp64 reference per case and quantity; a quantity passes below 16 * max(floor, 4 * 2^-24 * max |reference|).
tests/test_attention_window.py asserts, on the reference alone, what that rests on: the two largest weights of every frame are
>= 1e-3 apart and the fp32 and fp64 references take the same window at every frame, so round-off cannot move a window.

The persistent launch takes what its LDS holds (include/t2vae.h: T_in <= 224 at B = 1, 192 at B = 2, 160 at B = 3, 128 at
B = 4): the T_in = 224, B = 4 group runs the launch-per-stage loop on both paths, and the two last cases of window_ref.CASES put
the persistent kernels at both corners of that range.  Every case prints its figures before it asserts (pytest -s).
"""
import copy

import pytest
import torch

import steer_ref as S
import window_ref as W

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K = 16.0
PATHS = (('launch-per-stage', False), ('default', None))
IDS = [W.case_id(c) for c in W.CASES]
_DEVICE = {}


@pytest.fixture(scope='module', autouse=True)
def _release_results():
    yield
    _DEVICE.clear()
    W.reference.cache_clear()
    W.inputs.cache_clear()


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


def _decoder(case, window):
    T_in, lens, win, frames = case
    dec, memory = W.inputs(T_in, lens, win[1])
    dec = copy.deepcopy(dec).cuda().eval()                 # (the cached CPU decoder stays where the references read it)
    dec.gate_threshold = 1.0                               # never stop: all frames
    dec.max_decoder_steps = frames
    dec.attention_window = window
    return dec, memory.cuda()


def _decode(case, persistent, window, calls):
    """(mel (B, 80, frames), gate (B, frames), align (B, frames, T_in)) on the host: inference_batch for ragged lengths,
    inference for full-length items; asserts which decode loop ran"""
    import t2v_hip
    T_in, lens, _, frames = case
    dec, memory = _decoder(case, window)
    calls.update(persistent=0, stages=0)
    with torch.no_grad():
        if any(n != T_in for n in lens):
            mel, gate, align, n_frames = dec.inference_batch(memory, lens, persistent=persistent)
            assert n_frames.tolist() == [frames] * len(lens)
        else:
            mel, gate, align = dec.inference(memory, persistent=persistent)
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    one_launch = persistent is None and W.persistent_fits(len(lens), T_in)
    assert calls == ({'persistent': 1, 'stages': 0} if one_launch else {'persistent': 0, 'stages': 1}), (W.case_id(case), calls)
    assert mel.shape == (len(lens), 80, frames) and align.shape == (len(lens), frames, T_in)
    return mel.cpu(), gate.squeeze(-1).cpu(), align.cpu()


def _device(case, path, calls):
    """the windowed device result of (case, path), decoded once per module"""
    if (case, path) not in _DEVICE:
        _DEVICE[case, path] = _decode(case, dict(PATHS)[path], case[2], calls)
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
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_windowed_decode_matches_the_windowed_oracle(case, calls):
    """mel, gate and align of both decode paths within 16 * max(floor, 4 * 2^-24 * scale) of the windowed fp64 reference"""
    ref, floors = W.reference(case, F64)[:3], W.floors(case)
    failed = []
    for path, _ in PATHS:
        failed += _judge('window parity %s %s' % (W.case_id(case), path), _device(case, path, calls), ref, floors)[1]
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 2. exact zeros
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_weights_outside_the_window_are_exactly_zero(case, calls):
    """every device weight outside [p - back, p + ahead] ∩ [0, len) is == 0.0, p from the device's own previous row (the first
    index of its largest weight; 0 at frame 0), and the weights inside sum to 1"""
    T_in, lens, win, frames = case
    for path, _ in PATHS:
        align = _device(case, path, calls)[2]
        prev = torch.cat((torch.zeros(len(lens), 1, T_in), align[:, :-1]), 1)
        p = prev.argmax(2)
        out = W.outside_mass(align, p, lens, win)
        pos = torch.arange(T_in)[None, None, :]
        outside = (pos < p[:, :, None] - win[0]) | (pos > p[:, :, None] + win[1]) | (pos >= torch.tensor(lens)[:, None, None])
        print('exact zeros %s %s: p of item 0 %s, largest weight outside %.3e' % (W.case_id(case), path, p[0].tolist(),
                                                                                 align[outside].abs().max().item()))
        assert (align[outside] == 0.0).all() and (out == 0).all()
        assert (align.double().sum(2) - 1).abs().max() < 1e-5
        assert torch.equal(p, W.reference(case, F64)[3])


# ------------------------------------------------------------------------------------------------ 3. an off-by-one window is seen
@pytest.mark.parametrize("case", [W.CASES[3], W.CASES[6]], ids=[IDS[3], IDS[6]])
def test_an_off_by_one_window_in_the_oracle_is_seen(case, calls):
    """against a reference whose window is one position wider, in front or behind, the unaltered device result is over the
    parity bound on align"""
    back, ahead = case[2]
    floors = W.floors(case)
    for path, _ in PATHS:
        res = _device(case, path, calls)
        for other in ((back, ahead + 1), (back + 1, ahead)):
            ratio, _ = _judge('window %s against %s, %s %s' % (case[2], other, W.case_id(case), path), res,
                              W.reference(case, F64, other)[:3], floors)
            assert ratio['align'] > 1, (other, ratio)


# ------------------------------------------------------------------------------------------------ 4. a window over everything
@pytest.mark.parametrize("case", [W.CASES[0], W.CASES[3], W.CASES[5], W.CASES[6]], ids=[IDS[0], IDS[3], IDS[5], IDS[6]])
def test_an_all_covering_window_changes_nothing(case, calls):
    """with (T_in, T_in) the windowed kernels give the unconstrained decoder: within the bound of the unconstrained fp64
    reference (floor: unconstrained fp32 minus fp64), on both paths"""
    T_in = case[0]
    ref = W.reference(case, F64, None)[:3]
    floors = {k: v[0] for k, v in S.compare(W.reference(case, F32, None)[:3], ref).items()}
    failed = []
    for path, persistent in PATHS:
        res = _decode(case, persistent, (T_in, T_in), calls)
        failed += _judge('all-covering window %s %s' % (W.case_id(case), path), res, ref, floors)[1]
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 5. stepwise API
@pytest.mark.parametrize("case", [W.CASES[5], W.CASES[7]], ids=[IDS[5], IDS[7]])
def test_stepwise_decode_api_honours_the_window(case, calls):
    """initialize_decoder_states + decode() frame by frame under a window equals inference() under it (the pattern of
    test_inference_gpu.py::test_stepwise_decode_api_equals_inference): within the parity bound of the windowed reference, and
    within twice that bound of inference() (two results inside one bound are at most two bounds apart)"""
    T_in, lens, win, frames = case
    ref, floors = W.reference(case, F64)[:3], W.floors(case)
    inf = _device(case, 'default', calls)
    dec, memory = _decoder(case, win)
    with torch.no_grad():
        x = dec.get_go_frame(memory)
        dec.initialize_decoder_states(memory, mask=None)
        mels, gates, als = [], [], []
        for _ in range(frames):
            m, gt, al = dec.decode(dec.prenet(x))
            mels.append(m.clone()), gates.append(gt.clone()), als.append(al.clone())
            x = m
        mel, gate, align = dec.parse_decoder_outputs(mels, gates, als)
    torch.cuda.synchronize()
    res = (mel.cpu(), gate.squeeze(-1).cpu(), align.cpu())
    _, failed = _judge('stepwise window %s' % W.case_id(case), res, ref, floors)
    assert not failed, failed
    bound = S.bounds(floors, ref, K)
    for i, q in enumerate(('mel', 'gate', 'align')):
        d = (res[i] - inf[i]).abs().max().item()
        print('stepwise against inference %s %-5s %.2e (2 x bound %.2e)' % (W.case_id(case), q, d, 2 * bound[q]))
        assert d < 2 * bound[q], q
    assert dec.attention_weights_cum.shape == (1, T_in)
    assert (dec.attention_weights_cum.cpu() - align.cpu().sum(1)).abs().max() < 1e-5      # the windowed weights accumulate


# ------------------------------------------------------------------------------------------------ 6. the public surface
def test_synthesizer_reads_within_the_window(tmp_path):
    """Synthesizer(..., attention_window=(1, 3)) on a random-init model (flat alignments, Prenet dropout on): the alignment
    statistics report no jump (jump_share counts steps forward by more than 3 positions), the argmax path never steps back by
    more than 1 or forward by more than 3, and under (0, 3) back_share is 0 too.  Without a window the same calls may report
    them."""
    import t2v_hip
    from synthesizer import Synthesizer
    from test_batch_synthesis_gpu import OTHER_TEXTS, _synth
    hp, ck, fl = _synth(tmp_path, "max_decoder_steps=24", gate_bias=-1e3)
    texts = [OTHER_TEXTS[1], "한국어 음성 합성"]
    for window in ((1, 3), (0, 3), None):
        syn = Synthesizer(hp, attention_window=window).load(ck, filelist_path=fl)
        assert syn.model.decoder.attention_window == window
        rows = syn.alignment(texts)
        with torch.no_grad():
            _, _, _, al, n_frames, lens = syn._synthesize_ragged(texts, False, None, (1.0, 0.0, 0.0, 0.0))
        path = t2v_hip.alignment_stats(al, n_frames.tolist(), lens).path.cpu()
        for b, r in enumerate(rows):
            step = (path[b, 1:n_frames[b]] - path[b, :n_frames[b] - 1]).long()
            print('window %s text %d: back_share %.3f jump_share %.3f steps %d .. %d over %d frames'
                  % (window, b, r['back_share'], r['jump_share'], step.min(), step.max(), r['n_frames']))
            assert r['n_frames'] == 24 and n_frames[b] == 24
            if window is None:
                continue
            assert r['jump_share'] == 0.0
            assert step.min() >= -window[0] and step.max() <= window[1]
            if window[0] == 0:
                assert r['back_share'] == 0.0
            # frame 0 attends within [0, ahead], and no weight leaves the window around the previous frame's position
            assert path[b, 0] <= window[1]
            a = al[b, :n_frames[b], :lens[b]].cpu()
            prev = torch.cat((torch.zeros(1, lens[b]), a[:-1]), 0).argmax(1)
            pos = torch.arange(lens[b])[None, :]
            assert (a[(pos < prev[:, None] - window[0]) | (pos > prev[:, None] + window[1])] == 0.0).all()
