"""Host side of the planned free-running decode and its length regulator (no GPU): the integer definition of
tests/plan_ref.py on its edge cases, the C entries and their bindings, the planned reference against the unmodified oracle and
against the windowed reference of tests/window_ref.py, the conditions on the inputs that keep the bounds of
tests/test_attention_plan_gpu.py honest, the argument checks and the command lines."""
import os
import re

import numpy as np
import pytest
import torch

import plan_ref as P
import steer_ref as S
import window_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
K = 16.0
IDS = [P.case_id(c) for c in P.CASES]


# ------------------------------------------------------------------------------------------------ the length regulator
def test_regulate_ties_at_exactly_half():
    """E_j = (C_j + 32768) >> 16 rounds a half up: cumulative ends 0.5, 1.0, 1.5, 2.0 give frame ends 1, 1, 2, 2"""
    plan, n = P.regulate(np.full((1, 4), 0.5, np.float32), [4], 6)
    assert n.tolist() == [2] and plan[0].tolist() == [0, 2, 2, 2, 2, 2]
    # 1.5 + 1.0 + 0.5: ends 1.5 -> 2, 2.5 -> 3, 3.0 -> 3: the last symbol has no frame and is skipped
    plan, n = P.regulate(np.array([[1.5, 1.0, 0.5]], np.float32), [3], 8)
    assert n.tolist() == [3] and plan[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    # a rate that makes the ties: 1 * 0.5
    plan, n = P.regulate(np.ones((1, 4), np.float32), [4], 6, rate=0.5)
    assert n.tolist() == [2] and plan[0].tolist() == [0, 2, 2, 2, 2, 2]
    # q itself rounds ties to even in 16.16: 2^-17 frames is half a unit -> 0; three of them -> 1.5 units -> 2
    plan, n = P.regulate(np.array([[2.0 ** -17, 3 * 2.0 ** -17, 1.0]], np.float32), [3], 4)
    assert n.tolist() == [1] and plan[0].tolist() == [2, 2, 2, 2]


def test_regulate_zero_length_symbols_and_empty_rows():
    plan, n = P.regulate(np.array([[0, 2, 0, 0, 1, 0]], np.float32), [6], 5)
    assert n.tolist() == [3] and plan[0].tolist() == [1, 1, 4, 4, 4]
    plan, n = P.regulate(np.zeros((2, 3), np.float32), [3, 0], 4)
    assert n.tolist() == [0, 0] and not plan.any()
    # symbols past n_ids are not read
    plan, n = P.regulate(np.array([[1, 1, np.nan, -5]], np.float32), [2], 4)
    assert n.tolist() == [2] and plan[0].tolist() == [0, 1, 1, 1]


def test_regulate_scalar_rate_equals_per_symbol_rate():
    g = np.random.default_rng(0)
    dur = (g.integers(0, 9, (3, 40)) / 4).astype(np.float32)
    for r in (0.5, 1.25, 2.0, 1 / 3):
        a = P.regulate(dur, [40, 17, 1], 64, rate=r)
        b = P.regulate(dur, [40, 17, 1], 64, rate=np.full(dur.shape, r, np.float32))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = P.regulate(dur, [40, 17, 1], 64), P.regulate(dur, [40, 17, 1], 64, rate=1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a row is its own: alone it gives what it gives in the batch
    for i, L in enumerate((40, 17, 1)):
        one = P.regulate(dur[i:i + 1], [L], 64, rate=1.25)
        assert np.array_equal(one[0][0], P.regulate(dur, [40, 17, 1], 64, rate=1.25)[0][i])


def test_regulate_truncates_at_T_max():
    dur = np.array([[3, 3, 3, 3]], np.float32)
    plan, n = P.regulate(dur, [4], 7)
    assert n.tolist() == [7] and plan[0].tolist() == [0, 0, 0, 1, 1, 1, 2]
    plan, n = P.regulate(dur, [4], 1)
    assert n.tolist() == [1] and plan[0].tolist() == [0]
    plan, n = P.regulate(dur, [4], 14)
    assert n.tolist() == [12] and plan[0].tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 5
    # the largest admitted duration does not overflow
    plan, n = P.regulate(np.full((1, 8), 2.0 ** 20, np.float32), [8], 5)
    assert n.tolist() == [5] and not plan.any()


def test_regulate_refuses_rows():
    base = np.ones((6, 3), np.float32)
    base[1, 1] = -0.25
    base[2, 2] = np.nan
    base[3, 0] = np.inf
    base[4, 1] = 2.0 ** 20 + 1
    plan, n = P.regulate(base, [3] * 6, 4)
    assert n.tolist() == [3, -1, -1, -1, -1, 3] and not plan[1:5].any() and plan[0].tolist() == [0, 1, 2, 2]
    # through the rate too: a negative factor, and a product above 2^20 of two admissible numbers
    _, n = P.regulate(np.ones((1, 3), np.float32), [3], 4, rate=-1.0)
    assert n.tolist() == [-1]
    _, n = P.regulate(np.full((1, 2), 2.0 ** 19, np.float32), [2], 4, rate=4.0)
    assert n.tolist() == [-1]
    _, n = P.regulate(np.full((1, 2), 2.0 ** 19, np.float32), [2], 4, rate=2.0)
    assert n.tolist() == [4]


# ------------------------------------------------------------------------------------------------ the C ABI
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 't2vae.h')).read(), flags=re.S)


def _prototypes():
    out = {}
    for m in re.finditer(r'\b(?:int|long|void|size_t)\s+(t2v_\w+)\s*\(([^;]*?)\)\s*;', _header(), flags=re.S):
        out[m.group(1)] = [' '.join(a.split()) for a in m.group(2).split(',') if a.strip()]
    return out


def test_plan_entries_are_declared_and_bound_from_the_header():
    import ctypes as C
    import t2v_abi
    import t2v_hip
    protos = _prototypes()
    lib = t2v_hip.load_library()
    # the planned entries take the arguments of the windowed entries plus plan, plan_stride, n_plan as plain arguments
    for new, old in (('t2v_decoder_infer_steps_plan', 't2v_decoder_infer_steps_window'),
                     ('t2v_decoder_infer_persistent_plan', 't2v_decoder_infer_persistent_window')):
        assert new in t2v_hip.EXPORTS and new in protos and hasattr(lib, new), new
        assert protos[new][:-4] == protos[old][:-1] and protos[new][-1] == protos[old][-1]
        assert protos[new][-4:-1] == ['const int32_t* plan', 'int plan_stride', 'const int32_t* n_plan']
        assert getattr(lib, new).argtypes == getattr(lib, old).argtypes[:-1] + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert 't2v_duration_plan' in t2v_hip.EXPORTS and len(lib.t2v_duration_plan.argtypes) == len(protos['t2v_duration_plan']) == 13
    # no new host struct: the twelve of the binding table, and the windowed entries as they were
    assert len(t2v_abi.HOST_STRUCTS) + len(t2v_abi.DEVICE_STRUCTS) == 12
    assert len(protos['t2v_decoder_infer_steps_window']) == 13 and len(protos['t2v_decoder_infer_persistent_window']) == 11
    assert t2v_hip.PLAN_MAX_SYMBOLS == t2v_abi.load().define('T2V_PLAN_MAX_SYMBOLS') >= 1025
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('t2v_decoder_infer_steps_plan', 't2v_decoder_infer_persistent_plan', 't2v_duration_plan'):
        assert name in doc, name


# ------------------------------------------------------------------------------------------------ the planned reference
def test_all_covering_window_is_the_oracle_bit_for_bit():
    """a window that covers the text leaves every mask bit clear whatever the plan says: decode() is O.decoder_inference"""
    import t2v_oracle as O
    T_in, lens, frames = 97, (97, 97, 97), 6
    dec, memory = P.inputs(T_in, lens)
    sd = P.state_dict(dec, F32)
    with torch.no_grad():
        mel, gate, align = O.decoder_inference(sd, memory, max_steps=frames, stop_on_gate=False)
    plan = ((0, 40, 96, 3, 500, 7),) * 3
    got = P.decode(sd, memory, lens, (T_in, T_in), plan, (6, 6, 6), frames)
    assert torch.equal(got[0], mel) and torch.equal(got[1], gate.squeeze(-1)) and torch.equal(got[2], align)


@pytest.mark.parametrize("case", [W.CASES[0], W.CASES[3]], ids=[W.case_id(W.CASES[0]), W.case_id(W.CASES[3])])
def test_a_plan_of_the_windowed_centres_is_the_windowed_reference_bit_for_bit(case):
    """the p sequence the windowed reference took, given back as a plan under the same (back, ahead), gives its result"""
    T_in, lens, win, frames = case
    dec, memory = W.inputs(T_in, lens, win[1])
    for dtype in (F32, F64):
        ref = W.reference(case, dtype)
        got = P.decode(W.state_dict(dec, dtype), memory.to(dtype), lens, win, ref[3], (frames,) * len(lens), frames)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_centres_hold_and_clamp():
    p = P.centres(((0, 5, 9, 30), (2, 2, 2, 2)), (3, 1), (8, 2), 6)
    assert p.tolist() == [[0, 5, 7, 7, 7, 7], [1, 1, 1, 1, 1, 1]]
    assert P.centres(((0, 5, 9, 30),), (4,), (40,), 3, t0=2).tolist() == [[9, 30, 30]]
    assert P.centres(((-3, 5),), (2,), (4,), 2).tolist() == [[0, 3]]


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_reference_conditions(case):
    """A condition on the inputs, not a measurement: for every case of the GPU test the fp64 reference changes on `align` by at
    least 1000 parity bounds when the plan is shifted by one frame and when it is shifted by one symbol, so a kernel that reads
    plan[t - 1], plan[t + 1] or a neighbouring symbol cannot pass.  Also: the planned fp32 and fp64 references differ by
    round-off alone, weights outside the window are exactly 0, the case uses plan values at len - 1 where it says so."""
    T_in, lens, win, frames, plan, n_plan = case
    assert 8 <= frames <= 12 and len(plan) == len(lens) == len(n_plan) and all(1 <= n <= len(r) for n, r in zip(n_plan, plan))
    r64 = P.reference(case, F64)
    B = len(lens)
    assert r64[2].shape == (B, frames, T_in) and r64[0].shape == (B, 80, frames)
    floors = P.floors(case)
    assert max(floors.values()) < 2e-6, floors
    bound = S.bounds(floors, r64[:3], K)['align']
    assert (r64[2][P.outside(r64[3], lens, win, T_in)] == 0).all() and (r64[2].sum(2) - 1).abs().max() < 1e-12
    if win == (0, 0):
        assert torch.equal(r64[2], torch.nn.functional.one_hot(r64[3], T_in).to(F64))
    for how in ('frame', 'symbol'):
        d = (P.reference(case, F64, how)[2] - r64[2]).abs().max().item()
        print('%s: plan shifted by one %s moves align by %.3e = %.0f bounds (bound %.2e)' % (P.case_id(case), how, d, d / bound, bound))
        assert d >= 1000 * bound, (how, d, bound)
    for other in ((win[0], win[1] + 1), (win[0] + 1, win[1])):
        d = (P.reference(case, F64, None, other)[2] - r64[2]).abs().max().item()
        print('%s: window %s instead of %s moves align by %.3e = %.0f bounds' % (P.case_id(case), other, win, d, d / bound))
        assert d >= 1000 * bound, (other, d, bound)


def test_cases_cover_what_the_issue_names():
    wins = set(c[2] for c in P.CASES)
    assert wins == {(0, 0), (1, 1), (1, 3)}
    shapes = set((c[0], len(c[1])) for c in P.CASES)
    assert {(224, 1), (128, 4), (224, 4), (555, 2)} <= shapes
    assert P.persistent_fits(1, 224) and P.persistent_fits(4, 128) and not P.persistent_fits(4, 224) and not P.persistent_fits(1, 225)
    # the plans put a window centre on both sides of every cut
    seen = set()
    for T_in, lens, win, frames, plan, n_plan in P.CASES:
        seen |= set(P.centres(plan, n_plan, lens, frames).flatten().tolist())
    for cut in (16, 32, 64, 80, 128, 192, 256, 288, 384, 480, 512):
        assert cut - 1 in seen and cut in seen, cut
    # ragged: a value at len - 1, a value beyond it, and a plan shorter than the run
    assert any(n - 1 in r and max(r) >= n for c in P.CASES for r, n in zip(c[4], c[1]))
    assert any(n < c[3] for c in P.CASES for n in c[5])


# ------------------------------------------------------------------------------------------------ the Python surface
def test_check_plan_refuses_what_the_kernels_cannot_take():
    import t2v_hip
    cpu = torch.device('cpu')
    plan = torch.zeros(2, 6, dtype=torch.int32)
    n = torch.tensor([6, 3], dtype=torch.int32)
    got = t2v_hip.check_plan(plan, n, 2, 10, cpu, (0, 0))
    assert got[0] is plan and got[1] == [6, 3]
    bad = [
        dict(window=None),                                               # a plan needs a window
        dict(plan=plan.long()), dict(n_plan=n.long()), dict(plan=plan.float()),          # dtype
        dict(plan=plan[0]), dict(plan=plan[:1]), dict(n_plan=n[:1]), dict(plan=plan.t().contiguous().t()),     # shape, strides
        dict(n_plan=torch.tensor([6, 0], dtype=torch.int32)), dict(n_plan=torch.tensor([7, 3], dtype=torch.int32)),
        dict(max_steps=5),                                               # longer than the session
        dict(plan=None), dict(n_plan=None), dict(plan=[[0] * 6] * 2),
        dict(device=torch.device('meta')),                               # another device
    ]
    for kw in bad:
        a = dict(plan=plan, n_plan=n, B=2, max_steps=10, device=cpu, window=(0, 0))
        a.update(kw)
        with pytest.raises(ValueError):
            t2v_hip.check_plan(a['plan'], a['n_plan'], a['B'], a['max_steps'], a['device'], a['window'])


def test_decoder_validates_the_plan_arguments():
    import inspect
    import hparams as HP
    import model as M
    dec = M.Decoder(HP.create_hparams("max_decoder_steps=10"))
    for f in (dec.inference, dec.inference_batch, dec.initialize_decoder_states):
        par = inspect.signature(f).parameters
        assert [par[k].default for k in ('plan', 'n_plan', 'plan_window', 'plan_stop')] == [None, None, (1, 1), 'plan'], f
    cpu = torch.device('cpu')
    plan, n = torch.zeros(1, 4, dtype=torch.int32), torch.tensor([4], dtype=torch.int32)
    assert dec._checked_plan(None, None, (1, 1), 'plan', 1, cpu) is None
    pl = dec._checked_plan(plan, n, [0, 2], 'gate', 1, cpu)
    assert pl[2] == (0, 2) and pl[3] == [4] and pl[4] == 'gate'
    assert dec._plan_steps(pl) == (10, dec.gate_threshold) and dec._plan_steps(None) == (10, dec.gate_threshold)
    steps, thr = dec._plan_steps(dec._checked_plan(plan, n, (1, 1), 'plan', 1, cpu))
    assert steps == 4 and thr > 1                                        # a threshold no sigmoid reaches: the plan ends the loop
    for kw in (dict(plan_stop='never'), dict(plan_window=None), dict(plan_window=(1,)), dict(plan_window=(-1, 0)),
               dict(n=torch.tensor([11], dtype=torch.int32), plan=torch.zeros(1, 11, dtype=torch.int32)), dict(n=None)):
        a = dict(plan=plan, n=n, plan_window=(1, 1), plan_stop='plan')
        a.update(kw)
        with pytest.raises(ValueError):
            dec._checked_plan(a['plan'], a['n'], a['plan_window'], a['plan_stop'], 1, cpu)
    assert dec.attention_window is None                                  # plan_window belongs to a call, not to the decoder


def test_command_line_flags_are_checked():
    import evaluate as E
    import synthesizer as S
    syn = ['--load_path', 'ck', '--text', 'x']
    ev = ['--load_path', 'ck', '--filelist_path', 'f', '--out', 'o']
    a = S.parse_args(syn + ['--rhythm_from', 'a.wav', '--rhythm_scale', '1.5', '--rhythm_window', '0,2'])
    assert (a.rhythm_from, a.durations, a.rhythm_scale, a.rhythm_window) == ('a.wav', None, 1.5, (0, 2))
    a = S.parse_args(syn)
    assert (a.rhythm_from, a.durations, a.rhythm_scale, a.rhythm_window) == (None, None, 1.0, None)
    assert E.parse_args(ev).rhythm is None and E.parse_args(ev + ['--rhythm', 'ref']).rhythm == 'ref'
    for bad in (['--rhythm_scale', '2'], ['--rhythm_window', '1,1'], ['--rhythm_from', 'a', '--durations', 'd.npz'],
                ['--rhythm_from', 'a', '--rhythm_scale', '0'], ['--rhythm_from', 'a', '--rhythm_window', '1']):
        with pytest.raises(SystemExit):
            S.parse_args(syn + bad)
    for bad in (['--rhythm', 'text'], ['--rhythm_window', '1,1']):
        with pytest.raises(SystemExit):
            E.parse_args(ev + bad)
