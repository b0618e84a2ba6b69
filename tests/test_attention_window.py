"""Host side of the attention window of the free-running decode (Decoder.attention_window; no GPU): the C entries
and their bindings, the windowed reference of tests/window_ref.py against the unmodified oracle, the conditions that keep the
bounds of tests/test_attention_window_gpu.py honest, and the two command lines."""
import ctypes as C
import os
import re

import pytest
import torch

import window_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 't2vae.h')).read(), flags=re.S)


def _prototypes():
    out = {}
    for m in re.finditer(r'\b(?:int|long|void|size_t)\s+(t2v_\w+)\s*\(([^;]*?)\)\s*;', _header(), flags=re.S):
        out[m.group(1)] = [a.strip() for a in m.group(2).split(',') if a.strip()]
    return out


def test_window_entries_are_declared_and_bound_with_matching_arity():
    import t2v_hip
    protos = _prototypes()
    lib = t2v_hip.load_library()
    # the windowed entries take the arguments of the per-item entries they extend, plus the t2v_dec_window pointer
    for new, old in (('t2v_decoder_infer_steps_window', 't2v_decoder_infer_steps_items'),
                     ('t2v_decoder_infer_persistent_window', 't2v_decoder_infer_persistent_items')):
        assert new in t2v_hip.EXPORTS and new in protos and hasattr(lib, new), new
        assert len(getattr(lib, new).argtypes) == len(protos[new]), (new, protos[new])
        assert protos[new][:-2] == protos[old][:-1] and protos[new][-1] == protos[old][-1]
        assert 't2v_dec_window' in protos[new][-2]
        assert getattr(lib, new).argtypes[-2] == C.POINTER(t2v_hip._DecWindow)
        assert getattr(lib, new).argtypes[:-2] == getattr(lib, old).argtypes[:-1]
    m = re.search(r'typedef struct t2v_dec_window \{(.*?)\} t2v_dec_window;', _header(), flags=re.S)
    assert m and re.sub(r'\s+', ' ', m.group(1)).strip() == 'int32_t back; int32_t ahead;'
    assert t2v_hip._DecWindow._fields_ == [('back', C.c_int32), ('ahead', C.c_int32)] and C.sizeof(t2v_hip._DecWindow) == 8
    # the existing decode entries keep their signatures
    assert len(protos['t2v_decoder_infer_steps']) == 11 and len(protos['t2v_decoder_infer_persistent']) == 9
    assert len(protos['t2v_decoder_infer_steps_items']) == 12 and len(protos['t2v_decoder_infer_persistent_items']) == 10
    assert len(protos['t2v_decoder_persist_supported']) == 2
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 't2v_decoder_infer_steps_window' in doc and 't2v_decoder_infer_persistent_window' in doc and 't2v_dec_window' in doc


def test_all_covering_window_is_the_oracle_bit_for_bit():
    """a window that covers the text leaves every mask bit clear: the loop of window_ref is O.decoder_inference"""
    import t2v_oracle as O
    T_in, lens, frames = 97, (97, 97, 97), 6
    dec, memory = W.inputs(T_in, lens, 20)
    sd = W.state_dict(dec, F32)
    with torch.no_grad():
        mel, gate, align = O.decoder_inference(sd, memory, max_steps=frames, stop_on_gate=False)
    got = W.decode(sd, memory, lens, (T_in, T_in), frames)
    assert torch.equal(got[0], mel) and torch.equal(got[1], gate.squeeze(-1)) and torch.equal(got[2], align)
    none = W.decode(sd, memory, lens, None, frames)
    assert all(torch.equal(a, b) for a, b in zip(got, none))


@pytest.mark.parametrize("case", W.CASES, ids=[W.case_id(c) for c in W.CASES])
def test_reference_conditions(case):
    """What the parity bound of the GPU test rests on, asserted on the reference alone: at every frame of every item the two
    largest weights of the fp64 reference are >= 1e-3 apart (three orders above the fp32 round-off of a softmax weight, so
    round-off cannot move a window), the fp32 and fp64 references take the same window at every frame, no frame or item is
    left out, and the window matters: the unconstrained decoder has most of its mass outside it."""
    T_in, lens, win, frames = case
    r64, r32 = W.reference(case, F64), W.reference(case, F32)
    B = len(lens)
    assert r64[2].shape == (B, frames, T_in) and r64[3].shape == (B, frames) and r64[0].shape == (B, 80, frames)
    gap = W.top_two_gap(r64[2], lens)
    print('%s: min top-two gap %.2e, p of item 0 %s' % (W.case_id(case), gap, r64[3][0].tolist()))
    assert gap >= 1e-3
    assert torch.equal(r64[3], r32[3])
    assert (r64[3][:, 0] == 0).all() and (r64[3] < torch.tensor(lens)[:, None]).all()
    # exact zeros outside the window and the length, ones inside in sum
    assert (W.outside_mass(r64[2], r64[3], lens, win) == 0).all()
    assert (r64[2].sum(2) - 1).abs().max() < 1e-12
    # the window march: every step of p stays inside the window it was taken from
    step = r64[3][:, 1:] - r64[3][:, :-1]
    assert (step >= -win[0]).all() and (step <= win[1]).all()
    floors = W.floors(case)
    assert max(floors.values()) < 2e-6, floors                         # fp32 round-off, not a divergence
    free = W.reference(case, F64, None)
    out = W.outside_mass(free[2], r64[3], lens, win)
    print('   unconstrained: |align - windowed| %.2f, mass outside the window %.2f .. %.2f (frames >= 1)'
          % ((free[2] - r64[2]).abs().max().item(), out[:, 1:].min().item(), out[:, 1:].max().item()))
    assert (free[2] - r64[2]).abs().max() > 0.5 and out[0, 1:].max() > 0.5


def test_the_issue_table_is_reproduced():
    """item 0's window centres of the seven cases the feature was specified on"""
    want = {0: [0, 0, 0, 0, 3, 4], 2: [0, 0, 1, 2, 2, 3, 4, 4], 3: [0, 0, 20, 40, 60, 80], 4: [0, 0, 60, 120, 180],
            5: [0, 0, 60, 120, 180], 6: [0, 0, 130, 260, 390, 520]}
    for i, p in want.items():
        assert W.reference(W.CASES[i], F64)[3][0].tolist() == p, W.case_id(W.CASES[i])
    assert W.reference(W.CASES[1], F64)[3][0].tolist()[-4:] == [3, 4, 4, 4]
    assert W.reference(W.CASES[3], F64)[3][2].tolist()[-1] == 16             # the 17-symbol item ends pinned at its last symbol


def test_command_lines_take_the_window():
    import evaluate as E
    import synthesizer as S
    syn = ['--load_path', 'ck', '--text', 'x']
    ev = ['--load_path', 'ck', '--filelist_path', 'f', '--out', 'o']
    assert S.parse_args(syn + ['--attention_window', '1,3']).attention_window == (1, 3)
    assert E.parse_args(ev + ['--attention_window', '1,3']).attention_window == (1, 3)
    assert S.parse_args(syn + ['--attention_window', '0,0']).attention_window == (0, 0)
    assert S.parse_args(syn).attention_window is None and E.parse_args(ev).attention_window is None
    for bad in ('1', '-1,3', 'a,b', '1,2,3', '1,-3', '1.5,2'):
        for mod, base in ((S, syn), (E, ev)):
            with pytest.raises(SystemExit):
                mod.parse_args(base + ['--attention_window', bad])


def test_decoder_and_synthesizer_validate_the_window():
    import hparams as HP
    import model as M
    from synthesizer import Synthesizer
    hp = HP.create_hparams()
    assert 'attention_window' not in hp.values()
    dec = M.Decoder(hp)
    assert dec.attention_window is None
    dec.attention_window = (1, 3)
    assert dec.attention_window == (1, 3)
    dec.attention_window = [0, 7]
    assert dec.attention_window == (0, 7)
    for bad in ((1,), (1, 2, 3), (-1, 3), (1, -3), (1.0, 3), '13', 'a,b', 5, (True, 3), (None, 3)):
        with pytest.raises(ValueError):
            dec.attention_window = bad
        assert dec.attention_window == (0, 7)
    dec.attention_window = None
    assert dec.attention_window is None
    assert 'attention_window' not in ''.join(dec.state_dict())
    assert Synthesizer(hp).attention_window is None and Synthesizer(hp, attention_window=(2, 5)).attention_window == (2, 5)
    with pytest.raises(ValueError):
        Synthesizer(hp, attention_window=(1,))
