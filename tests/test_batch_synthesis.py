"""Host side of batched synthesis (no GPU): the new C entry points are declared with the arity the ctypes bindings use, the
decoder's seed reservation reproduces the seeds of sequential inference() calls, and the synthesizer's command line."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('t2v_decoder_infer_steps_items', 't2v_decoder_infer_persistent_items', 't2v_bn_act_fwd_len', 't2v_mask_time')


def _prototypes():
    text = open(os.path.join(ROOT, 'include', 't2vae.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|long|void|size_t)\s+(t2v_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S):
        args = [a.strip() for a in m.group(2).split(',') if a.strip()]
        out[m.group(1)] = args
    return out


def test_new_exports_are_declared_with_the_bound_arity():
    import ctypes as C
    import t2v_hip
    protos = _prototypes()
    lib = t2v_hip.load_library()
    for name in NEW_EXPORTS:
        assert name in t2v_hip.EXPORTS, name
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(protos[name]), (name, protos[name])
    # the per-item entries take the arguments of the entries they extend, plus the t2v_dec_items pointer
    for new, old in (('t2v_decoder_infer_steps_items', 't2v_decoder_infer_steps'),
                     ('t2v_decoder_infer_persistent_items', 't2v_decoder_infer_persistent')):
        assert protos[new][:-2] == protos[old][:-1] and protos[new][-1] == protos[old][-1]
        assert 't2v_dec_items' in protos[new][-2]
        assert getattr(lib, new).argtypes[-2] == C.POINTER(t2v_hip._DecItems)
    # the existing decode entries keep their signatures
    assert len(protos['t2v_decoder_infer_steps']) == 11 and len(protos['t2v_decoder_infer_persistent']) == 9


def test_seed_reservation_equals_sequential_calls():
    import hparams as HP
    import model as M
    hp = HP.create_hparams()
    dec = M.Decoder(hp)
    dec._calls = 5
    want = [(int(hp.seed) * 1000003 + c) & 0x7FFFFFFFFFFFFFFF for c in (6, 7, 8)]
    assert [dec.call_seed(c) for c in (6, 7, 8)] == want
    assert dec.reserve_seeds(3) == want and dec._calls == 8
    assert dec.reserve_seeds(1) == [dec.call_seed(9)] and dec._calls == 9
    dec.dropout_seed = 2 ** 62
    s = dec.call_seed(1)
    assert 0 <= s <= 0x7FFFFFFFFFFFFFFF and s == (2 ** 62 * 1000003 + 1) & 0x7FFFFFFFFFFFFFFF


def test_cli_arguments(tmp_path):
    import synthesizer as S
    tf = tmp_path / 'texts.txt'
    tf.write_text("셋째\n\n넷째\n", encoding='utf-8')
    a = S.parse_args(['--load_path', 'ck', '--text', '첫째', '--text', '둘째', '--text_file', str(tf),
                      '--vocoder', 'griffin_lim', '--ratios', '0.5,0,0.5,0', '--batch_size', '3'])
    assert a.texts == ['첫째', '둘째', '셋째', '넷째']
    assert a.ratios == (0.5, 0.0, 0.5, 0.0) and a.batch_size == 3 and a.vocoder == 'griffin_lim'
    assert a.sample_path == 'samples' and a.ref_audio is None
    d = S.parse_args(['--load_path', 'ck', '--text', 'x'])
    assert d.batch_size == S.DEFAULT_BATCH_SIZE and d.vocoder is None and d.ratios == (1.0, 0.0, 0.0, 0.0)
    for bad in (['--load_path', 'ck'], ['--load_path', 'ck', '--text', 'x', '--ratios', '1,0'],
                ['--load_path', 'ck', '--text', 'x', '--vocoder', 'waveglow'],
                ['--load_path', 'ck', '--text', 'x', '--batch_size', '0']):
        with pytest.raises(SystemExit):
            S.parse_args(bad)


def test_lengths_are_rejected_in_training_mode():
    import torch
    import hparams as HP
    import model as M
    hp = HP.create_hparams()
    post, enc = M.Postnet(hp), M.Encoder(hp)
    with pytest.raises(RuntimeError):
        post(torch.zeros(2, 80, 8), torch.tensor([8, 5]))
    with pytest.raises(RuntimeError):
        enc.train().inference(torch.zeros(2, 512, 8), torch.tensor([8, 5]))
