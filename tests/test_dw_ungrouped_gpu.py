"""GPU parity of the LSTM weight gradients issued one by one (T2V_DW_GROUPED=0): the loop over DecoderCore._dw_groups' products, on
two chunks so that the second one accumulates, against torch.autograd on the oracle's decoder."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T_IN, T, LENS = 3, 20, 12, [20, 17, 9]
LSTM_WEIGHTS = ('attention_rnn.weight_ih', 'attention_rnn.weight_hh', 'decoder_rnn.weight_ih', 'decoder_rnn.weight_hh')


@pytest.fixture(scope='module')
def case():
    """the decoder, its inputs and the oracle's gradients of the four LSTM weights — made once, read by every test"""
    from test_decoder_gpu import _oracle, _setup
    hp, M, dec, memory, mels, lengths, wm, wg = _setup(B, T_IN, T, LENS)
    _, _, _, o_sd, _ = _oracle(dec, memory, mels, lengths, wm, wg)
    want = {n: o_sd['decoder.' + n].grad.clone() for n in LSTM_WEIGHTS}
    return dec.state_dict(), memory, mels, lengths, wm, wg, want


def _forward_unfolded(dec, memory, decoder_inputs, memory_lengths):
    """Decoder.forward with the Prenet term of attention_rnn's gates made OUTSIDE the node (DecoderCore's gpre argument, pre=None):
    the Prenet columns of attention_rnn.weight_ih then get their gradient through gpre, not from the node's third product"""
    import t2v_hip
    from model import lengths_i32
    frames = dec.parse_decoder_inputs(decoder_inputs)
    x = torch.cat((dec.get_go_frame(memory).unsqueeze(0), frames), 0)
    pre = dec.prenet(x[:frames.size(0)], None)
    att = dec.attention_rnn
    gpre = pre @ att.weight_ih[:, :dec.prenet_dim].t() + att.bias_ih + att.bias_hh
    lin = t2v_hip.LinearHIP.apply
    pm = lin(memory, dec.attention_layer.memory_layer.weight, None, False, 0.0, 0, 0, 0)
    b_dec, w81, b81 = dec._param_operands()
    hc, _ = t2v_hip.DecoderCore.apply(gpre, memory, pm, lengths_i32(memory_lengths, memory.device), *dec._core_weights(b_dec),
                                      0.0, 0.0, 0, True)
    out = lin(hc, w81, b81, False, 0.0, 0, 0, 0)
    return out[..., :dec.n_mel_channels].permute(1, 2, 0), out[..., dec.n_mel_channels].transpose(0, 1)


@pytest.mark.parametrize("folded", [False, True], ids=['gpre', 'prenet-folded'])
@pytest.mark.parametrize("grouped", ['0', None], ids=['one-by-one', 'grouped'])
def test_lstm_weight_gradients_one_by_one_match_the_oracle(case, monkeypatch, grouped, folded):
    """launch-per-step passes on chunks of 2 + 1 items; the tolerance is test_decoder_gpu.py's for every gradient: 2e-3 of the
    tensor's largest entry"""
    import hparams as HP
    import model as M
    import t2v_hip
    sd, memory, mels, lengths, wm, wg, want = case
    monkeypatch.setattr(M, 'drop_rate', 0.0)
    monkeypatch.setattr(t2v_hip, 'MAX_DEC_B', 2)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent', False)
    monkeypatch.setattr(t2v_hip.DecoderCore, 'persistent_bwd', False)
    if grouped is None:
        monkeypatch.delenv('T2V_DW_GROUPED', raising=False)
    else:
        monkeypatch.setenv('T2V_DW_GROUPED', grouped)
    dev = torch.device('cuda:0')
    dec = M.Decoder(HP.create_hparams())
    dec.load_state_dict(sd)
    dec = dec.to(dev).train()
    dec.p_attention_dropout = dec.p_decoder_dropout = 0.0
    mem = memory.to(dev).requires_grad_(True)
    if folded:
        mel, gate, _ = dec(mem, mels.to(dev), lengths.to(dev))
    else:
        mel, gate = _forward_unfolded(dec, mem, mels.to(dev), lengths.to(dev))
    ((mel * wm.to(dev)).sum() + (gate * wg.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    t2v_hip.check_async_errors()
    assert t2v_hip.DecoderCore.chunk_bwd_kernels == ['k_lstm_bwd256 + k_attn_cell_bwd'] * 2
    params = dict(dec.named_parameters())
    for name in LSTM_WEIGHTS:
        d = (params[name].grad.cpu() - want[name]).abs().max().item()
        s = want[name].abs().max().item()
        print(name, 'max |diff| %.3e of max |grad| %.3e' % (d, s))
        assert s > 0 and d / (s + 1e-6) < 2e-3, (name, d, s)
