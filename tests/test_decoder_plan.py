"""Engine selection of the teacher-forced decoder (DecoderCore.plan): pure host logic, checked on the CPU with the library's
shape queries stubbed.  The expected column was produced once by running the four per-engine predicates this function replaced
(and forward()'s all-chunks rule on top of them) over the same cases with the same stubs, so the table pins the rules as
they were, not as plan() happens to compute them."""
import pytest

ENV = ('T2V_TRAIN_PERSISTENT', 'T2V_BWD_PERSISTENT', 'T2V_PERSIST16', 'T2V_PERSIST16_BWD')


class StubLib:
    """The shape limits of the library's queries (fp32-weight kernels: 6 items; bf16 kernels: 16; forward and bf16 reverse pass
    up to 560 symbols, fp32 reverse pass up to 576; the bf16 reverse pass's exchange arrays reach 2^31 bytes at T_out = 3277)
    and scratch sizes that grow with T_out like the real ones, so that the 31-bit limits are met inside the table."""
    @staticmethod
    def t2v_decoder_train_persist_supported(B, T_in):
        return int(1 <= B <= 6 and 1 <= T_in <= 560)

    @staticmethod
    def t2v_decoder_train_persist16_supported(B, T_in):
        return int(1 <= B <= 16 and 1 <= T_in <= 560)

    @staticmethod
    def t2v_decoder_bwd_persist_supported(B, T_in):
        return int(1 <= B <= 6 and 1 <= T_in <= 576)

    @staticmethod
    def t2v_decoder_bwd_persist16_fits(B, T_in, T):
        return int(1 <= B <= 16 and 1 <= T_in <= 560 and 1 <= T < 3277)

    @staticmethod
    def t2v_decoder_train_persist_scratch_floats(B, T_in, T):
        return 50000 * T

    @staticmethod
    def t2v_decoder_train_persist16_scratch_floats(B, T_in, T):
        return 120000 * T

    @staticmethod
    def t2v_decoder_bwd_achain_scratch_floats(B, T_in, T):
        return 200000 * T


# ((DecoderCore.persistent, .persistent_bwd, .persistent16, environment, bf16_run, B, T_in, T, need_grad),
#  [(forward engine, reverse engine) of every chunk of <= 16 items])
TABLE = [
    ((None, None, None, {}, False, 6, 84, 400, True), [('persist', 'achain')]),
    ((None, None, None, {}, False, 6, 84, 400, False), [('persist', None)]),
    ((None, None, None, {}, False, 7, 84, 400, True), [('steps', 'steps')]),
    ((None, None, None, {}, False, 16, 84, 400, True), [('steps', 'steps')]),
    ((None, None, None, {}, False, 22, 84, 400, True), [('steps', 'steps'), ('persist', 'steps')]),
    ((None, None, None, {}, False, 38, 84, 40, True), [('steps', 'steps'), ('steps', 'steps'), ('persist', 'steps')]),
    ((None, None, None, {}, True, 16, 84, 400, True), [('persist16', 'persist16')]),
    ((None, None, None, {}, True, 7, 84, 400, True), [('persist16', 'persist16')]),
    ((None, None, None, {}, True, 6, 84, 400, True), [('persist', 'achain')]),
    ((None, None, 'force', {}, True, 6, 84, 400, True), [('persist16', 'persist16')]),
    ((None, None, 'force', {}, False, 6, 84, 400, True), [('persist', 'achain')]),
    ((None, None, False, {}, True, 16, 84, 400, True), [('steps', 'steps')]),
    ((None, None, False, {}, True, 6, 84, 400, True), [('persist', 'achain')]),
    ((False, None, None, {}, False, 6, 84, 400, True), [('steps', 'achain')]),
    ((False, None, None, {}, True, 16, 84, 400, True), [('steps', 'persist16')]),
    ((False, False, None, {}, False, 6, 84, 400, True), [('steps', 'steps')]),
    ((False, False, None, {}, True, 16, 84, 400, True), [('steps', 'steps')]),
    ((False, True, None, {}, True, 16, 84, 400, True), [('steps', 'persist16')]),
    ((False, True, None, {}, False, 6, 84, 400, True), [('steps', 'achain')]),
    ((True, False, None, {}, False, 6, 84, 400, True), [('persist', 'steps')]),
    ((True, False, None, {}, True, 16, 84, 400, True), [('persist16', 'steps')]),
    ((True, False, 'force', {}, True, 6, 84, 400, True), [('persist16', 'steps')]),
    ((None, None, None, {'T2V_TRAIN_PERSISTENT': '0'}, False, 6, 84, 400, True), [('steps', 'steps')]),
    ((None, None, None, {'T2V_TRAIN_PERSISTENT': '0'}, True, 16, 84, 400, True), [('steps', 'steps')]),
    ((None, None, None, {'T2V_TRAIN_PERSISTENT': '0', 'T2V_BWD_PERSISTENT': '1'}, False, 6, 84, 400, True), [('steps', 'achain')]),
    ((None, None, None, {'T2V_BWD_PERSISTENT': '0'}, False, 6, 84, 400, True), [('persist', 'steps')]),
    ((None, None, None, {'T2V_BWD_PERSISTENT': '0'}, True, 16, 84, 400, True), [('persist16', 'steps')]),
    ((True, None, None, {'T2V_TRAIN_PERSISTENT': '0'}, False, 6, 84, 400, True), [('persist', 'steps')]),
    ((None, None, None, {'T2V_PERSIST16': '0'}, True, 16, 84, 400, True), [('steps', 'steps')]),
    ((None, None, None, {'T2V_PERSIST16': '0'}, True, 6, 84, 400, True), [('persist', 'achain')]),
    ((None, None, 'force', {'T2V_PERSIST16': '0'}, True, 6, 84, 400, True), [('persist16', 'persist16')]),
    ((None, None, None, {'T2V_PERSIST16_BWD': '0'}, True, 16, 84, 400, True), [('persist16', 'steps')]),
    ((None, None, None, {'T2V_PERSIST16_BWD': '0'}, True, 6, 84, 400, True), [('persist', 'achain')]),
    ((None, None, 'force', {'T2V_PERSIST16_BWD': '0'}, True, 6, 84, 400, True), [('persist16', 'achain')]),
    ((None, None, None, {'T2V_PERSIST16_BWD': '0'}, True, 22, 84, 400, True), [('persist16', 'steps'), ('persist', 'steps')]),
    ((None, None, None, {}, True, 22, 84, 400, True), [('persist16', 'persist16'), ('persist', 'achain')]),
    ((None, None, None, {}, True, 32, 84, 400, True), [('persist16', 'persist16'), ('persist16', 'persist16')]),
    ((None, None, None, {}, True, 64, 84, 400, True), [('persist16', 'persist16'), ('persist16', 'persist16'), ('persist16', 'persist16'), ('persist16', 'persist16')]),
    ((None, None, None, {}, True, 70, 84, 400, False), [('persist16', None), ('persist16', None), ('persist16', None), ('persist16', None), ('persist', None)]),
    ((None, None, None, {}, False, 64, 84, 400, True), [('steps', 'steps'), ('steps', 'steps'), ('steps', 'steps'), ('steps', 'steps')]),
    ((None, None, None, {}, False, 20, 84, 400, True), [('steps', 'steps'), ('persist', 'steps')]),
    ((None, None, None, {}, False, 6, 560, 30, True), [('persist', 'achain')]),
    ((None, None, None, {}, False, 6, 561, 9, True), [('steps', 'achain')]),
    ((None, None, None, {}, False, 3, 576, 6, True), [('steps', 'achain')]),
    ((None, None, None, {}, False, 6, 577, 6, True), [('steps', 'steps')]),
    ((None, None, None, {}, True, 6, 576, 6, True), [('steps', 'achain')]),
    ((None, None, None, {}, True, 16, 560, 6, True), [('persist16', 'persist16')]),
    ((None, None, None, {}, True, 16, 561, 6, True), [('steps', 'steps')]),
    ((None, None, None, {}, True, 22, 570, 6, True), [('steps', 'steps'), ('steps', 'steps')]),
    ((None, None, 'force', {}, True, 6, 570, 6, True), [('steps', 'achain')]),
    ((None, None, None, {}, True, 16, 84, 3276, True), [('persist16', 'persist16')]),
    ((None, None, None, {}, True, 16, 84, 3277, True), [('persist16', 'steps')]),
    ((None, None, None, {}, True, 22, 84, 3277, True), [('persist16', 'steps'), ('persist', 'steps')]),
    ((None, None, None, {}, True, 16, 84, 4474, True), [('steps', 'steps')]),
    ((None, None, None, {}, False, 6, 84, 2684, True), [('persist', 'achain')]),
    ((None, None, None, {}, False, 6, 84, 2685, True), [('persist', 'steps')]),
    ((None, None, None, {}, False, 6, 84, 10738, True), [('steps', 'steps')]),
    ((None, None, None, {}, True, 6, 84, 2685, True), [('persist', 'persist16')]),
]


@pytest.mark.parametrize("case,expected", TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_plan_matches_the_rules_it_replaced(case, expected, monkeypatch):
    import t2v_hip as H
    persistent, persistent_bwd, persistent16, env, bf16, B, T_in, T, need_grad = case
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(H.DecoderCore, 'persistent', persistent)
    monkeypatch.setattr(H.DecoderCore, 'persistent_bwd', persistent_bwd)
    monkeypatch.setattr(H.DecoderCore, 'persistent16', persistent16)
    monkeypatch.setattr(H, '_BF16', bf16)
    plans = H.DecoderCore.plan(StubLib, B, T_in, T, need_grad)
    assert [(p.fwd, p.bwd) for p in plans] == expected
    # the chunks tile the batch in order, 16 items at a time
    assert [p.b0 for p in plans] == list(range(0, B, 16)) and [p.b1 for p in plans] == [min(B, b + 16) for b in range(0, B, 16)]
    # the preparation goes out behind the forward launch exactly when both passes of the chunk are persistent kernels
    assert [p.prepare for p in plans] == [f != 'steps' and r in ('achain', 'persist16') for f, r in expected]
    # all or nothing: one chunk on the launch-per-step reverse pass puts every chunk of the call there
    assert len({r == 'steps' for _, r in expected}) == 1


def test_plan_asks_nothing_about_the_reverse_pass_without_a_gradient():
    import t2v_hip as H

    class FwdOnly(StubLib):
        t2v_decoder_bwd_persist_supported = t2v_decoder_bwd_persist16_fits = t2v_decoder_bwd_achain_scratch_floats = None

    assert [(p.fwd, p.bwd, p.prepare) for p in H.DecoderCore.plan(FwdOnly, 6, 84, 400, False)][0][1:] == (None, False)
