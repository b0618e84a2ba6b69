"""Host-side helper entry points of the C ABI (no kernel is launched, no GPU needed but by the one test marked `gpu`): the geometry
answers the Python mirror sizes its buffers with must stay consistent with what the launches use."""
import ctypes as C
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    import t2v_hip
    return t2v_hip.load_library()


def test_conv_stat_blocks_follow_the_tile_choice(lib):
    # encoder bank (6 x 84 positions): 48-position tiles with the input channels cut in two -> 2 tiles per item
    assert lib.t2v_conv1d_stat_blocks(6, 84, 512, 512, 5) == 12
    # Postnet (6 x 400): 80-position tiles, no split
    assert lib.t2v_conv1d_stat_blocks(6, 400, 512, 512, 5) == 30
    # generic kernel (Cin not a multiple of 16): 64 output positions per block over the flattened batch
    assert lib.t2v_conv1d_stat_blocks(2, 129, 33, 70, 3) == (2 * 129 + 63) // 64


@pytest.fixture(scope="module")
def conv_geometry(golden_dir):
    """(tools/record_conv_geometry.py as a module, the answers it recorded from a build of before the conv routing changed)"""
    path = os.path.join(os.path.dirname(os.path.dirname(golden_dir)), 'tools', 'record_conv_geometry.py')
    spec = importlib.util.spec_from_file_location('record_conv_geometry', path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(golden_dir, 'conv_geometry.json')) as f:
        return tool, json.load(f)


def test_conv_geometry_answers_are_the_recorded_ones(lib, conv_geometry):
    # x3 mode 0: the tiled and the generic kernels, 1000 shapes around every tile rule.  Exact
    tool, golden = conv_geometry
    assert golden['columns'] == tool.COLUMNS and len(golden['mode0']) == len(tool.MODE0_SHAPES) == 1000
    mode = lib.t2v_conv1d_x3_set_mode(-1)
    got = tool.section(lib, 'mode0')
    assert lib.t2v_conv1d_x3_set_mode(-1) == mode
    bad = [(g, w) for g, w in zip(got, golden['mode0']) if g != w]
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_conv_x3_eligibility_is_the_recorded_one(lib, conv_geometry):
    # x3 modes 1 and 2 ask for the library's plane ring: recorded on the MI355X.  Exact
    tool, golden = conv_geometry
    got = tool.section(lib, 'x3')
    for mode in ('1', '2'):
        assert len(golden['x3'][mode]) == len(tool.X3_SHAPES) == 45
        bad = [(g, w) for g, w in zip(got[mode], golden['x3'][mode]) if g != w]
        assert not bad, (mode, bad[:5])
    assert any(r[8] for r in golden['x3']['1']) and any(r[9] for r in golden['x3']['2'])    # (the section does see the plane kernels)


def test_reverse_pass_geometry(lib):
    assert lib.t2v_decoder_bwd_persist_slices(84) == 6 and lib.t2v_decoder_bwd_persist_slices(224) == 7
    assert lib.t2v_decoder_bwd_persist_supported(7, 84) == 0 and lib.t2v_decoder_bwd_achain_dq_offset(7, 84, 400) == -1
    if lib.t2v_decoder_bwd_persist_supported(6, 84) == 1:        # asks the device for its CU count: 0 on a machine without one
        off = lib.t2v_decoder_bwd_achain_dq_offset(6, 84, 400)
        total = lib.t2v_decoder_bwd_achain_scratch_floats(6, 84, 400)
        assert off > 0 and off % 4 == 0 and off + 400 * 6 * 128 <= total      # the summed-dq rows lie inside the scratch
    else:
        assert lib.t2v_decoder_bwd_achain_dq_offset(6, 84, 400) == -1


# the cooperative recurrences: (entry point, number of pointer arguments, indices of the optional ones).  Every call below must be
# turned away by the argument guard, before anything is launched: the pointers are host dummies.
_RECURRENT = (('t2v_bilstm_fwd', 8, (4, 5)), ('t2v_bilstm_bwd', 8, ()), ('t2v_gru_fwd', 7, (4,)), ('t2v_gru_fwd_len', 9, (4,)),
              ('t2v_gru_bwd', 8, ()))


@pytest.mark.parametrize("name,n_ptr,optional", _RECURRENT, ids=[r[0] for r in _RECURRENT])
def test_recurrent_entry_points_turn_bad_arguments_away(lib, name, n_ptr, optional):
    fn = getattr(lib, name)
    dummy = C.create_string_buffer(64)
    ptrs = [C.c_void_p(C.addressof(dummy))] * n_ptr
    for B, T in ((0, 4), (17, 4), (-1, 4), (4, 0), (4, -3)):
        assert fn(*ptrs, B, T, None) != 0, (B, T)
    for i in range(n_ptr):
        if i not in optional:
            assert fn(*(ptrs[:i] + [None] + ptrs[i + 1:]), 4, 4, None) != 0, i


def test_bilstm_fwd_wants_gates_and_cells_together(lib):
    dummy = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(dummy))
    assert lib.t2v_bilstm_fwd(p, p, p, p, p, None, p, p, 4, 4, None) != 0          # gates without cells
    assert lib.t2v_bilstm_fwd(p, p, p, p, None, p, p, p, 4, 4, None) != 0          # cells without gates


def test_scratch_size_answers_are_monotonic(lib):
    assert lib.t2v_gemm_splitk_scratch_floats(81, 1536, 2400) > 0            # the projection's weight gradient is split
    # large products: no scratch for the fp32-MFMA kernels; the x3 path (round 6) keeps the bf16 planes of both operands there
    # (6 bytes per element, padded to whole tiles) + the raw tiles of its k-splits
    prev = lib.t2v_gemm_f32_set_mode(0)
    try:
        assert lib.t2v_gemm_splitk_scratch_floats(4096, 2560, 2400) == 0
        lib.t2v_gemm_f32_set_mode(1)
        planes = 6 * (4096 + 2560) * 2400 // 4
        got = lib.t2v_gemm_splitk_scratch_floats(4096, 2560, 2400)
        assert planes <= got <= planes + 4 * 4096 * 2560
        assert lib.t2v_gemm_splitk_scratch_floats(81, 1536, 2400) > 0 and lib.t2v_gemm_splitk_scratch_floats(128, 128, 2400) > 0   # small: fp32 split-K
    finally:
        lib.t2v_gemm_f32_set_mode(prev)
    assert lib.t2v_colsum_scratch_floats(2400, 4096) >= 4096 and lib.t2v_colsum_scratch_floats(1, 7) == 0
    a, b = lib.t2v_decoder_train_persist_scratch_floats(6, 84, 100), lib.t2v_decoder_train_persist_scratch_floats(6, 84, 400)
    assert 0 < a < b
