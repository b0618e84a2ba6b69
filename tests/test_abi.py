"""The ctypes binding is derived from include/t2vae.h by t2v_abi.py (no GPU, no kernel launch): the derived types against
expectations written by hand from the header, the struct layouts against a C compiler, what the parser refuses, the
limits t2v_hip.py takes from the header, and that every declared entry point is bound."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import t2v_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 't2vae.h')
PKG = os.path.join(ROOT, 'tacotron2-vae_amd')


def test_abi_module_is_pure_python_and_finds_the_header():
    tree = ast.parse(open(os.path.join(PKG, 't2v_abi.py')).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name.split('.')[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or '').split('.')[0])
    assert mods <= {'re', 'os', 'ctypes'}, mods
    assert os.path.samefile(t2v_abi.HEADER, HEADER)
    assert t2v_abi.load() is t2v_abi.load()                 # parsed once per process


def _expected():
    """(restype, argtypes) written by hand from the prototypes of include/t2vae.h; shares nothing with the parser.  Together:
    every row of the type table (by value, or as a pointee where the header has it no other way), a void and a char* return,
    device pointers, the device-side struct pointer, POINTER(struct) of host structs, both two-star forms."""
    import t2v_hip as H
    i, l, f, vp = C.c_int, C.c_long, C.c_float, C.c_void_p
    u32, u64, P = C.c_uint32, C.c_uint64, C.POINTER
    return {
        't2v_version': (C.c_char_p, []),
        't2v_set_step_params': (None, [vp]),                                  # const t2v_step_params*: a device record
        't2v_stamp': (i, [vp, i, vp]),                                        # unsigned long long*
        't2v_decoder_qp_floats': (l, [i, i]),
        't2v_conv1d_staged_launches': (C.c_longlong, []),
        't2v_conv1d_takes_x3': (i, [i] * 6),
        't2v_bn_act_slices': (i, [i] * 6),
        't2v_istft_scratch_bytes': (C.c_size_t, [i, i]),
        't2v_gemm_epilogue_bwd': (i, [vp, vp, vp, C.c_size_t, f, vp]),
        't2v_gemm_f32': (i, [vp, l, l, vp, l, l, vp, vp, i, i, i, i, i, i, f, u64, u32, u32, vp]),
        't2v_alignment_stats': (i, [vp, C.c_longlong, C.c_longlong, vp, vp, i, i, i, i, f, vp, i, vp, i, vp, vp, vp, vp]),
        't2v_loudness': (i, [vp, vp, i, i, vp, i, vp, i, vp, i, vp, vp, vp]),             # const double* table
        't2v_stft_polar': (i, [vp, vp, i, i, i, i, vp, vp, vp, vp, vp, i, vp]),           # const int64_t* n_samples
        't2v_gather_words': (i, [P(vp), P(vp), i, vp]),                       # const void* const*, void* const*
        't2v_conv1d_flip_weights': (i, [vp, vp, vp, vp, i, i, vp]),           # const float* const*: a typed two-star stays a pointer
        't2v_gemm_f32_grouped': (i, [P(H._GemmGroup), i, i, i, i, vp, vp]),
        't2v_gemm_route': (i, [i, i, i, l, l, l, l, i, i, i, i, i, f, i, vp, vp, vp]),   # int* form, splits, k_per_split: host words
        't2v_gemm_route_name': (C.c_char_p, [i]),
        't2v_conv1d_route': (i, [i] * 8 + [vp] * 8),                          # eight int* outputs: host words
        't2v_conv1d_route_name': (C.c_char_p, [i]),
        't2v_decoder_infer_persistent_window': (i, [P(H._DecPersistWeights), P(H._DecPersistBufs), i, i, i, f, f, u64,
                                                    P(H._DecItems), P(H._DecWindow), vp]),
        't2v_clip_adam_step_guarded': (i, [vp, vp, vp, vp, u64] + [f] * 9 + [vp, vp, vp, i, vp]),
    }


def test_derived_types_equal_a_hand_written_expectation_object_for_object():
    import t2v_hip
    protos = t2v_abi.load().prototypes
    lib = t2v_hip.load_library()
    for name, (restype, argtypes) in _expected().items():
        for got_res, got_args in (protos[name], (getattr(lib, name).restype, getattr(lib, name).argtypes)):
            assert got_res is restype, (name, got_res, restype)
            assert len(got_args) == len(argtypes), (name, len(got_args), len(argtypes))
            for k, (a, b) in enumerate(zip(got_args, argtypes)):
                assert a is b, (name, k, a, b)


def test_structure_classes_keep_their_names_and_field_types():
    import t2v_hip as H
    abi = t2v_abi.load()
    names = ('_DecWeights', '_DecTrainBufs', '_DecBwdBufs', '_DecPersistWeights', '_DecPersistBufs', '_DecTrainPersistWeights',
             '_GemmGroup', '_AchainDw', '_DecInferBufs', '_DecItems', '_DecWindow')
    assert sorted(t2v_abi.HOST_STRUCTS.values()) == sorted(names)
    assert len(abi.layouts) == 12 and set(abi.layouts) == set(t2v_abi.HOST_STRUCTS) | {'t2v_step_params'}
    for c_name, py_name in t2v_abi.HOST_STRUCTS.items():
        cls = getattr(H, py_name)
        assert cls is abi.classes[c_name] and cls.__name__ == py_name and cls.C_NAME == c_name
        assert cls._fields_ == abi.layouts[c_name]
    # scalar field types, by hand from the header
    assert H._DecWeights._fields_[-1] == ('packs_bf16', C.c_int32) and all(t is C.c_void_p for _, t in H._DecWeights._fields_[:-1])
    assert H._AchainDw._fields_ == [('planes', C.c_void_p), ('d_w_ih', C.c_void_p), ('ld_ih', C.c_int), ('d_w_hh', C.c_void_p),
                                    ('ld_hh', C.c_int), ('accumulate', C.c_int), ('tile_cap', C.c_int)]
    g = dict(H._GemmGroup._fields_)
    assert [n for n, _ in H._GemmGroup._fields_] == ['A', 'sAi', 'sAk', 'nb', 'B', 'sBj', 'sBk', 'N', 'C', 'ldc']
    assert g['A'] is C.c_void_p and g['sAi'] is C.c_long and g['sAk'] is C.c_long and g['nb'] is C.c_int
    for n, t in (('B', C.c_void_p), ('sBj', C.c_long), ('sBk', C.c_long), ('N', C.c_int), ('C', C.c_void_p), ('ldc', C.c_int)):
        assert issubclass(g[n], C.Array) and g[n]._type_ is t and g[n]._length_ == 3, n
    assert abi.layouts['t2v_step_params'][0] == ('epoch', C.c_uint64)
    assert H._ARENA == tuple(n for n, _ in H._DecTrainBufs._fields_) and H._ARENA[0] == 'gpre' and H._ARENA[-1] == 'S'


def test_step_params_slots_come_from_the_record_layout():
    import t2v_hip
    assert t2v_hip.StepParams.SLOTS == {'lr': 2, 'bc1': 3, 'bc2s': 4, 'kl_weight': 5}       # the header's 32-byte record
    assert t2v_hip.StepParams.WORDS == 8
    assert not hasattr(t2v_hip.StepParams, 'FIELDS')


def _compiler():
    for cc in ('cc', 'gcc', 'clang', '/opt/rocm/llvm/bin/clang'):
        path = shutil.which(cc)
        if path:
            return path
    return None


def test_struct_layouts_equal_what_a_c_compiler_lays_out(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip('no C compiler (cc, gcc, clang) on this machine')
    abi = t2v_abi.load()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "t2vae.h"', 'int main(void) {']
    for s, fields in abi.layouts.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for n, _ in fields:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, n, s, n, s, n))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run([cc, '-x', 'c', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, timeout=60, stdout=subprocess.PIPE).stdout.decode().split('\n')
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out if ln.strip()}
    checked = 0
    for s, fields in abi.layouts.items():
        cls = abi.classes[s]
        assert got[s] == (C.sizeof(cls),), (s, got[s], C.sizeof(cls))
        for n, _ in fields:
            d = getattr(cls, n)
            assert got['%s.%s' % (s, n)] == (d.offset, d.size), (s, n, got['%s.%s' % (s, n)], d.offset, d.size)
            checked += 1
    assert len(got) == checked + len(abi.layouts) and checked > 100
    assert got['t2v_step_params'] == (32,) and got['t2v_step_params.pad'] == (24, 8)
    assert got['t2v_gemm_group.B'][1] == 3 * C.sizeof(C.c_void_p) and got['t2v_gemm_group.N'][1] == 12


def test_parser_refuses_what_it_does_not_know(tmp_path):
    E = t2v_abi.T2VHipError
    ok = 'int t2v_fine(const float* x, long n, void* stream);\n'
    assert list(t2v_abi.Abi(ok).prototypes) == ['t2v_fine']
    with pytest.raises(E, match=r't2v_foo.*widget_t'):
        t2v_abi.Abi(ok + 'int t2v_foo(const float* x, widget_t w, void* stream);\n')
    with pytest.raises(E, match=r't2v_dec_window\.ahead'):
        t2v_abi.Abi('typedef struct t2v_dec_window {\n    int32_t back;\n    gizmo_t ahead;\n} t2v_dec_window;\n' + ok)
    with pytest.raises(E, match='t2v_unlisted'):                # a struct nobody named: host-filled or a device record?
        t2v_abi.Abi('typedef struct t2v_unlisted { int a; } t2v_unlisted;\n' + ok)
    with pytest.raises(E, match='t2v_byvalue'):
        t2v_abi.Abi('typedef struct t2v_dec_window { int32_t back; int32_t ahead; } t2v_dec_window;\n'
                    'int t2v_byvalue(t2v_dec_window w);\n')
    with pytest.raises(E, match='t2v_ret'):
        t2v_abi.Abi('float* t2v_ret(int n);\n')
    with pytest.raises(E, match='t2v_bar'):                     # a t2v_*( that is no prototype
        t2v_abi.Abi(ok + 'static int y = t2v_bar(1);\n')
    with pytest.raises(E, match='t2v_fine'):
        t2v_abi.Abi(ok + ok)
    abi = t2v_abi.Abi('#define T2V_OK 0\n#define T2V_NEG -3\n#define T2V_BIG (1 << 20)   /* c */\n#define T2V_RATE 0.5f\n'
                      '#define T2V_SUM (T2V_OK + 1)\n#define T2V_GUARD\n' + ok)
    assert abi.defines == {'T2V_OK': 0, 'T2V_NEG': -3, 'T2V_BIG': 1048576} and abi.define('T2V_BIG') == 1 << 20
    for bad in ('T2V_RATE', 'T2V_SUM', 'T2V_GUARD', 'T2V_NOWHERE'):
        with pytest.raises(E, match=bad):
            abi.define(bad)
    missing = str(tmp_path / 'nowhere' / 't2vae.h')
    with pytest.raises(E, match='nowhere'):
        t2v_abi.load(missing)


CONSTANTS = ('DTW_MAX_FRAMES', 'NCEP', 'F0_MAX_LAG', 'RESAMPLE_MAX_TAPS', 'TSM_MAX_RATIO', 'TSM_MAX_FRAMES', 'ENV_MAX_ORDER',
             'ENV_MAX_ITERS', 'LOUDNESS_CHUNK', 'LOUDNESS_TILE', 'ALIGN_FRAMES', 'TSNE_MAX_POINTS', 'TSNE_EXAG_ITERS',
             'LATENT_MAX_POINTS', 'LATENT_MAX_CLASSES', 'LATENT_MAX_K', 'LATENT_TILE')


def test_limits_come_from_the_header_and_no_copy_is_left():
    import t2v_hip
    abi = t2v_abi.load()
    for n in CONSTANTS:
        v = getattr(t2v_hip, n)
        assert type(v) is int and v == abi.define('T2V_' + n), n
    assert t2v_hip.TSM_MAX_FRAMES == 1048576 and t2v_hip.DTW_MAX_FRAMES == 2048 and t2v_hip.NCEP == 13      # as the header reads
    assert abi.define('T2V_ERR_LAUNCH') == -3
    src = open(os.path.join(PKG, 't2v_hip.py')).read().split('\n')
    for ln in src:
        assert not re.search(r'= \d+\s+# T2V_\w+ of include/t2vae.h', ln), ln
        # nor a hand-written binding line, field list or slot table
        assert not re.search(r'\.t2v_\w+\.(argtypes|restype)\b', ln) and 'C.Structure' not in ln and 'FIELDS' not in ln, ln


def test_every_declared_entry_point_is_a_parsed_prototype_in_header_order():
    import t2v_hip
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    seen = re.findall(r'\b(t2v_\w+)\s*\(', text)
    protos = t2v_abi.load().prototypes
    assert seen == list(protos) and len(seen) == len(set(seen)) >= 144
    assert t2v_hip.EXPORTS == tuple(seen) and 't2v_conv1d_takes_x3' in t2v_hip.EXPORTS and 't2v_bn_act_slices' in t2v_hip.EXPORTS
    assert 't2v_gemm_route' in t2v_hip.EXPORTS and 't2v_gemm_route_name' in t2v_hip.EXPORTS
    assert 't2v_conv1d_route' in t2v_hip.EXPORTS and 't2v_conv1d_route_name' in t2v_hip.EXPORTS
    lib = t2v_hip.load_library()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
