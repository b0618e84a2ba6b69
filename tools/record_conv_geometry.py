#!/usr/bin/env python
"""Write tests/golden/conv_geometry.json: what the library answers about the geometry of its Conv1d launches (test infrastructure).

    python tools/record_conv_geometry.py [--sections mode0,x3] [--out FILE]

Host queries only, no kernel is launched.  T2V_LIB selects the library: the file pins the answers of a KNOWN-GOOD build (the
parent of a change of the conv routing), so record it from that build and never from the tree under test;
tests/test_abi_helpers.py and tests/test_conv_bn_gpu.py recompute both sections and compare exactly.

Sections (a section that is not asked for is kept as the file has it):
    mode0   t2v_conv1d_x3_set_mode(0), restored afterwards: the tiled and the generic kernels.  Needs no device.
            B in {1, 2, 6, 16, 64} x T in {1, 37, 84, 400, 1153} x Cin in {16, 33, 80, 272, 512} x Cout in {64, 70, 80, 512} x KS in {3, 5}
    x3      modes 1 and 2, KS = 5, Cin, Cout in {64, 80, 512}, (B, T) in {(1, 37), (6, 84), (6, 400), (16, 400), (64, 1153)}.
            Asks whether the library's plane ring is there: needs the MI355X.
Row: [B, T, Cin, Cout, KS, stat_blocks, stat_blocks_bf16, dw_scratch_floats, takes_x3 (fp32), takes_x3 (bf16)]
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ['B', 'T', 'Cin', 'Cout', 'KS', 'stat_blocks', 'stat_blocks_bf16', 'dw_scratch_floats', 'takes_x3', 'takes_x3_bf16']
MODE0_SHAPES = [(B, T, Cin, Cout, KS) for B, T, Cin, Cout, KS in
                itertools.product((1, 2, 6, 16, 64), (1, 37, 84, 400, 1153), (16, 33, 80, 272, 512), (64, 70, 80, 512), (3, 5))]
X3_SHAPES = [(B, T, Cin, Cout, 5) for (B, T), Cin, Cout in
             itertools.product(((1, 37), (6, 84), (6, 400), (16, 400), (64, 1153)), (64, 80, 512), (64, 80, 512))]


def rows(lib, mode, shapes):
    """the answers under t2v_conv1d_x3_set_mode(mode); the mode the process had is restored"""
    prev = lib.t2v_conv1d_x3_set_mode(mode)
    try:
        return [[B, T, Cin, Cout, KS,
                 lib.t2v_conv1d_stat_blocks(B, T, Cin, Cout, KS), lib.t2v_conv1d_stat_blocks_bf16(B, T, Cin, Cout, KS),
                 lib.t2v_conv1d_dw_scratch_floats(B, Cin, T, Cout, KS),
                 lib.t2v_conv1d_takes_x3(B, Cin, T, Cout, KS, 0), lib.t2v_conv1d_takes_x3(B, Cin, T, Cout, KS, 1)]
                for B, T, Cin, Cout, KS in shapes]
    finally:
        lib.t2v_conv1d_x3_set_mode(prev)


def section(lib, name):
    if name == 'mode0':
        return rows(lib, 0, MODE0_SHAPES)
    if name == 'x3':
        return {str(mode): rows(lib, mode, X3_SHAPES) for mode in (1, 2)}
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sections', default='mode0,x3')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'conv_geometry.json'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))
    import t2v_hip
    lib = t2v_hip.load_library()
    doc = {}
    if os.path.isfile(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc['columns'] = COLUMNS
    for name in args.sections.split(','):
        doc[name] = section(lib, name)
    with open(args.out, 'w') as f:          # one row per line
        f.write(json.dumps(doc, separators=(',', ':')).replace('[[', '[\n[').replace('],[', '],\n[').replace(']]', ']\n]') + '\n')
    print('wrote', args.out, 'from', t2v_hip.lib_path())


if __name__ == '__main__':
    main()
