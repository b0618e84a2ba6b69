"""tests/gemm_ref.py can tell a right GEMM from a subtly wrong one, for every case tests/test_gemm_routes_gpu.py runs (no GPU: the
route query is host code, everything else is torch on the CPU):

  (a) two honest fp32 results — one torch product, and k summed in tiles of 32 with the partial sums added in split order — pass the
      element-wise bound and the 0.1 % cap on excused ReLU / keep decisions;
  (b) every mutation of the oracle that can touch the case (a lost k, k-tail, row, column or k-split, the bias added once per split,
      ReLU before `accumulate`, the dropout index on N instead of ldc, the bias by row, bf16 by truncation) moves the honest result
      at least 8 bounds away — an empty trailing split excepted, whose loss must move nothing;
  and the table itself: the route query answers what each case expects, every route is reached, every mutation applies somewhere."""
import collections

import pytest
import torch

import gemm_ref as G

IDS = [c.name for c in G.CASES]
_SEEN = collections.defaultdict(set)          # mutation -> cases it was applied to; filled by the parametrised test


@pytest.fixture(scope='module')
def routes():
    """case name -> (route, form, splits, k per split) from t2v_gemm_route, cases behind a process switch asked in one child"""
    import t2v_hip
    lib = t2v_hip.load_library()
    out = {}
    prev = lib.t2v_gemm_f32_set_mode(-1)
    try:
        for c in G.CASES:
            if not c.env:
                lib.t2v_gemm_f32_set_mode(c.x3)
                out[c.name] = G.ask_route(lib, c)
    finally:
        lib.t2v_gemm_f32_set_mode(prev)
    envs = sorted(set(c.env for c in G.CASES if c.env))
    for env in envs:
        out.update(G.routes_in_child([c for c in G.CASES if c.env == env], env))
    return out


def test_route_query_answers_what_the_table_expects_and_every_route_is_reached(routes):
    import t2v_abi
    abi = t2v_abi.load()
    assert [abi.define('T2V_GEMM_ROUTE_' + r.upper()) for r in G.ROUTES] == list(range(abi.define('T2V_GEMM_ROUTES')))
    for c in G.CASES:
        route, form, splits, kps = routes[c.name]
        assert route == c.route, (c.name, route)
        assert (splits > 1) == route.endswith('_splitk') or route in ('f32_x3', 'bf16_planes'), (c.name, splits)
        assert c.splits is None or splits == c.splits, (c.name, splits)
        assert kps == c.K if splits == 1 else (splits - 1) * kps < c.K or route == 'f32_64_splitk', (c.name, splits, kps)
        if c.a != 's' and not route.startswith('bf16_big'):
            assert form == (c.a == 'k') + 2 * (c.b == 'k'), (c.name, form)
    assert set(r[0] for r in routes.values()) == set(G.ROUTES)
    # the fp32 64x64 split-K keeps its grid: 1100 = 6 x 160 + 140, the eighth split starts past K
    r = routes['f32_64_splitk_kr_65x33x1100_nobias']
    assert r[2:] == (8, 160) and 7 * 160 > 1100
    # in the default environment the one-plane route takes every product the 128x128 bf16 kernel would split
    c = G.BY_NAME['bf16_big_splitk_rr_1024x1024x1056']
    import t2v_hip
    assert G.ask_route(t2v_hip.load_library(), c)[0] == 'bf16_planes'


@pytest.mark.parametrize('name', IDS)
def test_honest_results_pass_and_mutations_fail(routes, name):
    c = G.BY_NAME[name]
    route, form, splits, kps = routes[name]
    inp = G.inputs(c)
    orc = G.oracle(c, inp)
    for how in ('torch', 'tiles'):
        v = G.judge(c, G.emulate(c, inp, how, splits, kps), orc)
        print(G.table_line(c, route + ':' + how, form, splits, v))
        assert v.ok, (how, v)
    honest = G.emulate(c, inp, 'tiles', splits, kps)
    for m in G.applicable(c, splits):
        drops = range(splits) if m == 'split_dropped' else (0,)
        for z in drops:
            v = G.judge(c, honest, G.oracle(c, inp, m, splits, kps, z))
            factor = v.worst / v.bound
            print('    %-24s%s  %.1f bounds' % (m, ' z=%d' % z if m == 'split_dropped' else '', factor))
            if m == 'split_dropped' and z * kps >= c.K:
                assert v.ok, (m, z, v)                    # an empty split: nothing to lose
                _SEEN['empty_split'].add(name)
            else:
                assert factor >= G.MUTATION_FACTOR and not v.ok, (m, z, factor)
        _SEEN[m].add(name)


def test_every_mutation_applies_to_some_case(routes):
    for c in G.CASES:          # (also when this test runs alone)
        _SEEN['empty_split' if (routes[c.name][2] - 1) * routes[c.name][3] >= c.K else '-'].add(c.name)
        for m in G.applicable(c, routes[c.name][2]):
            _SEEN[m].add(c.name)
    for m in G.MUTATIONS:
        assert _SEEN[m], m
    assert _SEEN['empty_split']
    # ... and to a case of every route it can mean something on
    for route in G.ROUTES:
        muts = set(m for c in G.CASES if c.route == route for m in G.applicable(c, routes[c.name][2]))
        assert {'last_k', 'last_row', 'last_col'} <= muts, route
        assert ('bf16_truncated' in muts) == (route.startswith('bf16') and route != 'bf16_to_f32_big'), route
        assert ('split_dropped' in muts) == any(routes[c.name][2] > 1 for c in G.CASES if c.route == route), route


def test_layouts_hold_the_logical_operands():
    c = G.BY_NAME['f32_64_strided_65x33x33']
    inp = G.inputs(c)
    for x, form, pad, off in ((inp.A, c.a, c.a_pad, c.a_off), (inp.B, c.b, c.b_pad, c.b_off)):
        v = G.place(x, form, pad, off)
        assert torch.equal(v, x) and v.stride() == G.layout(form, x.shape[0], x.shape[1], pad) and v.storage_offset() == off
        assert v.stride(0) != 1 and v.stride(1) != 1
    v = G.place(inp.A, 'r', 3, 0)
    assert v.stride() == (1, 68) and torch.equal(v, inp.A)


def test_rounding_is_bf16_refs_and_the_bound_is_the_projects():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9])
    assert G.rounding(G.BY_NAME['bf16_64_kk_64x64x32']) is G.bf16_ref.rne and G.rounding(G.BY_NAME['f32_64_kk_64x64x32']) is G.bf16_ref.identity
    assert G.rounding(G.BY_NAME['bf16_to_f32_big_kk_1924x1028x36']) is G.bf16_ref.identity
    assert G.bf16_ref.rne(x).tolist() == [1.0, 1.0 + 2.0 ** -7] and G.bf16_ref.truncate(x).tolist() == [1.0, 1.0]      # a tie to even, a round up
    assert G.bound(1) == 8e-7 and G.bound(16) == 8e-7 and abs(G.bound(548) - 2e-7 * 548 ** 0.5) < 1e-18
