"""gnn_loop_set_gather_form: the full-tile kernel walking the CSR (form 1) and reading the graph's gather program (form 2) evaluate every
row's fmaf chain in the same order - k, states and outputs identical bit for bit, in both arithmetic modes and both piece formats; the exact
path is the C oracle's.  State width 64 throughout (the full-tile kernel), graphs of 64 to 4,096 nodes."""
import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from test_gather_program import csr_from_degrees, hand_built_degrees
from util import make_mlp

pytestmark = pytest.mark.gpu

DS, NL = 64, 3
MODES = [(1, 2), (2, 2), (2, 3)]          # (impl, piece format)


def _engine():
    from GNN import _engine
    return _engine


def graph_from_degrees(rng, deg):
    """Oracle graph dict whose row r has deg[r] entries (sources ascending), with a distinct weight on every entry: any reordering within
    a row changes the low bits of its aggregate."""
    n = len(deg)
    indptr, src, w = csr_from_degrees(rng, deg, n)
    dst = np.repeat(np.arange(n), deg)
    arcs = np.stack([src, dst, 2 * rng.random(src.size) - 1], 1).astype(np.float32)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    g = orc.make_graph_dict(arcs, (2 * rng.random((n, NL)) - 1).astype(np.float32), 'average')
    assert np.array_equal(g['adjT'][0], indptr) and np.array_equal(g['adjT'][1], src)
    g['adjT'] = (g['adjT'][0], g['adjT'][1], w)
    return g


def nets(rng, nl=NL, hidden=(128, 128), gain=0.6):
    st = make_mlp(rng, 1 + 2 * (DS + nl), list(hidden) + [DS], 'selu', gain=gain, bn_random=True)
    ou = make_mlp(rng, DS + nl, [2], 'softmax', bn_random=True)
    return st, ou


def device_graph(e, g, **kw):
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    return e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'],
                   np.logical_and(g['set_mask'], g['output_mask']), **kw)


def make_loop(e, graph, mst, mou, max_it, thr, s0, impl, pieces, form, expect=None):
    lp = e.Loop(graph, mst, mou, DS, max_it, thr)
    assert lp.set_impl(impl) == impl
    lp.set_pieces(pieces)
    if impl == 2: assert lp.set_tile_form(1) == 1          # (small launches would otherwise take the wave pair, which has one gather form)
    assert lp.set_gather_form(form) == (form if expect is None else expect)
    lp.set_state0(s0)
    return lp


def run_forms(e, g, st, ou, max_it, thr, s0, impl, pieces):
    """{form: (k, state, output)} on one device graph; the program is built by the first form-2 loop."""
    graph = device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    res = {}
    for form in (1, 2):
        lp = make_loop(e, graph, mst, mou, max_it, thr, s0, impl, pieces, form)
        k = lp.run()
        res[form] = (k, lp.state(), lp.output())
        assert lp.run() == k and bits_equal(lp.state(), res[form][1])      # and again on the same handle
        lp.close()
    info = graph.gather_program_info()
    assert info['tiles'] == g['nodes'].shape[0] // 32 and info['bytes'] == 8 * info['tiles'] + 512 * info['batches']
    graph.close()
    return res


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same(res):
    (k1, s1, o1), (k2, s2, o2) = res[1], res[2]
    assert k1 == k2
    assert np.array_equal(s1, s2, equal_nan=True) and bits_equal(s1, s2), f'{int(np.sum(s1.view(np.uint32) != s2.view(np.uint32)))} of {s1.size} state values differ'
    assert bits_equal(o1, o2)


CASES = {}


def case(name):
    """Graph, nets, initial state and the C oracle's result of a named case: built once, shared by the modes, never modified."""
    if name not in CASES:
        rng = np.random.default_rng(sum(map(ord, name)))
        if name == 'hand': deg = hand_built_degrees()                                  # 512 nodes, 16 tiles
        elif name == 'random_partial': deg = rng.poisson(9.0, 1000)                    # 31 tiles + 8 rows that walk the CSR in the same launch
        elif name == 'two_tiles': deg = rng.poisson(4.0, 64)
        else: deg = np.minimum(300, (rng.pareto(1.2, 4096) * 3).astype(np.int64))     # 128 tiles, hubs of several batches
        g = graph_from_degrees(rng, deg)
        st, ou = nets(rng)
        s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
        CASES[name] = (g, st, ou, s0, corc.loop_node(g, st, ou, DS, 4, 0.0, s0))
    return CASES[name]


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('name', ['hand', 'random_partial', 'two_tiles', 'skewed'])
def test_gather_forms_are_bit_identical(name, impl, pieces):
    """Hand-built degrees (tests/test_gather_program.py: empty rows at every position, an empty group, an empty tile, a 200-entry hub, group
    totals 15 / 16 / 17 / 32, a group of a single row, balanced groups of exactly 16 and of 17 slots), a partial last tile, the smallest graph with a program, skewed degrees."""
    e = _engine()
    g, st, ou, s0, (kc, sc, oc) = case(name)
    res = run_forms(e, g, st, ou, 4, 0.0, s0, impl, pieces)
    assert_same(res)
    if impl == 1:
        assert res[2][0] == kc and np.array_equal(res[2][1], sc) and np.array_equal(res[2][2], oc)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_empty_row_beside_non_finite_rows_aggregates_to_zero(impl, pieces):
    """Rows 8 and 10 of a tile aggregate a NaN and a +inf state, row 9 between them is empty; one body, threshold 0.  The empty row's
    aggregate feeds layer 0 as an exact zero: its new state is finite and has form 1's bits (so have all the others, NaN included)."""
    e = _engine()
    rng = np.random.default_rng(7)
    deg = np.full(96, 3)
    deg[32 + 9] = 0
    g = graph_from_degrees(rng, deg)
    st, ou = nets(rng)
    s0 = (0.1 * rng.standard_normal((96, DS))).astype(np.float32)
    indptr, src = g['adjT'][0], g['adjT'][1]
    s0[src[indptr[32 + 8]]] = np.nan
    s0[src[indptr[32 + 10] + 1]] = np.inf
    res = run_forms(e, g, st, ou, 1, 0.0, s0, impl, pieces)
    assert_same(res)
    s2 = res[2][1]
    assert np.isnan(s2[32 + 8]).all() and not np.isfinite(s2[32 + 10]).any() and np.isfinite(s2[32 + 9]).all()
    if impl == 1:
        kc, sc, oc = corc.loop_node(g, st, ou, DS, 1, 0.0, s0)
        assert res[2][0] == kc and np.array_equal(s2, sc, equal_nan=True) and np.array_equal(res[2][2], oc, equal_nan=True)


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('world,layout', [(2, 'whole'), (3, 'whole'), (2, 'slice')])
def test_gather_forms_on_shards(world, layout, impl, pieces):
    """Loopback groups on 1,000 nodes: every rank but the first has row_begin != 0, and the last rank's range ends in a partial tile.  The sliced
    layout's owned rows take the given-aggregate loader, which has no gather: form 2 is not taken there and nothing changes."""
    import test_gpu_sharded as S
    e = _engine()
    n = 1000
    g, st, ou, s0, _ = case('random_partial')
    indptr, adj_src, adj_w, _, _ = S._csr_parts(g)
    res = {}
    for form in (1, 2):
        comms, graphs, loops, ranges = S._sharded_loops(e, g, st, ou, DS, 4, 0.0, s0, world, impl)
        for gr, lp in zip(graphs, loops):
            lp.set_pieces(pieces)
            if impl == 2: assert lp.set_tile_form(1) == 1
            if layout == 'slice':
                gr.set_full_adjacency(n, indptr, adj_src, adj_w)
                lp.set_slice_exchange(True)
            assert lp.set_gather_form(form) == (1 if layout == 'slice' else form)
        k = e.Loop.run_group(loops)
        res[form] = (k,) + S._collect(loops, ranges, None)
        for lp in loops: lp.close()
        for gr in graphs: gr.close()
        for c in comms: c.close()
    assert_same(res)
    if impl == 1 and layout == 'whole':
        kc, sc, oc = case('random_partial')[4]
        assert res[2][0] == kc and np.array_equal(res[2][1], sc) and np.array_equal(res[2][2], oc)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_derived_graph_shares_the_program(impl, pieces):
    """A graph made with derive() has the base graph's structure and its program (one copy); after update_labels rewrote its labels the
    Loop on it is form 1's bit for bit."""
    e = _engine()
    g, st, ou, s0, _ = case('random_partial')
    rng = np.random.default_rng(11)
    st1, ou1 = nets(rng, nl=NL + 2)
    base = device_graph(e, g)
    derived = base.derive(2)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    mst1, mou1 = e.Mlp(st1['weights'], st1['activations'], True), e.Mlp(ou1['weights'], ou1['activations'], True)
    assert base.gather_program_info()['tiles'] == 0
    res = {}
    for form in (1, 2):
        lp0 = make_loop(e, base, mst, mou, 3, 0.0, s0, impl, pieces, form)
        lp0.run()
        derived.update_labels(base, lp0, False, True)
        lp1 = make_loop(e, derived, mst1, mou1, 3, 0.0, s0, impl, pieces, form)
        k = lp1.run()
        res[form] = (k, lp1.state(), lp1.output())
        lp0.close(); lp1.close()
    info = base.gather_program_info()
    assert info['tiles'] == 31 and derived.gather_program_info() == info
    derived.close(); base.close()
    assert_same(res)
