"""The gather program's two entry formats on the device (gnn_graph_set_program_entries): a graph whose rows have uniform weights holds
4-byte entries and one weight per row, any other 8-byte entries; the CSR walk (gather form 1) and the program in either format evaluate
every row's fmaf chain in the same order - k, states and outputs identical bit for bit - and the exact path is the C oracle's.
State width 64, one wave per tile, graphs of 64 to 1,000 nodes with 'average'-style weights (1 / in-degree)."""
import numpy as np
import pytest

from oracle import c_oracle as corc
import test_gpu_gather_program as G
from test_gather_program import hand_built_degrees

pytestmark = pytest.mark.gpu

DS = G.DS
MODES = G.MODES                            # (impl, piece format): (1, 2), (2, 2), (2, 3)


def _engine():
    from GNN import _engine
    return _engine


def uniform_graph(rng, deg):
    """G.graph_from_degrees with every row's weights 1 / degree: the rows are uniform, the program compactable."""
    g = G.graph_from_degrees(rng, deg)
    d = np.asarray(deg, np.int64)
    g['adjT'] = (g['adjT'][0], g['adjT'][1], (1.0 / np.repeat(d, d)).astype(np.float32))
    return g


CASES = {}


def case(name):
    """Graph, nets, initial state, bodies and the C oracle's result of a named case: built once, shared by the modes, never modified."""
    if name not in CASES:
        rng = np.random.default_rng(sum(map(ord, name)) + 1)
        bodies = 4
        if name == 'hand': deg = hand_built_degrees()                    # 512 nodes: empty rows, an empty group and tile, a 200-entry hub, batch edges
        elif name == 'two_tiles': deg = rng.poisson(4.0, 64)             # the first tile's weights in front of the spread, the second's a tile ahead
        elif name == 'partial': deg = rng.poisson(9.0, 1000)             # 31 tiles and a partial last tile with a program of its own
        else:                                                            # 'non_finite': an empty row between a NaN and a +inf neighbour row
            deg = np.full(96, 3)
            deg[32 + 9] = 0
            bodies = 1
        g = uniform_graph(rng, deg)
        st, ou = G.nets(rng)
        s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
        if name == 'non_finite':
            indptr, src = g['adjT'][0], g['adjT'][1]
            s0[src[indptr[32 + 8]]] = np.nan
            s0[src[indptr[32 + 10] + 1]] = np.inf
        CASES[name] = (g, st, ou, s0, bodies, corc.loop_node(g, st, ou, DS, bodies, 0.0, s0))
    return CASES[name]


def run_once(lp):
    k = lp.run()
    return k, lp.state(), lp.output()


def assert_bits(a, b, what):
    assert a[0] == b[0], what
    assert G.bits_equal(a[1], b[1]), f'{what}: {int(np.sum(a[1].view(np.uint32) != b[1].view(np.uint32)))} of {a[1].size} state values differ'
    assert G.bits_equal(a[2], b[2]), what


def program_bytes(info, entries):
    slots = info['tiles'] + (1 if info['partial'] else 0)
    return 8 * info['tiles'] + (256 * info['batches'] + 128 * slots if entries == 4 else 512 * info['batches'])


def run_formats(e, g, st, ou, bodies, s0, impl, pieces, available=4):
    """{'csr', 4, 8: (k, state, output)} on one device graph: form 1, then form 2 with 4-byte entries asked for (`available`: what the graph
    then holds) and with 8 forced - the second on the SAME loop handle, whose next run must take the new format and repeat its bits."""
    n = g['nodes'].shape[0]
    graph = G.device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    res = {}
    lp = G.make_loop(e, graph, mst, mou, bodies, 0.0, s0, impl, pieces, 1)
    res['csr'] = run_once(lp)
    lp.close()
    assert graph.set_program_entries(4) == available and graph.gather_program_format() == available
    lp = G.make_loop(e, graph, mst, mou, bodies, 0.0, s0, impl, pieces, 2)
    res[4] = run_once(lp)
    info = dict(graph.gather_program_info(), partial=n % 32 != 0)
    assert info['tiles'] == n // 32 and info['bytes'] == program_bytes(info, available)
    assert graph.set_program_entries(8) == 8 and graph.gather_program_format() == 8
    res[8] = run_once(lp)                                       # the handle's next run: the rebuilt program in the other format
    info8 = dict(graph.gather_program_info(), partial=info['partial'])
    assert (info8['tiles'], info8['batches']) == (info['tiles'], info['batches']) and info8['bytes'] == program_bytes(info8, 8)
    assert graph.set_program_entries(0) == available            # the library's choice again
    assert_bits(run_once(lp), res[4], 'after switching back')
    lp.close(); graph.close()
    return res


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('name', ['hand', 'two_tiles', 'partial', 'non_finite'])
def test_entry_formats_are_bit_identical(name, impl, pieces):
    e = _engine()
    g, st, ou, s0, bodies, (kc, sc, oc) = case(name)
    res = run_formats(e, g, st, ou, bodies, s0, impl, pieces)
    assert_bits(res['csr'], res[4], 'form 1 against 4-byte entries')
    assert_bits(res['csr'], res[8], 'form 1 against 8-byte entries')
    if name == 'non_finite':
        s = res[4][1]
        assert np.isnan(s[32 + 8]).all() and not np.isfinite(s[32 + 10]).any() and np.isfinite(s[32 + 9]).all()
    if impl == 1:
        assert res[4][0] == kc and np.array_equal(res[4][1], sc, equal_nan=True) and np.array_equal(res[4][2], oc, equal_nan=True)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_one_non_uniform_row_keeps_eight_byte_entries(impl, pieces):
    """One entry of one row a single ulp off its row's weight: the graph holds 8-byte entries whatever is asked for, and form 2 keeps form 1's bits."""
    e = _engine()
    g, st, ou, s0, bodies, _ = case('partial')
    indptr, src, w = g['adjT']
    row = int(np.flatnonzero(np.diff(indptr) >= 2)[7])
    w2 = w.copy()
    w2[indptr[row] + 1] = np.nextafter(w2[indptr[row] + 1], np.float32(0.0))
    g2 = dict(g, adjT=(indptr, src, w2))
    res = run_formats(e, g2, st, ou, bodies, s0, impl, pieces, available=8)
    assert_bits(res['csr'], res[4], 'form 1 against the program of a non-uniform graph')
    assert_bits(res['csr'], res[8], 'form 1 against 8-byte entries')
    if impl == 1:
        kc, sc, oc = corc.loop_node(g2, st, ou, DS, bodies, 0.0, s0)
        assert res[4][0] == kc and np.array_equal(res[4][1], sc) and np.array_equal(res[4][2], oc)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_entry_formats_on_two_ranks(impl, pieces):
    """A two-rank loopback group on 1,000 nodes: rank 1 has row_begin != 0 and ends in a partial tile; every rank's graph holds the compact format."""
    import test_gpu_sharded as S
    e = _engine()
    g, st, ou, s0, bodies, (kc, sc, oc) = case('partial')
    res = {}
    for key, form, entries in (('csr', 1, 0), (4, 2, 0), (8, 2, 8)):
        comms, graphs, loops, ranges = S._sharded_loops(e, g, st, ou, DS, bodies, 0.0, s0, 2, impl)
        for gr, lp in zip(graphs, loops):
            lp.set_pieces(pieces)
            if impl == 2: assert lp.set_tile_form(1) == 1
            if entries: assert gr.set_program_entries(entries) == entries
            assert lp.set_gather_form(form) == form
            if form == 2: assert gr.gather_program_format() == (entries or 4)
        k = e.Loop.run_group(loops)
        res[key] = (k,) + S._collect(loops, ranges, None)
        for lp in loops: lp.close()
        for gr in graphs: gr.close()
        for c in comms: c.close()
    assert_bits(res['csr'], res[4], 'form 1 against 4-byte entries')
    assert_bits(res['csr'], res[8], 'form 1 against 8-byte entries')
    if impl == 1:
        assert res[4][0] == kc and np.array_equal(res[4][1], sc) and np.array_equal(res[4][2], oc)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_derived_graph_shares_the_compact_program(impl, pieces):
    """A graph made with derive() shares the base graph's program in the format the base holds; after update_labels rewrote its labels the
    Loop on it is form 1's bit for bit."""
    e = _engine()
    g, st, ou, s0, bodies, _ = case('partial')
    rng = np.random.default_rng(11)
    st1, ou1 = G.nets(rng, nl=G.NL + 2)
    base = G.device_graph(e, g)
    derived = base.derive(2)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    mst1, mou1 = e.Mlp(st1['weights'], st1['activations'], True), e.Mlp(ou1['weights'], ou1['activations'], True)
    res = {}
    for form in (1, 2):
        lp0 = G.make_loop(e, base, mst, mou, 3, 0.0, s0, impl, pieces, form)
        lp0.run()
        derived.update_labels(base, lp0, False, True)
        lp1 = G.make_loop(e, derived, mst1, mou1, 3, 0.0, s0, impl, pieces, form)
        res[form] = run_once(lp1)
        lp0.close(); lp1.close()
    info = base.gather_program_info()
    assert info['tiles'] == 31 and derived.gather_program_info() == info
    assert base.gather_program_format() == 4 and derived.gather_program_format() == 4
    derived.close(); base.close()
    assert_bits(res[1], res[2], 'derived graph, form 1 against the compact program')
