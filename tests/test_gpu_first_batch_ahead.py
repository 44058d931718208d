"""The program kernel of the full-tile form (gather form 2) at its seams: the partial last tile, which it now gathers from a program of its
own, and a tile's first batch, which it requests during the tile before.  Exact comparisons only: on impl 1 and on impl 2 with both piece
formats, form 2 equals form 1 bit for bit in k, state and output, and on impl 1 both equal the C oracle.  State width 64 throughout.

A wave's first two tiles are fixed by the launch (tiles w and w + W, W = waves of the launch); only its third and later ones are drawn from
a counter.  The batch-count sequences are therefore laid into the first two rounds of a launch of 2 W + 1 tiles, and the launches of the
tile-assignment cases are prefixes of that graph: its arcs all start in the first tile and the run is one body long, so that one oracle
result serves every prefix."""
import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from test_gpu_gather_program import (DS, MODES, NL, assert_same, bits_equal, device_graph, graph_from_degrees, make_loop, nets)

pytestmark = pytest.mark.gpu


def _engine():
    from GNN import _engine
    return _engine


def waves_of_a_launch():
    """One workgroup of 8 waves on each of the MI355X's 256 CUs.  (On a device with another CU count the cases below stay valid comparisons;
    they just no longer sit on the boundaries between the rounds.)"""
    return 8 * 256


def run_forms(e, g, st, ou, max_it, s0, impl, pieces, derive=False):
    """{form: (k, state, output)}; the program's size as the graph reports it, and as a graph derived from it does."""
    n = g['nodes'].shape[0]
    graph = device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    res = {}
    for form in (1, 2):
        lp = make_loop(e, graph, mst, mou, max_it, 0.0, s0, impl, pieces, form, expect=None if n >= 32 else 1)
        res[form] = (lp.run(), lp.state(), lp.output())
        lp.close()
    info = graph.gather_program_info()
    assert info['tiles'] == n // 32 and info['bytes'] == 8 * info['tiles'] + 512 * info['batches']
    if n >= 32: assert info['batches'] >= info['tiles'] + (1 if n % 32 else 0)      # the partial tile's batches are counted
    if derive:
        d = graph.derive(2)
        assert d.gather_program_info() == info
        d.close()
    graph.close()
    return res


def check(res, impl, oracle, n=None):
    assert_same(res)
    if impl == 1:
        kc, sc, oc = oracle
        assert res[2][0] == kc and np.array_equal(res[2][1], sc[:n], equal_nan=True) and np.array_equal(res[2][2], oc[:n], equal_nan=True)


# ---- the partial last tile through the program -----------------------------------------------------------------------------------------
PARTIAL = {}


def partial_case(name):
    if name not in PARTIAL:
        rng = np.random.default_rng(sum(map(ord, name)))
        if name == 'hub': deg = rng.poisson(5.0, 32 * 3 + 5); deg[-1] = 70         # the last valid row: more than 64 arcs (several batches)
        elif name == 'no_arcs': deg = rng.poisson(5.0, 70); deg[64:] = 0           # a partial tile of empty rows only
        else: deg = rng.poisson(6.0, int(name[1:]))                                # n33, n63, n65, n1000: 1, 31, 1 and 8 valid rows
        deg = np.minimum(deg, len(deg) - 1)
        if name == 'hub': assert deg[-1] > 64
        g = graph_from_degrees(rng, deg)
        st, ou = nets(rng)
        s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
        PARTIAL[name] = (g, st, ou, s0, corc.loop_node(g, st, ou, DS, 4, 0.0, s0))
    return PARTIAL[name]


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('name', ['n33', 'n63', 'n65', 'n1000', 'hub', 'no_arcs'])
def test_partial_last_tile_through_the_program(name, impl, pieces):
    g, st, ou, s0, oracle = partial_case(name)
    check(run_forms(_engine(), g, st, ou, 4, s0, impl, pieces, derive=True), impl, oracle)


# ---- batch counts around the tile boundary, tile assignment ------------------------------------------------------------------------------
# degrees of a 32-row tile with the given number of batches (four lane groups of 8 rows: 16 slots each per batch; an empty row takes one slot)
TILE = {0: np.zeros(32, np.int64), 1: np.full(32, 2), 2: np.full(32, 4), 7: np.full(32, 14)}
ROUND1 = [1, 7, 1, 2, 2]        # batches of tile t < W by t % 5, and of the tile the same wave takes next (t + W): 1 -> 7, 7 -> 1, 1 -> 1,
ROUND2 = [7, 1, 1, 0, 2]        # full -> all-empty (which also sits between two full tiles of its round), 2 -> 2
ROUNDS = {}


def rounds_case():
    """2 W + 1 tiles, the very last a one-batch tile; every arc starts in tile 0."""
    if not ROUNDS:
        W = waves_of_a_launch()
        rng = np.random.default_rng(2025)
        kinds = [ROUND1[t % 5] for t in range(W)] + [ROUND2[t % 5] for t in range(W)] + [1]
        deg = np.concatenate([TILE[k] for k in kinds])
        n = deg.size
        indptr = np.zeros(n + 1, np.int64)
        np.cumsum(deg, out=indptr[1:])
        dst = np.repeat(np.arange(n), deg)
        j = np.arange(dst.size) - indptr[dst]
        src = (dst * 5 + j * 2 + (dst >> 5)) % 32                                      # distinct within a row (at most 14 entries, step 2 ... of 32)
        order = np.lexsort((src, dst))
        src = src[order]
        assert all(np.unique(src[indptr[r]:indptr[r + 1]]).size == deg[r] for r in (0, 33, 64, n - 1))
        w = (0.25 + rng.permutation(src.size) / (4.0 * src.size)) / np.repeat(deg, deg)
        nodes = (2 * rng.random((n, NL)) - 1).astype(np.float32)
        lab = (2 * rng.random(src.size) - 1).astype(np.float32)                       # arc labels, in the order of (dst, src)
        st, ou = nets(rng)
        s0 = (0.1 * rng.standard_normal((n, DS))).astype(np.float32)
        ROUNDS.update(W=W, kinds=kinds, lab=lab, src=src, dst=dst, w=w.astype(np.float32), nodes=nodes, st=st, ou=ou, s0=s0, indptr=indptr)
        ROUNDS['oracle'] = corc.loop_node(prefix_graph(2 * W + 1), st, ou, DS, 1, 0.0, s0)
    return ROUNDS


def prefix_graph(tiles):
    """The first `tiles` tiles of the rounds graph as an oracle graph dict."""
    c = ROUNDS
    n, ne = 32 * tiles, int(c['indptr'][32 * tiles])
    arcs = np.stack([c['src'][:ne], c['dst'][:ne], c['lab'][:ne]], 1).astype(np.float32)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    g = orc.make_graph_dict(arcs, c['nodes'][:n], 'average')
    assert np.array_equal(g['adjT'][0], c['indptr'][:n + 1]) and np.array_equal(g['adjT'][1], c['src'][:ne])
    g['adjT'] = (g['adjT'][0], g['adjT'][1], c['w'][:ne])
    return g


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('tiles', ['1', '100', 'W', 'W+1', '2W', '2W+1'])
def test_tile_assignment_and_batch_counts(tiles, impl, pieces):
    """One tile; fewer tiles than waves; exactly W (no wave has a second tile); W + 1 (one wave does); 2 W (the static rounds, no ticket);
    2 W + 1 (one ticket is served, every other wave's draw and its look-ahead end past the last tile).  In the launches of more than W tiles
    the waves cross the tile boundaries 1 -> 7, 7 -> 1, 1 -> 1, 2 -> all-empty and 2 -> 2 batches; the very last tile has one batch."""
    e = _engine()
    c = rounds_case()
    W = c['W']
    t = {'1': 1, '100': 100, 'W': W, 'W+1': W + 1, '2W': 2 * W, '2W+1': 2 * W + 1}[tiles]
    g = prefix_graph(t)
    hdr, _ = e.gather_program(g['adjT'][0], g['adjT'][1], g['adjT'][2])
    assert hdr[:, 1].tolist() == [max(1, k) for k in c['kinds'][:t]]                      # the batch counts the case is about
    check(run_forms(e, g, c['st'], c['ou'], 1, c['s0'][:32 * t], impl, pieces), impl, c['oracle'], 32 * t)


@pytest.mark.parametrize('impl,pieces', MODES)
def test_last_tile_of_one_batch_and_an_empty_tile_between_full_ones(impl, pieces):
    """Few tiles, one per wave: 2, all-empty, 7, 1 batches and a partial tile; four bodies."""
    rng = np.random.default_rng(77)
    deg = np.concatenate([TILE[2], TILE[0], TILE[7], TILE[1], np.full(5, 3)])
    g = graph_from_degrees(rng, deg)
    st, ou = nets(rng)
    s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
    check(run_forms(_engine(), g, st, ou, 4, s0, impl, pieces), impl, corc.loop_node(g, st, ou, DS, 4, 0.0, s0))


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('world', [2, 3])
def test_ranges_of_a_loopback_group(world, impl, pieces):
    """1,000 nodes over 2 and 3 ranks: row_begin != 0 on every rank but the first; a rank's graph holds its own rows only, so its range ends
    in the partial tile of that graph's program (the last rank's always does: 1,000 rows are no whole number of tiles per rank)."""
    import test_gpu_sharded as S
    e = _engine()
    g, st, ou, s0, oracle = partial_case('n1000')
    res = {}
    for form in (1, 2):
        comms, graphs, loops, ranges = S._sharded_loops(e, g, st, ou, DS, 4, 0.0, s0, world, impl)
        for lp in loops:
            lp.set_pieces(pieces)
            if impl == 2: assert lp.set_tile_form(1) == 1
            assert lp.set_gather_form(form) == form
        k = e.Loop.run_group(loops)
        res[form] = (k,) + S._collect(loops, ranges, None)
        if form == 2:
            for gr, (rb, nr) in zip(graphs, ranges):
                info = gr.gather_program_info()
                assert info['tiles'] == nr // 32 and info['bytes'] == 8 * info['tiles'] + 512 * info['batches']
        for lp in loops: lp.close()
        for gr in graphs: gr.close()
        for cm in comms: cm.close()
    check(res, impl, oracle)


# ---- stale rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impl,pieces', MODES)
def test_nan_row_as_first_entry_of_a_first_batch(impl, pieces):
    """Three bodies.  The source of the first entry of tile 2's batch 0 (lane group 0, slot 0: the first arc of the tile's first row) is a
    NaN row from the start, and the NaN spreads with every body: a batch taken from the wrong body's table, or too early, has other bits."""
    rng = np.random.default_rng(5)
    deg = np.maximum(1, rng.poisson(5.0, 32 * 5 + 7))
    g = graph_from_degrees(rng, deg)
    st, ou = nets(rng)
    s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
    indptr, src = g['adjT'][0], g['adjT'][1]
    s0[src[indptr[64]]] = np.nan
    res = run_forms(_engine(), g, st, ou, 3, s0, impl, pieces)
    nan_rows = np.isnan(res[2][1]).any(1)
    assert nan_rows[64] and 1 < nan_rows.sum() < len(deg)
    assert res[1][0] == res[2][0] and bits_equal(res[1][1], res[2][1]) and bits_equal(res[1][2], res[2][2])
    if impl == 1:
        kc, sc, oc = corc.loop_node(g, st, ou, DS, 3, 0.0, s0)
        assert res[2][0] == kc and np.array_equal(res[2][1], sc, equal_nan=True) and np.array_equal(res[2][2], oc, equal_nan=True)
