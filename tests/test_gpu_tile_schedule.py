"""gnn_loop_set_tile_schedule: the program kernel working through its tiles in ascending order (schedule 1) and in the balanced order
(schedule 2) computes every node with the same arithmetic - k, states and outputs identical bit for bit on impl 1 and on impl 2 with both
piece formats; on impl 1 both are the C oracle's.  State width 64 throughout.

The large cases have 2 W + 3 full tiles and a partial one, W = waves of a launch: the static rounds (slots w and w + W), one round of
tickets, and a balanced order that differs from the ascending one in nearly every slot (read back through the host builder)."""
import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from test_gpu_gather_program import (DS, MODES, NL, bits_equal, device_graph, graph_from_degrees, make_loop, nets)
from test_tile_schedule_host import tile_costs
from util import make_mlp

pytestmark = pytest.mark.gpu

W = 8 * 256           # waves of a launch on the MI355X's 256 CUs (on another device the cases stay valid comparisons)
N_LARGE = 32 * (2 * W + 3) + 5
HUB = 5000


def _engine():
    from GNN import _engine
    return _engine


def fast_graph(rng, deg):
    """graph_from_degrees without its per-row loops: row r takes the sources (5 r + 13 + 7919 j) mod n, j < deg[r] - distinct within a row
    because 7919 is prime and does not divide n - and every entry a distinct weight."""
    deg = np.asarray(deg, np.int64)
    n = deg.size
    assert n % 7919 and deg.max() < n
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    dst = np.repeat(np.arange(n), deg)
    j = np.arange(dst.size) - indptr[dst]
    src = (dst * 5 + 13 + j * 7919) % n
    src = src[np.lexsort((src, dst))]
    w = ((0.25 + rng.permutation(src.size) / (4.0 * max(1, src.size))) / np.repeat(deg, deg)).astype(np.float32)
    arcs = np.stack([src, dst, 2 * rng.random(src.size) - 1], 1).astype(np.float32)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    g = orc.make_graph_dict(arcs, (2 * rng.random((n, NL)) - 1).astype(np.float32), 'average')
    assert np.array_equal(g['adjT'][0], indptr) and np.array_equal(g['adjT'][1], src)
    g['adjT'] = (g['adjT'][0], g['adjT'][1], w)
    return g


CASES = {}
BODIES = {'n33': 3, 'n63': 3, 'n65': 3, 'n160': 3, 'no_arcs': 2, 'equal_rows': 2, 'tickets': 1, 'hub_last': 1, 'hub_first': 1}


def case(name):
    """Graph, nets, initial state and the C oracle's result of a named case: built once, shared by the modes, never modified."""
    if name not in CASES:
        rng = np.random.default_rng(sum(map(ord, name)))
        if name in ('tickets', 'hub_last', 'hub_first'):
            deg = rng.poisson(3.0, N_LARGE)
            if name == 'hub_last': deg[N_LARGE - 2] = HUB          # a row of the partial last tile: more than 255 batches
            if name == 'hub_first': deg[7] = HUB
            g = fast_graph(rng, deg)
        else:
            if name == 'no_arcs': deg = np.zeros(100, np.int64)
            elif name == 'equal_rows': deg = np.full(160, 4)
            else: deg = np.minimum(rng.poisson(6.0, int(name[1:])), int(name[1:]) - 1)
            g = graph_from_degrees(rng, deg)
        st, ou = nets(rng)
        s0 = (0.1 * rng.standard_normal((len(deg), DS))).astype(np.float32)
        CASES[name] = (g, st, ou, s0, corc.loop_node(g, st, ou, DS, BODIES[name], 0.0, s0))
    return CASES[name]


def loop_on(e, graph, mst, mou, max_it, s0, impl, pieces, schedule, expect=None):
    lp = make_loop(e, graph, mst, mou, max_it, 0.0, s0, impl, pieces, 2)
    assert lp.set_tile_schedule(schedule) == (schedule if expect is None else expect)
    return lp


def run_schedules(e, g, st, ou, max_it, s0, impl, pieces):
    """{schedule: (k, state, output)} on one device graph; the balanced order is built by the first loop that asks for it."""
    graph = device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    res = {}
    for schedule in (1, 2):
        lp = loop_on(e, graph, mst, mou, max_it, s0, impl, pieces, schedule)
        res[schedule] = (lp.run(), lp.state(), lp.output())
        lp.close()
    info, prog = graph.tile_schedule_info(), graph.gather_program_info()
    n = g['nodes'].shape[0]
    assert info['slots'] == (n + 31) // 32 and info['kind'] == 2 and info['body'] + info['tail'] == info['slots']
    assert info['tail'] == min(2 * W, info['slots'] // 2)
    assert prog['tiles'] == n // 32 and prog['bytes'] == 8 * prog['tiles'] + 512 * prog['batches']      # the program itself is as it was
    graph.close()
    return res


def assert_same(a, b):
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1], equal_nan=True) and bits_equal(a[1], b[1]), f'{int(np.sum(a[1].view(np.uint32) != b[1].view(np.uint32)))} of {a[1].size} state values differ'
    assert bits_equal(a[2], b[2])


def check(res, impl, oracle):
    assert_same(res[1], res[2])
    if impl == 1:
        kc, sc, oc = oracle
        for r in (res[1], res[2]):
            assert r[0] == kc and np.array_equal(r[1], sc) and np.array_equal(r[2], oc)


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('name', ['n33', 'n63', 'n65', 'n160', 'no_arcs', 'equal_rows'])
def test_small_and_light_graphs(name, impl, pieces):
    """2 to 5 tiles, all in the first static round: a partial tile of 1, 31 and 1 rows, five full tiles, no arc at all, all rows equal."""
    g, st, ou, s0, oracle = case(name)
    check(run_schedules(_engine(), g, st, ou, BODIES[name], s0, impl, pieces), impl, oracle)


def balanced_order(e, g):
    cost = tile_costs(g['adjT'][0])
    return cost, e.tile_schedule(cost, W, 1)


@pytest.mark.parametrize('name', ['tickets', 'hub_last', 'hub_first'])
def test_large_orders_really_differ(name):
    """What the large comparisons exercise, read back through the host builder from the graph's own costs: a heaviest tile opens the launch,
    one of the lightest tiles sits behind the last ticket round, and nearly every slot holds another tile than under the ascending order."""
    e = _engine()
    g = case(name)[0]
    cost, order = balanced_order(e, g)
    slots = cost.size
    assert slots == 2 * W + 4 and (N_LARGE % 32) == 5
    assert cost[order[0]] == cost.max() and cost[order[-1]] == cost.min()
    body = order[:slots - slots // 2]
    assert cost[order[2 * W:]].max() <= cost[body].min()               # the ticket round: tail tiles, none heavier than any body tile
    assert cost[2 * W:slots - 1].max() > cost[body].min()              # ... which the tiles with the highest ids are not
    assert np.count_nonzero(order != np.arange(slots)) > slots * 9 // 10
    if name == 'hub_last': assert order[0] == slots - 1 and cost[slots - 1] >= HUB       # the partial tile is slot 0
    if name == 'hub_first': assert order[0] == 0
    if name != 'tickets':
        hdr, _ = e.gather_program(g['adjT'][0][:32 * (slots - 1) + 1], g['adjT'][1], g['adjT'][2])
        if name == 'hub_first': assert hdr[0, 1] > 255                 # batches of the hub's tile do not fit a byte


@pytest.mark.parametrize('impl,pieces', MODES)
@pytest.mark.parametrize('name', ['tickets', 'hub_last', 'hub_first'])
def test_ticket_rounds_and_hubs(name, impl, pieces):
    """2 W + 3 full tiles and a partial one at mean degree 3; a hub row of 5,000 arcs in the partial last tile (slot 0 of the balanced
    order) and in tile 0.  One body."""
    g, st, ou, s0, oracle = case(name)
    check(run_schedules(_engine(), g, st, ou, 1, s0, impl, pieces), impl, oracle)


GENERIC = {}


def generic_case(ds):
    """The 'tickets' graph under a net_state of state width ds with one 32-wide hidden layer, and the C oracle's result after one body:
    built once per width, shared by the modes, never modified."""
    if ds not in GENERIC:
        g = case('tickets')[0]
        rng = np.random.default_rng(9000 + ds)
        st = make_mlp(rng, 1 + 2 * (ds + NL), [32, ds], 'selu', gain=0.6, bn_random=True)
        ou = make_mlp(rng, ds + NL, [2], 'softmax', bn_random=True)
        s0 = (0.1 * rng.standard_normal((N_LARGE, ds))).astype(np.float32)
        GENERIC[ds] = (g, st, ou, s0, corc.loop_node(g, st, ou, ds, 1, 0.0, s0))
    return GENERIC[ds]


@pytest.mark.parametrize('impl', [1, 2])
@pytest.mark.parametrize('ds', [32, 48])
def test_ticket_round_of_the_generic_kernel(ds, impl):
    """k_fused_generic (state widths 32: one feature tile, and 48: two) on the 2 W + 3 full tiles and a partial one of 'tickets': the two
    static rounds and one round of tickets drawn through the functions it shares with k_fused_full.  One body against the C oracle: impl 1
    bit for bit, impl 2 the same k and a state within 2e-6 relative."""
    e = _engine()
    g, st, ou, s0, (kc, sc, oc) = generic_case(ds)
    assert 2 * W * 32 < g['nodes'].shape[0] == N_LARGE
    graph = device_graph(e, g)
    lp = e.Loop(graph, e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True), ds, 1, 0.0)
    assert lp.set_impl(impl) == impl and lp.body_kernel() == 1
    lp.set_state0(s0)
    k, s, o = lp.run(), lp.state(), lp.output()
    lp.close(); graph.close()
    if impl == 1: assert k == kc and np.array_equal(s, sc) and np.array_equal(o, oc)
    else:
        err = float(np.max(np.abs(s - sc)))
        assert k == kc and err < 2e-6 * max(1.0, float(np.max(np.abs(sc)))), f'max |state - oracle| {err}, NaNs {int(np.isnan(s).sum())}'


@pytest.mark.parametrize('impl,pieces', MODES)
def test_switching_on_one_handle(impl, pieces):
    """One loop handle 2 -> 1 -> 2 between runs."""
    e = _engine()
    g, st, ou, s0, oracle = case('tickets')
    graph = device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    lp = loop_on(e, graph, mst, mou, 1, s0, impl, pieces, 2)
    runs = []
    for schedule in (2, 1, 2):
        assert lp.set_tile_schedule(schedule) == schedule
        runs.append((lp.run(), lp.state(), lp.output()))
    lp.close(); graph.close()
    assert_same(runs[0], runs[1])
    assert_same(runs[0], runs[2])
    if impl == 1: assert runs[0][0] == oracle[0] and np.array_equal(runs[0][1], oracle[1]) and np.array_equal(runs[0][2], oracle[2])


def test_derived_graph_shares_the_schedule():
    e = _engine()
    g, st, ou, s0, _ = case('n160')
    base = device_graph(e, g)
    derived = base.derive(2)
    assert base.tile_schedule_info() == dict(slots=0, kind=0, body=0, tail=0, build_ms=0.0)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    lp = loop_on(e, base, mst, mou, 1, s0, 1, 2, 1)
    assert base.tile_schedule_info()['kind'] == 1 and derived.tile_schedule_info() == base.tile_schedule_info()
    assert lp.set_tile_schedule(2) == 2
    info = base.tile_schedule_info()
    assert info['kind'] == 2 and info['slots'] == 5 and info['tail'] == 2 and info['body'] == 3
    assert derived.tile_schedule_info() == info
    lp.close(); derived.close(); base.close()


@pytest.mark.parametrize('impl,pieces', MODES)
def test_not_applicable_without_a_program(impl, pieces):
    """Gather form 1 reads no program: the setter answers 0 and the results are the program kernel's."""
    e = _engine()
    g, st, ou, s0, oracle = case('n160')
    graph = device_graph(e, g)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    lp = make_loop(e, graph, mst, mou, 3, 0.0, s0, impl, pieces, 1)
    before = (lp.run(), lp.state(), lp.output())
    assert lp.set_tile_schedule(2) == 0
    after = (lp.run(), lp.state(), lp.output())
    lp.close()
    lp = loop_on(e, graph, mst, mou, 3, s0, impl, pieces, 2)
    prog = (lp.run(), lp.state(), lp.output())
    lp.close(); graph.close()
    assert_same(before, after)
    assert_same(before, prog)
    if impl == 1: assert before[0] == oracle[0] and np.array_equal(before[1], oracle[1]) and np.array_equal(before[2], oracle[2])
