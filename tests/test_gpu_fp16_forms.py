"""Piece format 2 (two fp16 pieces per fp32 operand, impl 2) at its edges in the fused forms that tests/test_fp16_edges.py does not reach:
k_fused_generic with hidden layers in its tile pairs (1,1), (2,2), (4,2), the wide-state form on 4, 5 and 7 waves with both tile loaders, the
seeded kernels of the label projection (full-tile, generic, wide) and the kernels for a last layer with its own activation.

The cases and what they expect are tests/fp16_form_cases.py; tests/test_fp16_form_cases_host.py shows on the CPU that their inputs decide
each verdict.  Every expectation is exact: identity-chain nets make a body's result the emulated cut applied once per layer, bit for bit; a
guard that must trip (one operand at exactly 4,094 = 65,504 / 2^4) returns the bits of the same form in format 3; the fp32 just below must
not trip.  Every loop first proves the form it runs in: kernel, waves per workgroup and the setters' answers."""
import numpy as np
import pytest

import fp16_form_cases as fc
from test_fp16_edges import UNDER, _device_graph, _mismatch, _same, cut

pytestmark = pytest.mark.gpu

IDS = [r['id'] for r in fc.FORMS]
WIDE = [r['id'] for r in fc.FORMS if r['kind'] == 'W']
SEEDED = [r['id'] for r in fc.FORMS if r['seeded']]


def _engine():
    from GNN import _engine
    return _engine


def corc_spmm(g, s0):
    from oracle import c_oracle as corc
    return corc.spmm(g['adjT'], s0)


def _open(case, pieces=2, proj=None, loader=None, graph=None):
    """A Loop of the case in the row's form (proj 'off': a seeded row's net as the unseeded kernel of the same shape runs it), proven."""
    e = _engine()
    row, st, ou = case['row'], case['st'], case['ou']
    proj = row['proj'] if proj is None else proj
    seeded, wide = proj != 'off', row['wide'] != 'off'
    graph = graph or _device_graph(e, case['g'])
    lp = e.Loop(graph, e.Mlp(st['weights'], st['activations'], False), e.Mlp(ou['weights'], ou['activations'], False), row['ds'], case['bodies'], 0.0)
    assert lp.set_persistent(False) is False            # (the persistent small-graph loop uses exact arithmetic)
    if seeded: assert lp.set_label_projection(proj) is (not wide)      # (a state wider than 64 is not covered by the projection alone)
    if wide: assert lp.set_wide_state(row['wide']) is True
    assert lp.set_impl(2) == 2 and lp.set_pieces(pieces) == pieces
    if seeded: assert lp.set_label_projection(proj) is True
    if row['kernel'] == 2: assert lp.set_tile_form(1) == 1
    if loader: assert lp.set_wide_loader(loader) is (loader == 'wide')
    assert lp.body_kernel() == row['kernel'] and lp.body_launch()[0] == row['waves'], (lp.body_kernel(), lp.body_launch())
    lp.set_state0(case['s0'])
    return graph, lp


def _run(case, pieces=2, proj=None, loader=None):
    graph, lp = _open(case, pieces, proj, loader)
    k = lp.run()
    res = (k, lp.state(), lp.output(), lp.range_info(), lp.gate_info())
    lp.close()
    graph.close()
    return res


def _check(case, proj=None, loaders=(None,)):
    """The case's verdict on the device: a trip is one repeat and format 3's bits of the same form; no trip is the emulated chain."""
    first = None
    for loader in loaders:
        r2 = _run(case, 2, proj, loader)
        first = first or r2
        assert _same(first, r2) and first[3] == r2[3], (case['row']['id'], loader)      # the two tile loaders: the same bits
        what = (case['row']['id'], loader, r2[3])
        if case['trip']:
            r3 = _run(case, 3, proj, loader)
            assert r3[3] == (False, 0), what                  # format 3 never trips
            assert r2[3] == (True, 1) and _same(r2, r3), what
        else:
            assert r2[0] == case['bodies'] and r2[3] == (False, 0), what
            if case['want'] is not None: assert np.array_equal(r2[1], case['want']), (what, _mismatch(case['x'], r2[1], case['want']))
    return r2


def _loaders(row, pos):
    """The wide-state form loads its full tiles with load_tile_wide and its partial last tile with load_tile_generic; an offender in a full
    tile is also run with load_tile_generic on every tile."""
    return (None, 'generic') if row['kind'] == 'W' and pos == 'full' else (None,)


# ---- 1. the chain, bit for bit -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ['own', 'agg'])
@pytest.mark.parametrize('name', IDS)
def test_chain_is_the_emulated_cut(name, route):
    """One body over the probe set (ties in both pieces, subnormal p1, +-0, up to the fp32 below 4,094), through the own state or the
    aggregated state: every state is cut applied once per layer to its input, bit for bit, and nothing trips.  A seeded form carries a node
    label and an aggregated arc label in fp32 through layer 0: those two columns are cut once fewer."""
    case = fc.chain_case(fc.BY_ID[name], route)
    assert case['trip'] is None and case['want'] is not None
    _check(case, loaders=_loaders(case['row'], 'full'))


# ---- 2. layer 0's guard, per column block --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('where', fc.WHERES)
@pytest.mark.parametrize('name', IDS)
def test_layer0_guard_boundary(name, where):
    """One offending operand in the whole graph, on a row in a full tile and on the last row of the partial tile: 4,094 trips, the fp32 below
    does not.  Aggregated blocks: a 'sum' hub over two sources of 2,047 (UNDER / 2) each.  A seeded form never cuts a label column: there a
    label at 4,094 must not trip either."""
    row = fc.BY_ID[name]
    for pos in fc.ROWS:
        for at_limit in (True, False):
            case = fc.layer0_case(row, where, pos, at_limit)
            assert (case['trip'] is not None) == (at_limit and not (row['seeded'] and where not in ('state', 'agg_state')))
            _check(case, loaders=_loaders(row, pos))


# ---- 3. the hidden layers' guard -------------------------------------------------------------------------------------------------------------------

def _hidden_params():
    return [pytest.param(r['id'], layer, unit, id=f'{r["id"]}-layer{layer}-unit{unit}') for r in fc.FORMS for layer, unit in fc.hidden_units(r)]


@pytest.mark.parametrize('name,layer,unit', _hidden_params())
def test_hidden_guard_boundary(name, layer, unit):
    """hidden_range: one unit's pre-activation is its bias, exactly 4,094 (trips) or the fp32 below (does not), in every 32-feature tile of
    every hidden layer - the padded second tile of a 48-wide layer and hidden layer 2 of the three-layer nets included."""
    row = fc.BY_ID[name]
    for at_limit in (True, False):
        _check(fc.hidden_case(row, layer, unit, at_limit))


# ---- 4. activations ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('act,v,trips', fc.ACTIVATIONS)
@pytest.mark.parametrize('name', fc.ACTIVATION_FORMS)
def test_activation_guard(name, act, v, trips):
    """test_fp16_edges.test_activation_guard on k_fused_generic (4,2) and on the wide-state form (5 waves): the guard reads the accumulator
    before the activation.  selu at 3,000 trips in both: they are instantiations of one kernel, whose hidden accumulators hold log2(e) v (the
    weights folded by gnn_fused_pack, the bias by fused_stage_vectors; hidden_range reads those accumulators in GNN_FUSED_DENSE_LAYERS), and
    log2(e) x 3,000 = 4,328.  selu at 2,600 (3,751) does not, and is compared with format 3 under the bound derived in
    test_fp16_edges.test_activation_guard for three layers - 2^-19 relative + 2^-26 absolute - which these three-layer nets take unchanged."""
    case = fc.activation_case(fc.BY_ID[name], act, v, trips)
    r2 = _check(case)
    if not trips and act == 'selu':
        r3 = _run(case, 3)
        err = np.abs(r2[1] - r3[1])
        print(f'{name}, selu at {v}: max |format 2 - format 3| {err.max():.3e}, max error / bound {np.max(err / (2.0 ** -19 * np.abs(r3[1]) + 2.0 ** -26)):.3f}')
        assert r3[3] == (False, 0) and np.all(err <= 2.0 ** -19 * np.abs(r3[1]) + 2.0 ** -26)


# ---- 5. what is different in the seeded forms ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('value', [5000.0, 1e5])
@pytest.mark.parametrize('name', SEEDED)
def test_seeded_label_behind_zero_weights_does_not_trip(name, value):
    """(a) A node label and the arc labels of one row far out of the fp16 range, every label row of W1 zero: the projection takes them in
    fp32, nothing cuts them - no repeat, and the bits of the run with those labels as generated.  The same narrow-label net unseeded cuts
    the label at layer 0: one repeat, format 3's bits."""
    row = fc.BY_ID[name]
    case = fc.zeroed_label_case(row, value, True)
    r = _check(case)
    plain = _run(fc.zeroed_label_case(row, None, True))
    assert r[0] == plain[0] and np.array_equal(r[1], plain[1])            # (net_output reads the node labels: its outputs differ)
    if row['nl'] == 1 and row['wide'] == 'off':
        off = fc.zeroed_label_case(row, value, False, arc=False)
        assert off['trip'] == 'b0.layer0'
        _check(off, proj='off')


@pytest.mark.parametrize('name', [n for n in SEEDED if fc.BY_ID[n]['hidden']])
def test_seeded_label_through_a_unit_weight(name):
    """(b) A node label through a weight of 1 into one hidden unit: the seed is the label itself.  4,094 trips (hidden_range reads the seeded
    accumulator); the fp32 below does not, and the column is what the layers behind layer 0 make of the uncut label.  Unseeded (narrow
    labels) layer 0 cuts the label first; the cut is idempotent, so behind a hidden layer both give the same bits - the two expectations
    differ only in the one-layer form (test_one_layer_seeded_net)."""
    row = fc.BY_ID[name]
    L = len(row['hidden']) + 1
    for pos in fc.ROWS:
        _check(fc.unit_weight_case(row, fc.LIMIT, True, 'b0.hidden1', pos))
        case = fc.unit_weight_case(row, UNDER, True, None, pos)
        r = _check(case)
        assert np.array_equal(r[1][:, fc.LABEL_UNIT], fc.behind_label_unit(case['g']['nodes'][:, 0], L))
        assert r[1][fc.ROWS[pos], fc.LABEL_UNIT] == (UNDER if L == 2 else UNDER / 2)
        if row['nl'] == 1:
            off = fc.unit_weight_case(row, UNDER, False, None, pos)
            assert np.array_equal(off['want'], case['want'])
            _check(off, proj='off')


def test_one_layer_seeded_net():
    """(c) One layer: the label term reaches the state uncut.  A term of 1e5 does not trip in one body - nothing is cut behind it - and the
    second body, which cuts that state, does: one repeat, format 3's bits.  In range, the seeded column is the label itself and the
    unseeded one its cut: the two expectations really differ."""
    row = fc.BY_ID['S-generic-40-one-layer-nl1']
    hub = fc.ROWS['partial']
    r = _check(fc.unit_weight_case(row, 1e5, True, None))
    assert r[1][hub, fc.LABEL_UNIT] == np.float32(1e5)
    _check(fc.unit_weight_case(row, 1e5, True, 'b1.layer0', bodies=2))
    seeded, off = fc.unit_weight_case(row, UNDER, True, None), fc.unit_weight_case(row, UNDER, False, None)
    assert np.sum(seeded['want'] != off['want']) > 100 and np.array_equal(off['want'][:, fc.LABEL_UNIT], cut(seeded['want'][:, fc.LABEL_UNIT]))
    _check(seeded)
    _check(off, proj='off')
    _check(fc.unit_weight_case(row, 1e5, False, 'b0.layer0'), proj='off')      # unseeded, layer 0 cuts the label: a repeat in the first body


# ---- 6. bookkeeping of the repeat ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', fc.BOOKKEEPING_FORMS)
def test_repeat_leaves_the_form_in_format_2(name):
    """A tripping run, then set_state0 with in-range values on the same handle: (True, 1), then (False, 1), and the second run is bit-equal
    to a fresh format-2 loop of the same form - the emulated cut, which format 3 does not return."""
    case, small = fc.bookkeeping_case(fc.BY_ID[name])
    graph, lp = _open(case)
    lp.run()
    assert lp.range_info() == (True, 1)
    lp.set_state0(small)
    k = lp.run()
    second = (k, lp.state(), lp.output())
    assert lp.range_info() == (False, 1) and lp.body_kernel() == case['row']['kernel'] and lp.body_launch()[0] == case['row']['waves']
    lp.close()
    graph.close()
    again = dict(case, s0=small, trip=None)
    again['want'] = fc.emulate(again)[0]
    fresh2, fresh3 = _check(again), _run(again, 3)
    assert _same(second, fresh2)
    assert not np.array_equal(second[1], fresh3[1])


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------------------------

def test_sharded_wide_state_repeats_when_only_the_last_rank_trips():
    """A loopback world of 2 in the wide-state form (state width 128, 4 waves): the one operand at the limit is a node label on the last
    rank, the repeat is decided from the exchanged range word - both ranks report it, and k, states and outputs are bit-equal to the same
    group in format 3."""
    from test_gpu_sharded import _collect, _sharded_loops
    e = _engine()
    case = fc.sharded_case()
    row = case['row']

    def group(pieces):
        comms, graphs, loops, ranges = _sharded_loops(e, case['g'], case['st'], case['ou'], row['ds'], 1, 0.0, case['s0'], 2, 2, strict=False)
        for lp in loops:
            lp.set_wide_state('always')                      # (the helper left the ranks on impl 0, where there is nothing to take)
            assert lp.set_impl(2) == 2 and lp.set_pieces(pieces) == pieces and lp.set_wide_state('always') is True
            assert lp.body_kernel() == 1 and lp.body_launch()[0] == row['waves']
        k = e.Loop.run_group(loops)
        state, out = _collect(loops, ranges, None)
        info = [lp.range_info() for lp in loops]
        for lp in loops: lp.close()
        for c in comms: c.close()
        return (k, state, out), info

    r2, info2 = group(2)
    r3, info3 = group(3)
    assert info2 == [(True, 1)] * 2 and info3 == [(False, 0)] * 2
    assert _same(r2, r3)


# ---- 8. stale rows behind a short shard ----------------------------------------------------------------------------------------------------------------

def test_sliced_exchange_does_not_trip_on_stale_rows_behind_a_short_shard():
    """Feature-sliced exchange on a loopback world of 2, 1,000 rows: the last rank owns 488, and the full-tile kernel's loader of a given
    aggregate copies all 32 rows of its last tile - 24 of them behind the shard's end, which the exchange never writes.  Layer 0 cuts them
    and the guard reads them like any operand, so they must be zeros, not what the allocation held before.  A first group on 1,024 rows
    (no short shard: every row of every exchange block is written) and states of 5,000, run and closed, leaves values of that size in blocks
    of exactly the sizes the second group asks for; the second group, in range, must not repeat, twice over with the same bits."""
    import test_gpu_sharded as S
    e = _engine()
    n, d = 1000, 64
    g, st, ou, s0 = S._case(8100, n, d, hidden=(128, 128))
    assert e.shard_range(n, 1, 2)[1] % 32 != 0 and float(np.max(np.abs(corc_spmm(g, s0)))) < 4094.0

    def group(g, state0, impl):
        n = g['nodes'].shape[0]
        indptr, adj_src, adj_w, _, _ = S._csr_parts(g)
        comms, graphs, loops, ranges = S._sharded_loops(e, g, st, ou, d, 2, 0.0, state0, 2, impl)
        for gr, lp in zip(graphs, loops):
            if impl == 2: assert lp.set_pieces(2) == 2 and lp.set_tile_form(1) == 1
            gr.set_full_adjacency(n, indptr, adj_src, adj_w)
            lp.set_slice_exchange(True)
            if impl == 2: assert lp.body_kernel() == 2
        k = e.Loop.run_group(loops)
        state, out = S._collect(loops, ranges, None)
        info = [(lp.range_info(), lp.gate_info()) for lp in loops]
        for lp in loops: lp.close()
        for gr in graphs: gr.close()
        for c in comms: c.close()
        return (k, state, out), info

    full = S._case(8101, 1024, d, hidden=(128, 128))[0]
    assert e.shard_range(1024, 0, 2)[1] == e.shard_range(1024, 1, 2)[1] == 512
    group(full, np.full((1024, d), 5000.0, np.float32), 1)
    first, info = group(g, s0, 2)
    assert info == [((False, 0), (False, 0))] * 2, info
    again, info = group(g, s0, 2)
    assert info == [((False, 0), (False, 0))] * 2 and _same(first, again)
