"""The wide-state form (gnn_loop_set_wide_state) on the GPU: k_fused_generic on workgroups of 4 to 7 waves with the wide-row tile loader,
for state widths 76 .. 128 (tests/wide_state_cases.py).

Bounds, none of them measured on the code under test:
  impl 1   bit-identical to the C oracle (k, state, output): the loader evaluates the oracle's fmaf chain per element;
  impl 2   the oracle's k, states and outputs within 2e-6 max(1, max |state|) of the C oracle - the bound test_gpu_parity holds the split path
           to - and 1e-5 of the float64 oracle (the default path's contract);
  no repeat: gate_info()[0] == 0 and range_info()[0] == 0 - the result is the form's, not a per-op repeat's (every gate of the
           threshold-0 runs sees a robust mover: wide_state_cases.check_case)."""
import numpy as np
import pytest

import wide_state_cases as wc

pytestmark = pytest.mark.gpu

ALL = range(len(wc.CASES))


def _engine():
    from GNN import _engine
    return _engine


def _device_graph(g):
    e = _engine()
    mask = np.logical_and(g['set_mask'], g['output_mask'])
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    return e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'], mask)


def _loop(i, max_it, thr):
    e = _engine()
    g, st, ou, s0 = wc.case(i)
    loop = e.Loop(_device_graph(g), e.Mlp(st['weights'], st['activations'], st['batch_normalization']),
                  e.Mlp(ou['weights'], ou['activations'], ou['batch_normalization']), wc.CASES[i]['d'], max_it, thr)
    loop.set_state0(s0)
    return loop


def _wide(i, max_it, thr, impl):
    """A loop of case i in the wide-state form (case 5: together with the label projection, impl 2 only)."""
    loop = _loop(i, max_it, thr)
    if wc.CASES[i].get('seeded'): assert loop.set_label_projection('auto') is False      # not covered by the projection alone
    assert loop.set_wide_state('always') is True
    assert loop.set_impl(impl) == impl and loop.body_kernel() == 1 and loop.body_launch()[0] == wc.CASES[i]['waves']
    return loop


def _close(s, o, sc, oc, s64, o64, what=''):
    tol = 2e-6 * max(1.0, float(np.max(np.abs(sc))))
    e64, ec = float(np.max(np.abs(s - s64))), float(np.max(np.abs(s - sc)))
    eo64, eoc = float(np.max(np.abs(o - o64))), float(np.max(np.abs(o - oc)))
    print(f'{what}: |state - f64| {e64:.2e}, |state - C oracle| {ec:.2e} (bound {tol:.2e}), |out - f64| {eo64:.2e}, |out - C oracle| {eoc:.2e}')
    assert e64 <= 1e-5 and ec <= tol and eo64 <= 1e-5 and eoc <= tol, (what, e64, ec, tol, eo64, eoc)


# ---- 1. default refusal and acceptance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', ALL)
def test_off_by_default_and_taken_when_asked(i):
    e = _engine()
    c = wc.CASES[i]
    dims, acts, d, nl, al, n = wc.net_description(i)
    loop = _loop(i, c['max_it'], 0.0)
    assert loop.set_impl(1) != 1 and loop.set_impl(2) != 2 and loop.body_kernel() == 0 and loop.body_launch() == (0, 0)
    if c.get('seeded'):
        assert loop.set_label_projection('auto') is False and loop.set_impl(2) != 2         # the projection alone: still no tile of eight waves
        assert loop.set_wide_state('always') is True
        assert loop.set_impl(1) != 1                                                         # the projection is a form of impl 2
        assert loop.set_impl(2) == 2
        form = e.wide_state_form(dims, acts, d, nl, al, n, 'always', 'auto')
        assert form['seeded'] and loop.set_label_projection('auto') is True
    else:
        assert loop.set_wide_state('always') is True
        assert loop.set_impl(1) == 1
        form = e.wide_state_form(dims, acts, d, nl, al, n, 'always')
    assert loop.body_kernel() == 1 == form['kernel']
    waves, grid = loop.body_launch()
    assert waves == form['waves'] == c['waves'] and grid == (n + 31) // 32
    assert (waves == 4) == (d == 128) and (i not in (2, 4) or waves > 4)
    assert loop.set_wide_state('off') is False and loop.set_impl(1) != 1 and loop.body_kernel() == 0


# ---- 2. impl 1 bit for bit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', wc.UNSEEDED)
def test_impl_one_is_the_c_oracle_bit_for_bit(i):
    c = wc.CASES[i]
    for max_it, thr in ((c['max_it'], 0.0),) + (((30, 0.01),) if c['k'] is not None else ()):
        (kc, sc, oc), _ = wc.oracles(i, max_it, thr)
        loop = _wide(i, max_it, thr, 1)
        k = loop.run()
        assert k == kc and (thr == 0.0 or kc == c['k']), (thr, k, kc)
        assert np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), thr
        assert loop.run() == kc and np.array_equal(loop.state(), sc)                        # a second run on the same handle


# ---- 3. impl 2, both piece formats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pieces', [2, 3])
@pytest.mark.parametrize('i', ALL)
def test_impl_two_within_the_default_paths_bounds(i, pieces):
    c = wc.CASES[i]
    wc.check_case(i)
    for max_it, thr in ((c['max_it'], 0.0),) + (((30, 0.01),) if c['k'] is not None else ()):
        (kc, sc, oc), (k64, s64, o64) = wc.oracles(i, max_it, thr)
        loop = _wide(i, max_it, thr, 2)
        assert loop.set_pieces(pieces) == pieces
        if c.get('seeded'): assert loop.set_label_projection('auto') is True                # the seeded form
        k = loop.run()
        print(f'case {i}, threshold {thr}: k {k}, gate_info {loop.gate_info()}, range_info {loop.range_info()}')
        if thr == 0.0: assert loop.gate_info()[0] == 0 and loop.range_info()[0] == 0, 'the Loop was repeated: the result is not the form\'s'
        assert k == kc == k64
        _close(loop.state(), loop.output(), sc, oc, s64, o64, f'case {i}, pieces {pieces}, threshold {thr}')


# ---- 4. second static tile and tickets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impl', [1, 2])
@pytest.mark.parametrize('i', [0, 2])
def test_capped_grids_reach_the_ticket_counter_with_the_same_bits(i, impl):
    c = wc.CASES[i]
    tiles = (c['n'] + 31) // 32
    # one workgroup: two static tiles per wave and, in case 0 (11 tiles on 4 waves), the rest by ticket; case 2 (10 tiles on 5 waves) ends
    # with the second static round, the edge of "tiles beyond 2 W exist"
    assert tiles >= 2 * c['waves'] and (i != 0 or tiles > 2 * c['waves'])
    loop = _wide(i, c['max_it'], 0.0, impl)
    k = loop.run()
    s, o = loop.state(), loop.output()
    assert loop.gate_info()[0] == 0 and loop.range_info()[0] == 0
    for limit in (1, 2):
        assert loop.set_grid_limit(limit) == limit and loop.body_launch() == (c['waves'], limit)
        assert loop.run() == k and loop.gate_info()[0] == 0 and loop.range_info()[0] == 0
        assert np.array_equal(loop.state(), s) and np.array_equal(loop.output(), o), limit
    assert loop.set_grid_limit(0) == tiles


# ---- 5. the two loaders ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 3, 4, 6])
def test_wide_loader_equals_the_generic_loader(i):
    c = wc.CASES[i]
    (kc, sc, oc), _ = wc.oracles(i, c['max_it'], 0.0)
    loop = _wide(i, c['max_it'], 0.0, 1)
    assert loop.set_wide_loader('generic') is False
    k = loop.run()
    assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc)
    assert loop.set_wide_loader('wide') is True
    assert loop.run() == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc)


# ---- 6. two ranks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sliced', [False, True])
def test_loopback_world_two_is_bit_equal_to_one_rank(sliced):
    """Row all-gather: every rank takes the form on its shard.  Feature-sliced exchange: the same launch with the given aggregate."""
    from test_gpu_sharded import _csr_parts, _sharded_loops
    e = _engine()
    c = wc.CASES[0]
    g, st, ou, s0 = wc.case(0)
    (kc, sc, oc), _ = wc.oracles(0, c['max_it'], 0.0)
    comms, graphs, loops, ranges = _sharded_loops(e, g, st, ou, c['d'], c['max_it'], 0.0, s0, 2, 1, strict=False)
    indptr, adj_src, adj_w, _, _ = _csr_parts(g)
    for gr, lp in zip(graphs, loops):
        if sliced:
            gr.set_full_adjacency(c['n'], indptr, adj_src, adj_w)
            lp.set_slice_exchange(True)
        lp.set_wide_state('always')                          # (the helper left the ranks on impl 0, where there is nothing to take)
        assert lp.set_impl(1) == 1 and lp.set_wide_state('always') is True
        assert lp.body_kernel() == 1 and lp.body_launch()[0] == c['waves']
        assert lp.set_wide_loader('wide') is (not sliced)
    k = e.Loop.run_group(loops)
    assert k == kc == c['max_it']
    assert np.array_equal(np.concatenate([lp.state() for lp in loops]), sc)
    assert np.array_equal(np.concatenate([lp.output() for lp in loops]), oc)
    for lp in loops: lp.close()
    for cm in comms: cm.close()


# ---- 7. the model surface --------------------------------------------------------------------------------------------------------------------------
def test_model_surface(tmp_path):
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject, GraphTensor
    from test_gpu_parity import _models
    c = wc.CASES[0]
    g, st, ou, s0 = wc.case(0)
    n = c['n']
    assert g['set_mask'].all() and g['output_mask'].all()
    targets = np.eye(2, dtype=np.float32)[np.random.default_rng(9190).integers(0, 2, n)]
    go = GraphObject(arcs=np.asarray(g['arcs']), nodes=np.asarray(g['nodes']), targets=targets)
    gt = GraphTensor.fromGraphObject(go)
    model = _models(st, ou, c['d'], c['max_it'], 0.0, GNNnodeBased)
    model.impl = 1
    (kc, sc, oc), _ = wc.oracles(0, c['max_it'], 0.0)
    model.set_wide_state('always')
    k, state, out = model.Loop(gt, state0=s0)
    dev_loop = model._device_loop(gt.device_graph(model.device))
    assert dev_loop.set_wide_state('always') is True and dev_loop.body_launch()[0] == c['waves']      # (the loop that ran)
    assert k == kc and np.array_equal(state, sc) and np.array_equal(out, oc)                # the _engine run's bits: the C oracle's
    # the mode survives copy() and save() / load(); a model saved before the key existed loads as off
    assert model.copy().wide_state == 'always'
    model.save(str(tmp_path / 'm'))
    assert GNNnodeBased.load(str(tmp_path / 'm')).wide_state == 'always'
    import json
    cfg = json.load(open(tmp_path / 'm' / 'config.json'))
    del cfg['wide_state']
    json.dump(cfg, open(tmp_path / 'm' / 'config.json', 'w'))
    assert GNNnodeBased.load(str(tmp_path / 'm')).wide_state == 'off'
    # an LGNN forwards it
    lgnn = LGNN([model.copy(), model.copy()], False, True, None, None, None, 'c')
    lgnn.set_wide_state('auto')
    assert [m.wide_state for m in lgnn.gnns] == ['auto', 'auto']
    # a training step does not take the form: the same bits with the mode on and off
    from GNN import optimizers
    steps = {}
    for mode in ('off', 'always'):
        m = model.copy()
        m.optimizer = optimizers.SGD(learning_rate=0.01)
        m.set_wide_state(mode)
        m.seed = 3
        res = m.training_step(gt, True, state0=s0)
        steps[mode] = [np.float64(res['loss']), np.float64(res['k'])] + [np.array(w) for w in m.net_state.get_weights() + m.net_output.get_weights()]
    assert np.isfinite(steps['off'][0]) and steps['off'][1] >= 1
    assert len(steps['off']) == len(steps['always']) and all(np.array_equal(a, b) for a, b in zip(steps['off'], steps['always']))
