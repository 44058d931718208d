"""Label projection (gnn_loop_set_label_projection) on the GPU: the projection kernel against the float64 product, seeded Loops against
the C oracle (the bit-exact fp32 chain) and the float64 oracle, the cache keys, the exact paths beside it, two ranks, a model.

Bounds, none of them measured on the code under test:
  projection   per element IW 2^-24 sum_k |x_k w_k| + ulp: the order-free fp32 dot-product bound;
  states       1e-5 from the float64 oracle (the default path's contract, README) and 2e-6 max(1, max |state|) from the C oracle, the bound
               test_gpu_parity.test_wide_states_and_fallback holds the unseeded split path to; outputs the same.
Loops at threshold 0 run a fixed number of bodies, chosen so that every gate of the run, the last included, sees a robust mover of the
certified gate on the fp32 oracle (label_projection_cases.mover_margin; 10 to 2,800 times the band): no certified-gate repeat may
replace the seeded result by the per-op one, and the tests assert that none happened."""
import numpy as np
import pytest

import label_projection_cases as lc
from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp

pytestmark = pytest.mark.gpu


def _engine():
    from GNN import _engine
    return _engine


def _device_graph(g):
    e = _engine()
    mask = np.logical_and(g['set_mask'], g['output_mask'])
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    return e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'], mask)


def _loop(g, st, ou, d, max_it, thr, s0, mst=None):
    e = _engine()
    mst = mst or e.Mlp(st['weights'], st['activations'], st['batch_normalization'])
    loop = e.Loop(_device_graph(g), mst, e.Mlp(ou['weights'], ou['activations'], ou['batch_normalization']), d, max_it, thr)
    if d: loop.set_state0(s0)
    return loop


def _close(s, o, sc, oc, s64, o64, what=''):
    tol = 2e-6 * max(1.0, float(np.max(np.abs(sc))))
    e64, ec = float(np.max(np.abs(s - s64))), float(np.max(np.abs(s - sc)))
    eo64, eoc = float(np.max(np.abs(o - o64))), float(np.max(np.abs(o - oc)))
    print(f'{what}: |state - f64| {e64:.2e}, |state - C oracle| {ec:.2e} (bound {tol:.2e}), |out - f64| {eo64:.2e}, |out - C oracle| {eoc:.2e}')
    assert e64 <= 1e-5 and ec <= tol and eo64 <= 1e-5 and eoc <= tol, (what, e64, ec, tol, eo64, eoc)


# ---- (a) the projection kernel alone -----------------------------------------------------------------------------------------------------------
# (n, IW, H1) -> a loop that has them: IW = 2 nl + al (d > 0) or al (d == 0: the state is the label table), H1 the first hidden width
PROJECTIONS = [
    pytest.param(dict(n=31, d=0, nl=48, al=1, hidden=(20,), act='tanh'), 1, 20, 2, id='31-1-20'),
    pytest.param(dict(n=333, d=64, nl=21, al=3, hidden=(128,), act='tanh'), 45, 128, 1, id='333-45-128'),
    pytest.param(dict(n=320, d=20, nl=150, al=2, hidden=(64,), act='tanh'), 302, 64, 1, id='320-302-64'),
    pytest.param(dict(n=65, d=32, nl=40, al=3, hidden=(32, 32), act='tanh'), 83, 32, 1, id='65-83-32'),
]


@pytest.mark.parametrize('shape,iw,h1,mode', PROJECTIONS)
def test_projection_kernel_against_float64(shape, iw, h1, mode):
    g, st, ou, s0 = lc.build(7100 + iw, **shape)
    d = shape['d']
    loop = _loop(g, st, ou, d, 2, 0.0, s0)
    assert loop.set_label_projection(mode) is True
    loop.run()
    p = loop.label_projection()
    x = lc.label_block(g, d)
    wl, b1 = lc.label_rows(st, d if d else shape['nl'], shape['nl'] if d else 0)
    assert x.shape == (shape['n'], iw) and wl.shape == (iw, h1) and p.shape == (shape['n'], h1)
    ref = x.astype(np.float64) @ wl.astype(np.float64) + b1.astype(np.float64)
    bound = iw * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(wl).astype(np.float64)) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(p.astype(np.float64) - ref)
    print(f'projection {shape["n"]} x {iw} x {h1}: max error {err.max():.2e}, max error / bound {np.max(err / bound):.3f}')
    assert np.all(np.isfinite(p)) and np.all(err <= bound), (float(err.max()), float(np.max(err / bound)))
    loop.drop_cached_aggregates()                      # the next run rebuilds the block and the projection
    loop.run()
    assert np.array_equal(loop.label_projection(), p), 'two runs of the projection differ'


# ---- (b) Loops at threshold 0 --------------------------------------------------------------------------------------------------------------------
def _forms():
    out = []
    for i, c in enumerate(lc.CASES):
        for pieces in (2, 3):
            for gather in ((1, 2) if c['kernel'] == 2 else (0,)):
                out.append(pytest.param(i, pieces, gather, id=f'case{i}-pieces{pieces}-gather{gather}'))
    return out


@pytest.mark.parametrize('i,pieces,gather', _forms())
def test_seeded_loop_at_threshold_zero(i, pieces, gather):
    c = lc.CASES[i]
    margin, bodies = lc.mover_margin(i, c['max_it'])
    assert bodies == c['max_it'] and margin > 5.0, f'the case has no robust mover at every gate (margin {margin:.1f} x band)'
    g, st, ou, s0 = lc.case(i)
    (kc, sc, oc), (k64, s64, o64) = lc.oracles(i, c['max_it'], 0.0)
    loop = _loop(g, st, ou, c['d'], c['max_it'], 0.0, s0)
    assert loop.set_pieces(pieces) == pieces
    if gather: loop.set_gather_form(gather)
    assert loop.set_label_projection(1) is True and loop.body_kernel() == c['kernel']
    if gather == 2 and c['n'] >= 32: assert loop.set_gather_form(2) == 2
    k = loop.run()
    assert loop.gate_info()[0] == 0 and loop.range_info()[0] == 0, 'the Loop was repeated: the result is not the seeded kernels\''
    assert k == kc == k64 == c['max_it']
    _close(loop.state(), loop.output(), sc, oc, s64, o64, f'case {i}, pieces {pieces}, gather {gather}')


# ---- (c) converging Loops --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', lc.CONVERGING)
def test_seeded_loop_converges_with_the_oracles_k(i):
    c = lc.CASES[i]
    g, st, ou, s0 = lc.case(i)
    (kc, sc, oc), (k64, s64, o64) = lc.oracles(i, 30, 0.01)
    assert kc == k64 == c['k']
    loop = _loop(g, st, ou, c['d'], 30, 0.01, s0)
    assert loop.set_label_projection('auto') is True
    k = loop.run()
    print(f'case {i}: k {k}, gate_info {loop.gate_info()}, range_info {loop.range_info()}')
    assert k == kc
    _close(loop.state(), loop.output(), sc, oc, s64, o64, f'case {i}, threshold 0.01')


# ---- (d) mode 2 on narrow labels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,hidden,kernel', [(64, (128, 128), 2), (20, (64,), 1)])
def test_mode_two_on_narrow_labels_against_the_unseeded_kernel(d, hidden, kernel):
    g, st, ou, s0 = lc.build(7200 + d, n=333, d=d, nl=3, al=2, hidden=hidden, act='selu')
    kc, sc, oc = corc.loop_node(g, st, ou, d, 12, 0.01, s0)
    loop = _loop(g, st, ou, d, 12, 0.01, s0)
    loop.set_persistent(False)                          # (a narrow net on few rows runs in the persistent launch, which stays as it is)
    assert loop.set_label_projection(1) is False        # covered as it stands
    k0 = loop.run()
    s_un, o_un = loop.state(), loop.output()
    assert loop.set_label_projection(2) is True and loop.body_kernel() == kernel
    k2 = loop.run()
    s_se, o_se = loop.state(), loop.output()
    assert k0 == k2 == kc
    tol = 2e-6 * max(1.0, float(np.max(np.abs(sc))))
    print(f'd {d}: seeded - unseeded {np.max(np.abs(s_se - s_un)):.2e}, seeded - C oracle {np.max(np.abs(s_se - sc)):.2e}, unseeded - C oracle {np.max(np.abs(s_un - sc)):.2e}')
    assert np.max(np.abs(s_se - sc)) <= tol and np.max(np.abs(o_se - oc)) <= tol and np.max(np.abs(s_se - s_un)) <= 2 * tol
    assert loop.set_label_projection(0) is False
    assert loop.run() == k0 and np.array_equal(loop.state(), s_un) and np.array_equal(loop.output(), o_un)      # off: today's bits


# ---- (e) cache keys --------------------------------------------------------------------------------------------------------------------------------
def test_projection_follows_the_weights():
    e = _engine()
    c = lc.CASES[5]
    g, st, ou, s0 = lc.case(5)
    _, st_new, _, _ = lc.build(7300, **c)
    mst = e.Mlp(st['weights'], st['activations'], True)
    loop = _loop(g, st, ou, c['d'], 2, 0.0, s0, mst)
    assert loop.set_label_projection(1) is True
    loop.run()
    p_old = loop.label_projection()
    mst.set_weights(st_new['weights'])
    k = loop.run()
    fresh = _loop(g, st_new, ou, c['d'], 2, 0.0, s0)
    assert fresh.set_label_projection(1) is True
    kf = fresh.run()
    assert k == kf and np.array_equal(loop.state(), fresh.state()) and np.array_equal(loop.output(), fresh.output())
    assert np.array_equal(loop.label_projection(), fresh.label_projection()) and not np.array_equal(loop.label_projection(), p_old)


def test_projection_follows_the_labels_through_an_lgnn_stack():
    """Two layers, outputs propagated: layer 2's labels are layer 1's widened by its outputs, rewritten on the device in every Loop of the
    stack - the second Loop() call, from other initial states, must not reuse the projection of the first."""
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject
    from test_gpu_parity import _models
    from util import random_arcs
    rng = np.random.default_rng(7400)
    n, nl, al, d, max_it = 333, 14, 3, 64, 4
    arcs = random_arcs(rng, n, 3 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    go = GraphObject(arcs=arcs, nodes=nodes, targets=np.zeros((n, 2)))
    gd = orc.make_graph_dict(arcs, nodes, 'average')
    gnns, models = [], []
    for layer in range(2):
        ins, ls = orc.get_inout_dims('state', nl, al, 2, 'n', d, [128, 128], layer=layer, get_output=True)
        ino, lo = orc.get_inout_dims('output', nl, al, 2, 'n', d, None, layer=layer, get_output=True)
        st, ou = make_mlp(rng, ins, ls, 'selu', gain=0.5, bn_random=True), make_mlp(rng, ino, lo, 'softmax', bn_random=True)
        gnns.append(dict(net_state=st, net_output=ou, state_vect_dim=d, max_iteration=max_it, threshold=0.0))
        models.append(_models(st, ou, d, max_it, 0.0, GNNnodeBased))
        models[-1].impl = 2
    assert gnns[1]['net_state']['weights'][0].shape[0] == gnns[0]['net_state']['weights'][0].shape[0] + 4      # layer 2: two more label columns
    lgnn = LGNN(models, False, True, None, None, None, 'c')
    lgnn.set_label_projection('auto')
    states = []
    for call in range(2):
        s0s = [(0.1 * rng.standard_normal((n, d))).astype(np.float32) for _ in range(2)]
        K, state, outs = lgnn.Loop(go, state0=s0s)
        gtmp, Kc = dict(gd), []                        # the bit-exact chain: C oracle per layer + the reference's relabelling rule
        for gnn, s0 in zip(gnns, s0s):
            kc, sc, oc = corc.loop_node(gtmp, gnn['net_state'], gnn['net_output'], d, max_it, 0.0, s0)
            Kc.append(kc)
            gtmp = orc.update_graph(gd, sc, oc, False, True)
        K64, s64, o64 = orc.lgnn_loop(gd, gnns, False, True, False, s0s, np.float64)
        assert K == Kc == K64
        _close(state, outs[-1], sc, oc, s64, o64[-1], f'LGNN, call {call}')
        states.append(state)
    assert not np.array_equal(states[0], states[1])


# ---- (f) the exact path beside it ------------------------------------------------------------------------------------------------------------------
def test_impl_one_runs_as_without_the_projection():
    c = lc.CASES[5]
    g, st, ou, s0 = lc.case(5)
    (kc, sc, oc), _ = lc.oracles(5, 30, 0.01)
    loop = _loop(g, st, ou, c['d'], 30, 0.01, s0)
    assert loop.set_label_projection(1) is True
    for impl in (1, 0):
        loop.set_impl(impl)
        assert loop.set_label_projection(1) is False
        k = loop.run()
        assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), impl
        with pytest.raises(Exception): loop.label_projection()
    loop.set_impl(2)
    assert loop.set_label_projection(1) is True


def test_uncertified_gate_repeats_on_the_per_op_path():
    """Case 2 (one partial tile) has converged inside the certified gate's band after five bodies: at threshold 0 the gate of a sixth body
    is decided by borderline nodes alone, and the seeded run is repeated on impl 1 - per-op kernels, this net is too wide for the exact fused kernel - and the caller gets that run's
    k / state / output, the oracle's bits."""
    c = lc.CASES[2]
    g, st, ou, s0 = lc.case(2)
    margin, _ = lc.mover_margin(2, 6)
    kc, sc, oc = corc.loop_node(g, st, ou, c['d'], 6, 0.0, s0)
    loop = _loop(g, st, ou, c['d'], 6, 0.0, s0)
    assert loop.set_label_projection(1) is True
    k = loop.run()
    print(f'margin {margin:.2f} x band, gate_info {loop.gate_info()}')
    if loop.gate_info()[0]:
        assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc)
    else:
        assert k == kc and np.max(np.abs(loop.state() - sc)) <= 2e-6 * max(1.0, float(np.max(np.abs(sc))))
    assert margin < 1.0 and loop.gate_info()[0], 'the case was chosen to end inside the band'
    assert loop.set_label_projection(1) is True and loop.run() == kc      # and the next run is seeded again


# ---- (g) two ranks ---------------------------------------------------------------------------------------------------------------------------------
def test_loopback_world_two_is_bit_equal_to_one_rank():
    from test_gpu_sharded import _sharded_loops
    e = _engine()
    c = lc.CASES[0]
    g, st, ou, s0 = lc.case(0)
    one = _loop(g, st, ou, c['d'], c['max_it'], 0.0, s0)
    one.set_gather_form(1)
    assert one.set_label_projection(1) is True
    k1 = one.run()
    comms, graphs, loops, ranges = _sharded_loops(e, g, st, ou, c['d'], c['max_it'], 0.0, s0, 2, 2, strict=False)
    for lp in loops:
        lp.set_impl(2); lp.set_gather_form(1)
        assert lp.set_label_projection(1) is True and lp.body_kernel() == 2
    k2 = e.Loop.run_group(loops)
    assert all(lp.gate_info()[0] == 0 and lp.range_info()[0] == 0 for lp in loops + [one])
    assert k1 == k2 == c['max_it']
    assert np.array_equal(np.concatenate([lp.state() for lp in loops]), one.state())
    assert np.array_equal(np.concatenate([lp.output() for lp in loops]), one.output())
    assert np.array_equal(np.concatenate([lp.label_projection() for lp in loops]), one.label_projection())


# ---- (h) a model -----------------------------------------------------------------------------------------------------------------------------------
def test_graph_based_model_on_a_mutag_batch():
    import load_MUTAG
    from GNN.GNN import GNNgraphBased
    from GNN.graph_class import GraphObject, GraphTensor
    from test_gpu_parity import _models
    rng = np.random.default_rng(7500)
    graphs = load_MUTAG.load(limit=32)
    batch = GraphTensor.fromGraphObject(GraphObject.merge(graphs, problem_based='g', aggregation_mode='average'))
    d = 64
    st = make_mlp(rng, 3 + 2 * (d + 14), [128, 128, d], 'selu', gain=0.5, bn_random=True)
    ou = make_mlp(rng, d + 14, [2], 'softmax', bn_random=True)
    gnn = _models(st, ou, d, 20, 0.01, GNNgraphBased)
    gnn.impl = 2
    res = {}
    for mode in ('off', 'auto'):
        gnn.set_label_projection(mode)
        gnn.seed = 5
        res[mode] = gnn.evaluate_single_graph(batch, training=False)
        assert gnn._device_loop(batch.device_graph(gnn.device)).set_label_projection(mode) is (mode == 'auto')      # (the loop that ran)
    (it0, loss0, _, out0), (it1, loss1, _, out1) = res['off'], res['auto']
    print(f'MUTAG batch: iterations {it0} / {it1}, loss {loss0:.6f} / {loss1:.6f}, max |out| difference {np.max(np.abs(out0 - out1)):.2e}')
    assert it0 == it1 and abs(loss0 - loss1) <= 1e-5 * max(1.0, abs(loss0)) and np.max(np.abs(out0 - out1)) <= 1e-5
