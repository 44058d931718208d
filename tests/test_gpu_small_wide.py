"""The persistent small-graph launch for net_state hidden layers up to 64 wide (k_small16 with WIDE, csrc/gnn_small16_kernel.h): one launch runs
the initial state, the first condition, every body and the output stage of a Loop on up to 4,096 nodes when net_state has two or three
layers, hidden layers <= 64 (one of them > 32), a state <= 32 and a concat <= 96 wide.  The arithmetic is the exact f32-MFMA chain under
impl 1 and 2: k, states and outputs are bit-identical to the C oracle and to one launch per body.  The shapes are the smallest that reach
each layout decision of the kernel."""
import functools
import os

import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

ALL_GATES = ((0.01, 30), (0.0, 7), (0.01, 0), (1e9, 5))
ONE_GATE = ((0.01, 30),)
ACTS = ['linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid']


def _engine():
    from GNN import _engine
    return _engine


@functools.lru_cache(maxsize=None)
def _case(seed, n, d, nl, al, hidden, acts, deg=3):
    """A seeded random graph with a set_mask of 80 % and random nets (BatchNormalization with random statistics); acts: one name for all
    layers of net_state or the whole list.  Built once per key and never changed."""
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, deg * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    ds, nls = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nls), list(hidden) + [ds], acts if isinstance(acts, str) else 'selu', gain=0.6, bn_random=True)
    if not isinstance(acts, str): st['activations'] = list(acts)
    ou = make_mlp(rng, ds + nls, [2], 'softmax', bn_random=True)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
    g['set_mask'] = rng.random(n) < 0.8
    return g, st, ou, s0


@functools.lru_cache(maxsize=None)
def _oracle(key, thr, max_it):
    g, st, ou, s0 = _case(*key)
    return corc.loop_node(g, st, ou, key[2], max_it, thr, s0)


def _device(e, key):
    g, st, ou, s0 = _case(*key)
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    graph = e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'],
                    np.logical_and(g['set_mask'], g['output_mask']))
    return graph, e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True), s0


def _same(loop, want):
    kc, sc, oc = want
    k = loop.run()
    return k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc)


def _check(key, gates):
    """The persistent launch is taken; impl 1 and 2, twice per handle: the C oracle's bits; then one launch per body (impl 1): the same"""
    e = _engine()
    d = key[2]
    graph, mst, mou, s0 = _device(e, key)
    for thr, max_it in gates:
        want = _oracle(key, thr, max_it)
        for impl in (1, 2):
            loop = e.Loop(graph, mst, mou, d, max_it, thr)
            assert loop.set_impl(impl) == impl
            assert loop.set_persistent(True) is True, key
            if d: loop.set_state0(s0)
            for rep in range(2):
                assert _same(loop, want), (key, thr, max_it, impl, rep)
            if impl == 1:
                assert loop.set_persistent(False) is False
                assert _same(loop, want), (key, thr, max_it, 'one launch per body')
            loop.close()
    graph.close()


SHAPES = {   # id: (seed, n, d, nl, al, hidden, act, deg), gates
    'two_layers_partial_tile': ((8101, 333, 8, 3, 2, (64,), 'selu', 3), ALL_GATES),        # 21 tiles, the last with 13 rows; 64-byte exchange rows
    'mutag_widened': ((8102, 970, 0, 14, 3, (64, 64), 'selu', 3), ALL_GATES),              # D = 0, three layers
    'concat_96': ((8103, 100, 32, 15, 2, (33, 64), 'tanh', 3), ONE_GATE),                  # S0 = 24, one valid feature in the third hidden tile,
                                                                                           # 128-byte exchange rows, two last-layer tiles
    'one_row_tile_state_1': ((8104, 17, 1, 1, 1, (48,), 'relu', 3), ONE_GATE),             # two tiles, the second with one row
    'all_workgroups': ((8105, 4096, 16, 4, 1, (64, 64), 'selu', 11), ONE_GATE),            # 256 workgroups, eight arcs per gather round
    'uncached_gather': ((8106, 200, 8, 3, 1, (40,), 'elu', 70), ONE_GATE),                 # more than 1,024 arcs per tile
    'narrow_then_wide': ((8107, 300, 8, 3, 2, (16, 64), 'sigmoid', 3), ONE_GATE),
    'wide_then_narrow': ((8108, 300, 8, 3, 2, (64, 16), 'selu', 3), ONE_GATE),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_wide_persistent_launch_shapes(name):
    key, gates = SHAPES[name]
    g, st, _, _ = _case(*key)
    dims = [st['weights'][0].shape[0]] + [st['weights'][2 * i].shape[1] for i in range(len(st['activations']))]
    f = _engine().small_form(dims, st['activations'], key[1])
    assert f['persistent'] and f['wide'] and f['tile'] == 16, (name, f)
    if name == 'concat_96': assert dims[0] == 96 and f['steps'] == 24
    if name == 'uncached_gather':
        ip = np.asarray(g['adjT'][0])
        assert max(int(ip[min(i + 16, key[1])] - ip[i]) for i in range(0, key[1], 16)) > 1024
    _check(key, gates)


@pytest.mark.parametrize('act', ACTS)
def test_every_activation(act):
    _check((8200 + ACTS.index(act), 333, 8, 3, 2, (64, 64), act, 3), ONE_GATE)


@pytest.mark.parametrize('acts', [('tanh', 'tanh', 'linear'), ('relu', 'sigmoid')], ids='-'.join)
def test_last_layer_with_its_own_activation(acts):
    _check((8300 + len(acts), 333, 8, 3, 2, (64,) * (len(acts) - 1), acts, 3), ONE_GATE)


def test_run_many_runs_wide_loops_side_by_side():
    """three wide loops of different sizes in one gnn_loop_run_many call: what each returns alone, on two calls in a row"""
    e = _engine()
    keys = [(8401, 570, 0, 14, 3, (64, 64), 'selu', 3), (8402, 300, 8, 3, 2, (48,), 'tanh', 3), (8403, 1999, 20, 2, 1, (64, 40), 'relu', 3)]
    loops, want, graphs = [], [], []
    for key in keys:
        graph, mst, mou, s0 = _device(e, key)
        lp = e.Loop(graph, mst, mou, key[2], 20, 0.01)
        assert lp.set_impl(1) == 1 and lp.set_persistent(True) is True
        if key[2]: lp.set_state0(s0)
        loops.append(lp); graphs.append(graph)
        want.append(_oracle(key, 0.01, 20))
    for _ in range(2):
        ks = e.Loop.run_many(loops)
        for lp, k, (kc, sc, oc) in zip(loops, ks, want):
            assert k == kc and np.array_equal(lp.state(), sc) and np.array_equal(lp.output(), oc)
    assert all(lp.set_persistent(True) for lp in loops)              # no launch gave up
    for lp, w in zip(loops, want):
        assert _same(lp, w)                                          # ... and alone
    for lp in loops: lp.close()
    for graph in graphs: graph.close()


def test_graph_based_model_with_wide_hidden_layers():
    """GNNgraphBased with MLP hidden [64, 64] on a MUTAG batch: Loop(g) with the persistent launch allowed and forbidden (impl 1), and a
    second call with it allowed, where the graph readout is folded into the launch - the same bits every time, and the C oracle's"""
    import load_MUTAG
    from GNN import losses
    from GNN.GNN import GNNgraphBased
    from GNN.MLP import MLP
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(85)
    batch = GraphObject.merge(load_MUTAG.load(limit=32), problem_based='g', aggregation_mode='average')
    st, ou = make_mlp(rng, 3 + 2 * 14, [64, 64, 14], 'selu', gain=0.7), make_mlp(rng, 14, [2], 'softmax')

    def build(net):
        w = net['weights']
        m = MLP(input_dim=w[0].shape[0], layers=[w[2 * i].shape[1] for i in range(len(net['activations']))], activations=net['activations'],
                kernel_initializer='zeros', bias_initializer='zeros', batch_normalization=net['batch_normalization'])
        m.set_weights(w)
        return m

    gnn = GNNgraphBased(net_state=build(st), net_output=build(ou), optimizer=None, loss_function=losses.categorical_crossentropy,
                        loss_arguments=None, state_vect_dim=0, max_iteration=50, threshold=0.01, addressed_problem='c')
    gnn.impl = 1
    gt = GraphTensor.fromGraphObject(batch)
    k, s, o = gnn.Loop(gt)
    loop = gnn._device_loop(gt.device_graph(gnn.device))
    assert loop.set_persistent(True) is True
    gd = orc.make_graph_dict(batch.arcs, batch.nodes, 'average', NodeGraph=batch.NodeGraph)
    kc, sc, on = corc.loop_node(gd, st, ou, 0, 50, 0.01)
    assert k == kc and np.array_equal(s, sc) and o.shape == (32, 2) and np.array_equal(o, corc.readout(batch.NodeGraph, on))
    k2, s2, o2 = gnn.Loop(gt)                                        # the NodeGraph is cached with the loop now: folded readout
    assert k2 == k and np.array_equal(s2, s) and np.array_equal(o2, o)
    assert loop.set_persistent(False) is False
    k3, s3, o3 = gnn.Loop(gt)
    assert k3 == k and np.array_equal(s3, s) and np.array_equal(o3, o)
