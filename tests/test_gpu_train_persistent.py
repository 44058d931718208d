"""The persistent training forward of small batches (gnn_loop_set_train_persistent: every body of net_state in ONE launch) against the
per-body launches it replaces: the two forms of the SAME loop must agree bit for bit in k, published state, outputs, loss,
BatchNormalization statistics and every gradient (np.array_equal), at the row counts where the kernel changes shape (tile, chunk and
rows-per-workgroup edges), at every stopping point, and after an inference run; the persistent form against the float64 oracle at the
tolerances of tests/test_gpu_train.py; models get it without a change to their Python."""
import functools
import os

import numpy as np
import pytest

from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

NL, AL, T = 3, 2, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mutag_raw.npz')


def _graph(rng, n, sizes=None):
    """Random graph on n nodes (n == 1: no arcs); sizes: node counts of the graphs it is a merged batch of (graph-based readout)."""
    arcs = random_arcs(rng, n, 3 * n, AL) if n > 1 else np.zeros((0, 2 + AL), np.float32)
    nodes = (2 * rng.random((n, NL)) - 1).astype(np.float32)
    return arcs, nodes, sizes


@functools.lru_cache(maxsize=None)
def _mutag_batch():
    """The first 32 molecules of the MUTAG fixture as one merged batch: (arcs with one-hot labels, one-hot node labels, nodes per graph)."""
    import load_MUTAG
    load_MUTAG._PACKED = GOLDEN
    graphs = load_MUTAG.load(limit=32)
    arcs, nodes, sizes, off = [], [], [], 0
    for g in graphs:
        a = np.asarray(g.arcs, np.float32).copy()
        a[:, :2] += off
        arcs.append(a); nodes.append(np.asarray(g.nodes, np.float32)); sizes.append(g.nodes.shape[0])
        off += g.nodes.shape[0]
    return np.concatenate(arcs), np.concatenate(nodes), tuple(sizes)


def _ng_csr(sizes):
    """NodeGraph^T as a CSR over graphs with average weights, and the dense [N, G] matrix the oracle takes."""
    n, G = int(sum(sizes)), len(sizes)
    ip = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    w = np.concatenate([np.full(s, 1.0 / s, np.float32) for s in sizes])
    dense = np.zeros((n, G), np.float32)
    for gi in range(G): dense[ip[gi]:ip[gi + 1], gi] = 1.0 / sizes[gi]
    return (ip, np.arange(n, dtype=np.int32), w), dense


class Case:
    """One loop with everything a training step needs; step() runs it in one of the two forms."""

    def __init__(self, e, seed, arcs, nodes, sizes, hidden, act, last_act, bn, d, max_it, thr, gain=0.8, edge=False, rows_masked=None, s0=None):
        rng = np.random.default_rng(seed)
        self.e, self.n, self.d, self.max_it, self.thr, self.edge = e, nodes.shape[0], d, max_it, thr, edge
        n, nl, al = self.n, nodes.shape[1], arcs.shape[1] - 2
        self.ng_csr, ng = _ng_csr(sizes) if sizes else (None, None)
        self.g = g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
        ds, nlc = (d if d else nl), (nl if d else 0)
        self.st = make_mlp(rng, al + 2 * (ds + nlc), list(hidden) + [ds], act, batch_normalization=bn, out_activation=last_act, gain=gain, bn_random=True)
        self.ou = make_mlp(rng, (2 * (ds + nlc) + al) if edge else ds + nlc, [T], 'tanh', out_activation='softmax', bn_random=True)
        self.st['dropout'], self.ou['dropout'] = {}, {}
        if edge:
            mask = rng.random(len(arcs)) < 0.75
            g['set_mask'], g['output_mask'] = mask, np.ones(len(arcs), bool)
            graph_mask = np.ones(n, np.uint8)
        else:
            mask = np.ones(n, bool) if (sizes or rows_masked is None) else rows_masked
            g['set_mask'] = mask
            graph_mask = mask
        self.m = int(mask.sum())
        n_t = len(sizes) if sizes else self.m
        self.targets = np.eye(T)[rng.integers(0, T, n_t)].astype(np.float32)
        self.weights = rng.uniform(0.5, 1.5, n_t).astype(np.float32)
        drawn = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
        self.s0 = s0 if s0 is not None else drawn
        arc_lab = np.asarray(arcs, np.float32)[:, 2:]
        self.graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_lab[g['arcT'][1]], nodes, graph_mask)
        self.mst, self.mou = e.Mlp(self.st['weights'], self.st['activations'], bn), e.Mlp(self.ou['weights'], self.ou['activations'], True)
        self.loop = e.Loop(self.graph, self.mst, self.mou, d, max_it, thr)
        if edge:
            self.graph.set_arc_order(g['arcT'][1], arc_lab)
            self.loop.set_edge_readout(np.repeat(np.arange(n, dtype=np.int32), np.diff(g['adjT'][0])), arc_lab, mask)
        if d: self.loop.set_state0(self.s0)

    def step(self, persistent, must_take=True, **kw):
        """One train_step in the given form -> everything the step returns plus the published state / outputs."""
        used = self.loop.set_train_persistent(persistent)
        res = self.loop.train_step(self.mst, self.mou, None, self.targets, self.weights, 0, self.ng_csr, seed=7, **kw)
        info = self.loop.train_info()
        if must_take: assert used == persistent and info['persistent'] == persistent, (used, info)
        res.update(state=self.loop.state(), out=self.loop.output(), info=info)
        return res

    def forward_backward(self, persistent):
        """train_forward + train_backward with the label (and, edge-based, arc-label) gradients requested."""
        assert self.loop.set_train_persistent(persistent) == persistent
        k, out = self.loop.train_forward(self.mst, self.mou, None, seed=7)
        assert self.loop.train_info()['persistent'] == persistent
        state = self.loop.state()
        d_out = np.random.default_rng(5).standard_normal(out.shape).astype(np.float32)
        res = self.loop.train_backward(d_out, want_d_nodes=True, want_d_arcs=self.edge)
        res.update(k=k, out=out, state=state)
        return res

    def oracle(self, **kw):
        return tro.train_step(self.g, self.st, self.ou, self.d, self.max_it, self.thr, self.s0, [{}] * self.max_it, {}, self.targets, self.weights,
                              mean=False, graph_based=self.ng_csr is not None, **kw)


def same(a, b, keys=('k', 'loss', 'state', 'out', 'bn_batch_state', 'bn_batch_output', 'd_nodes', 'd_arcs')):
    for key in keys:
        if key in a or key in b:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    for x, y in zip(a['grads_state'] + a['grads_output'], b['grads_state'] + b['grads_output']):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert np.isfinite(a['loss'] if 'loss' in a else 0.0) and all(np.isfinite(x).all() for x in a['grads_state'] + a['grads_output'])


@pytest.fixture(scope='module')
def e():
    from GNN import _engine
    return _engine


# rows: 1; the 16-row tile edge; the 32-row chunk edge; rows_per_block 32 -> 48 at 2,049; the last eligible count.  The nets walk through
# two and three Dense layers, hidden widths 8 / 32 / 40, selu / tanh / relu, a last layer with its own activation, with and without
# BatchNormalization (a state wider than 32 takes two column blocks of its statistics), a softmax last layer, state_vect_dim 0 and > 0,
# node-based and graph-based (NodeGraph CSR) readout.
FORMS = [
    (1, (8,), 'selu', None, True, 4, False), (15, (32,), 'tanh', None, False, 0, False), (16, (40,), 'relu', 'tanh', True, 5, True),
    (17, (8, 32), 'tanh', 'sigmoid', False, 6, False), (32, (32, 8), 'selu', None, True, 0, True), (33, (40, 40), 'relu', None, True, 4, False),
    (2048, (32,), 'tanh', None, True, 4, True), (2049, (8, 8), 'selu', 'tanh', False, 0, False), (4095, (40,), 'tanh', None, True, 6, True),
    (33, (8,), 'tanh', 'softmax', True, 4, False), (70, (16,), 'tanh', None, True, 40, False),
]


@pytest.mark.parametrize('n,hidden,act,last_act,bn,d,graph_based', FORMS)
def test_forms_agree_bit_for_bit(e, n, hidden, act, last_act, bn, d, graph_based):
    rng = np.random.default_rng(n)
    sizes = None
    if graph_based:
        cut = sorted(set([0, n // 3, n // 2, n]))
        sizes = tuple(b - a for a, b in zip(cut[:-1], cut[1:]) if b > a)
    c = Case(e, n + 1, *_graph(rng, n, sizes), hidden, act, last_act, bn, d, 3, 0.0, rows_masked=None if graph_based else rng.random(n) < 0.8 if n > 1 else None)
    on, off = c.step(True), c.step(False)
    # (one row under BatchNormalization: the batch variance is 0, the state is beta from the first body on and the loop stops after the second)
    assert on['k'] == (3 if n > 1 else 2) and on['info']['barriers_per_body'] == (2 if bn else 1)
    assert on['info']['workgroups'] == -(-n // (32 if n <= 2048 else 48 if n <= 3072 else 64))
    same(on, off)


@pytest.mark.parametrize('bn', [False, True])
def test_mutag_batch_forms_agree(e, bn):
    arcs, nodes, sizes = _mutag_batch()
    c = Case(e, 3, arcs, nodes, sizes, (32, 32), 'selu', None, bn, 0, 6, 0.0, gain=0.6)
    assert len(sizes) == 32 and c.n > 32
    on, off = c.step(True), c.step(False)
    assert on['k'] == 6
    same(on, off)


@pytest.mark.parametrize('edge', [False, True])
def test_label_gradients_agree(e, edge):
    """d_nodes (and, edge-based with the arc order set, d_arcs) through train_forward / train_backward."""
    rng = np.random.default_rng(21)
    c = Case(e, 22, *_graph(rng, 70), (8,), 'tanh', None, True, 4, 3, 0.0, edge=edge)
    on, off = c.forward_backward(True), c.forward_backward(False)
    assert on['d_nodes'] is not None and (on['d_arcs'] is not None) == edge and np.abs(on['d_nodes']).max() > 0
    same(on, off)


def _contraction_rates(c, bodies):
    """r[i] = max over the nodes of |s_i - s_{i-1}| / |s_{i-1}| along the float64 oracle's trajectory (s_{-1} = ones): gate i is open iff
    threshold < r[i]."""
    states = [np.ones_like(c.s0, np.float64), np.asarray(c.s0, np.float64)]
    for it in range(1, bodies + 1):
        states.append(tro.train_forward(c.g, c.st, c.ou, c.d, it, 0.0, c.s0, [{}] * it, {})['state'])
    return [float(np.max(np.linalg.norm(b - a, axis=1) / np.linalg.norm(a, axis=1))) for a, b in zip(states[:-1], states[1:])]


@pytest.mark.parametrize('want_k,max_it', [(1, 7), (3, 7), (7, 7), (1, 1)])
def test_stops_where_the_oracle_stops(e, want_k, max_it):
    """A contractive net without BatchNormalization: thresholds between two contraction rates of the oracle's trajectory, so that the oracle
    alone gives k = 1, a k strictly inside and k = max_iter."""
    rng = np.random.default_rng(31)
    arcs, nodes, _ = _graph(rng, 90)
    probe = Case(e, 32, arcs, nodes, None, (10,), 'tanh', None, False, 5, 7, 0.0, gain=1.2)
    # (start two bodies into the oracle's trajectory: from a random state the first body moves further than the start is away from ones)
    s0 = tro.train_forward(probe.g, probe.st, probe.ou, 5, 2, 0.0, probe.s0, [{}] * 2, {})['state'].astype(np.float32)
    probe.s0 = s0
    r = _contraction_rates(probe, 7)
    assert all(r[i + 1] < 0.8 * r[i] for i in range(7)) and r[7] > 1e-3, r      # a contraction: the gates close in order, with a margin far above float32 rounding
    thr = float(np.sqrt(r[want_k] * r[want_k - 1])) if want_k < max_it else 0.5 * r[max_it - 1]
    c = Case(e, 32, arcs, nodes, None, (10,), 'tanh', None, False, 5, max_it, thr, gain=1.2, s0=s0)
    assert c.oracle()['k'] == want_k
    on, off = c.step(True), c.step(False)
    assert on['k'] == want_k
    same(on, off)


@pytest.mark.parametrize('max_it', [1, 7])
def test_batch_normalization_exhausts_max_iter(e, max_it):
    """Training-mode BatchNormalization renormalises the state in every body: the relative change stays far above the threshold and the loop
    runs max_iter bodies - in the oracle and in both forms."""
    rng = np.random.default_rng(41)
    c = Case(e, 42, *_graph(rng, 90), (10,), 'tanh', None, True, 5, max_it, 0.01, gain=0.4)
    assert c.oracle()['k'] == max_it
    on, off = c.step(True), c.step(False)
    assert on['k'] == max_it and on['bn_batch_state'].shape[0] == max_it
    same(on, off)


@pytest.mark.parametrize('graph_based,bn', [(False, True), (True, False)])
def test_persistent_form_matches_the_oracle(e, graph_based, bn):
    """Tolerances of tests/test_gpu_train.py::test_train_step_matches_oracle for the same quantities."""
    rng = np.random.default_rng(51)
    n = 300
    c = Case(e, 52, *_graph(rng, n, (120, 100, 80) if graph_based else None), (16,), 'tanh', None, bn, 6, 5, 0.0, rows_masked=rng.random(n) < 0.8)
    ref, res = c.oracle(), c.step(True)
    assert res['k'] == ref['k'] == 5
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for got, want in list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])):
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))
    if bn:
        mov = [np.asarray(v, np.float64).copy() for v in c.st['weights'][-2:]]
        for it in range(5):
            mov[0] = mov[0] * 0.99 + res['bn_batch_state'][it, 0] * 0.01
            mov[1] = mov[1] * 0.99 + res['bn_batch_state'][it, 1] * 0.01
        np.testing.assert_allclose(mov[0], ref['moving_state'][0], atol=1e-5)
        np.testing.assert_allclose(mov[1], ref['moving_state'][1], atol=1e-5)


def test_two_persistent_runs_are_bit_equal(e):
    rng = np.random.default_rng(61)
    c = Case(e, 62, *_graph(rng, 200), (32, 8), 'selu', None, True, 0, 4, 0.0)
    same(c.step(True), c.step(True))


def test_train_evaluate_train(e):
    """A MUTAG-sized graph-based loop: training step, two inference runs (the second folds the graph readout into its persistent launch),
    training step again - the second step equals one that never saw the inference runs (no update in between: the first)."""
    arcs, nodes, sizes = _mutag_batch()
    c = Case(e, 71, arcs, nodes, sizes, (16,), 'tanh', None, True, 5, 4, 0.0, gain=0.7)
    first = c.step(True)
    assert c.loop.set_persistent(True)
    for _ in range(2):
        c.loop.run()
        folded = c.loop.readout(*c.ng_csr)
    assert np.isfinite(folded).all()
    second = c.step(True)
    assert not np.allclose(c.loop.readout(*c.ng_csr), folded, atol=1e-4)          # the training-mode outputs, not the inference run's host copy
    same(first, second)
    same(second, c.step(False))


def _mutag_models(e, persistent, seen):
    from GNN import losses, optimizers
    from GNN.GNN import GNNgraphBased
    from GNN.MLP import MLP, set_seed

    def model(n_in, n_state, layer=0):
        set_seed(layer)
        st = MLP(n_in, [16, n_state], 'selu', 'glorot_normal', 'zeros')
        ou = MLP(n_state, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
        m = GNNgraphBased(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.01), loss_function=losses.categorical_crossentropy, loss_arguments=None,
                          state_vect_dim=0, max_iteration=4, threshold=0.001, addressed_problem='c')
        inner = m._device_loop

        def device_loop(dev_graph):                     # the model's Python is unchanged: the form is set on the loops it creates
            loop = inner(dev_graph)
            loop.set_train_persistent(persistent)
            seen.append(loop)
            return loop

        m._device_loop = device_loop
        return m

    return model


def _mutag_batches():
    import load_MUTAG
    from GNN.graph_class import GraphObject
    load_MUTAG._PACKED = GOLDEN
    graphs = load_MUTAG.load(limit=64)
    return [GraphObject.merge(graphs[i:i + 32], problem_based='g', aggregation_mode='average') for i in (0, 32)]


def test_models_train_the_same_weights_in_both_forms(e):
    """GNNgraphBased.train, two epochs on two MUTAG batches, and one LGNN joint step: get_weights() bit-equal between the forms."""
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    batches = _mutag_batches()
    nl, al = batches[0].nodes.shape[1], batches[0].arcs.shape[1] - 2
    weights, lgnn_weights = {}, {}
    for persistent in (True, False):
        seen = []
        model = _mutag_models(e, persistent, seen)
        gnn = model(al + 2 * nl, nl)
        gnn.train(batches, 2, None, update_freq=1, verbose=0)
        assert seen and all(lp.train_info()['persistent'] == persistent for lp in seen)
        weights[persistent] = gnn.net_state.get_weights() + gnn.net_output.get_weights()
        seen.clear()
        lgnn = LGNN([model(al + 2 * nl, nl, 1), model(al + 2 * (nl + 2), nl + 2, 2)], False, True, optimizers.Adam(0.01), losses.categorical_crossentropy, None, 'c')
        lgnn.train(batches[:1], 1, None, update_freq=1, training_mode='parallel', verbose=0)
        assert seen and all(lp.train_info()['persistent'] == persistent for lp in seen)
        lgnn_weights[persistent] = [w for g_ in lgnn.gnns for w in g_.net_state.get_weights() + g_.net_output.get_weights()]
    for a, b in list(zip(weights[True], weights[False])) + list(zip(lgnn_weights[True], lgnn_weights[False])):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_ineligible_loops_take_the_launches_of_today(e):
    rng = np.random.default_rng(81)
    # 4,096 rows: the matrix-core forms, never the persistent launch
    c = Case(e, 82, *_graph(rng, 4096), (16,), 'tanh', None, True, 4, 2, 0.0)
    a, b = c.step(True, must_take=False), c.step(False)
    assert not c.loop.set_train_persistent(True) and not a['info']['persistent'] and a['info']['workgroups'] == 0
    same(a, b)
    # Dropout in net_state: the loop as such is eligible (no rates known yet), the forward with the rates is not
    c = Case(e, 83, *_graph(rng, 100), (16,), 'tanh', None, True, 4, 2, 0.0)
    for rates in ([0.2, 0, 0], [0, 0.2, 0], [0, 0, 0.2]):
        a, b = c.step(True, must_take=False, dropout_state=rates), c.step(False, dropout_state=rates)
        assert c.loop.set_train_persistent(True) and not a['info']['persistent']
        same(a, b)
    assert c.step(True)['info']['persistent']
    # a sharded loopback loop: no persistent training forward, and training on it is refused as it is today
    comms = e.Comm.loopback(2)
    g = c.g
    arc_lab = np.asarray(g['arcs'], np.float32)[:, 2:][g['arcT'][1]]
    rb, nr, ip, src, w, aw, al_ = e.shard_csr(100, 1, 2, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_lab)
    shard = e.Graph(100, ip, src, w, aw, al_, g['nodes'], np.ones(nr, np.uint8), row_begin=rb)
    loop = e.Loop(shard, c.mst, c.mou, 4, 2, 0.0, comms[1])
    assert not loop.set_train_persistent(True)
    with pytest.raises(ValueError, match='one process per rank'):
        loop.train_forward(c.mst, c.mou, None)
    assert not loop.train_info()['persistent'] and loop.train_info()['timeouts'] == 0
