"""Recomputation of the bodies' activations (gnn_loop_set_train_recompute) against the step it must not change.

The yardstick in every test is the same step with the mode OFF on the same loop inputs, and nothing is compared to a tolerance: the replayed
body runs the first pass's kernels on the first pass's inputs in a fixed order, so loss, k, every gradient, the BatchNormalization statistics,
d_nodes and d_arc_labels must be np.array_equal.  Every comparison first asserts that two runs with the mode off agree bit for bit, so that
a failure is not blamed on the wrong side.  Inputs come from seeds through tests/util.py and tests/train_graph_cases.py (directed, unsorted
arc lists); they are built once per spec and never modified.

Shapes (the smallest that reach each forward / backward form):
  (a) 37 rows, 7 -> 8 -> 3: k_mlp_fwd builds the concat itself (7 -> 8 -> 2 where state_vect_dim > 0: 7 = 1 + 2 (2 + 1))
  (b) 83 rows, a Dropout between the layers: the per-layer kernels
  (c) 4,113 rows, one wide layer: the per-layer matrix-core products
  (d) 4,113 rows (128 full 32-row tiles and 17 rows), 135 -> 128 -> 128 -> 64: the three-layer chain; the first pass must launch the
      cache-less chain and the backward pass must replay k bodies"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import train_graph_cases as G
from oracle import gnn_oracle as orc
from util import make_mlp

pytestmark = pytest.mark.gpu

T = 2
ADAM = (1, [0.01, 0.9, 0.999, 1e-7])      # kind and hyper of gnn_loop_arm_optimizer

# d: state_vect_dim; rates: Dropout rates of net_state [layers + 1] (None: none); inject: the masks are injected (else the engine's generator);
# kind: 'node' / 'graph' / 'edge'; far: initial state rows of norm 100 (the first body moves every node, the second hardly: k = 1);
# bn_out: BatchNormalization behind net_output's softmax (off in most specs: its two columns are then mirror images, one of them negative on
# nearly every row, and the clipped crossentropy passes no gradient through such a row)
Spec = namedtuple('Spec', 'n d nl al layers act last_act bn rates inject kind max_it thr gain seed far bn_out',
                  defaults=(None, True, None, False, 'node', 3, 0.0, 0.5, 1, False, False))

A = Spec(37, 0, 3, 1, (8, 3), 'tanh')
A_D = Spec(37, 2, 1, 1, (8, 2), 'tanh')
B = Spec(83, 4, 3, 2, (7, 4), 'tanh', rates=(0.0, 0.25, 0.0))
C_ = Spec(4113, 32, 3, 1, (32,), 'tanh')
D = Spec(4113, 64, 3, 1, (128, 128, 64), 'selu')
D_0 = Spec(4113, 0, 40, 1, (72, 96, 40), 'tanh')        # labels as state: concat 81, a last layer of 40 (the backward pass runs layer by layer)


def ds_of(s): return s.d if s.d else s.nl
def nlc_of(s): return s.nl if s.d else 0
def in_s_of(s): return s.al + 2 * (ds_of(s) + nlc_of(s))


@functools.lru_cache(maxsize=None)
def inputs(s):
    """Everything a loop of this spec is created from (NumPy only)"""
    rng = np.random.default_rng(s.seed)
    n, ds, nlc, in_s, edge = s.n, ds_of(s), nlc_of(s), in_s_of(s), s.kind == 'edge'
    arcs = G.directed_graph(3000 + s.seed, n, degrees=True, al=s.al)
    nodes = (2 * rng.random((n, s.nl)) - 1).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if s.d else None
    if s.far:
        rows = rng.standard_normal((n, ds))
        rows = (100.0 * rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        if s.d: s0 = rows
        else: nodes = rows
    ng = G.node_graph(rng, n) if s.kind == 'graph' else None
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    st = make_mlp(rng, in_s, list(s.layers), s.act, batch_normalization=s.bn, out_activation=s.last_act, gain=s.gain, bn_random=True)
    ou = make_mlp(rng, 2 * (ds + nlc) + s.al if edge else ds + nlc, [T], 'tanh', out_activation='softmax', batch_normalization=s.bn_out, bn_random=True)
    if edge: mask = G.edge_mask(arcs, n, s.seed)[0]
    elif s.kind == 'graph': mask = np.ones(n, bool)
    else: mask = rng.random(n) < 0.8
    n_t = ng.shape[1] if ng is not None else int(mask.sum())
    targets = np.eye(T)[rng.integers(0, T, n_t)].astype(np.float32)
    weights = rng.uniform(0.5, 1.5, n_t).astype(np.float32)
    rates = list(s.rates) if s.rates else [0.0] * (len(s.layers) + 1)
    widths = [in_s] + list(s.layers)
    masks = None
    if s.inject:        # per body: the Dropout positions in order, [N, width] keep bytes each
        masks = np.concatenate([(rng.random((n, widths[p])) >= abs(rates[p])).astype(np.uint8).ravel()
                                for _ in range(max(s.max_it, 1)) for p in range(len(rates)) if rates[p] != 0.0])
    d_out = rng.standard_normal((int(mask.sum()), T)).astype(np.float32)
    return dict(arcs=arcs, g=g, st=st, ou=ou, mask=mask, s0=s0, targets=targets, weights=weights, rates=rates, masks=masks, d_out=d_out,
                ng_csr=G.nodegraph_csr(ng) if ng is not None else None)


class Dev:
    """A fresh graph, nets and loop of a spec on the device"""

    def __init__(self, e, s, max_it=None, thr=None):
        self.s, self.i = s, inputs(s)
        i, g, n, edge = self.i, self.i['g'], s.n, s.kind == 'edge'
        labels = np.asarray(g['arcs'])[:, 2:]
        self.graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], labels[g['arcT'][1]], g['nodes'],
                             np.ones(n, bool) if edge else i['mask'])
        self.mst, self.mou = e.Mlp(i['st']['weights'], i['st']['activations'], s.bn), e.Mlp(i['ou']['weights'], i['ou']['activations'], s.bn_out)
        self.loop = e.Loop(self.graph, self.mst, self.mou, s.d, s.max_it if max_it is None else max_it, s.thr if thr is None else thr)
        if edge:
            self.graph.set_arc_order(g['arcT'][1], labels)
            self.loop.set_edge_readout(np.repeat(np.arange(n, dtype=np.int32), np.diff(g['adjT'][0])), labels, i['mask'])
        if s.d: self.loop.set_state0(i['s0'])

    def kw(self):
        return dict(dropout_state=self.i['rates'], dropout_output=[0.0, 0.0], masks_state=self.i['masks'], seed=11)

    def step(self, recompute, armed=False, cacheless=True):
        used = self.loop.set_train_recompute(recompute, cacheless=cacheless)
        assert used == recompute
        if armed: self.loop.arm_optimizer(ADAM[0], ADAM[1], True)
        res = self.loop.train_step(self.mst, self.mou, None, self.i['targets'], self.i['weights'], 0, self.i['ng_csr'], **self.kw())
        res['info'] = self.loop.train_recompute_info()
        assert res['info']['state_only'] == recompute and res['info']['replayed'] == (int(res['k']) if recompute else 0), res['info']
        return res

    def forward_backward(self, recompute):
        assert self.loop.set_train_recompute(recompute) == recompute
        k, out = self.loop.train_forward(self.mst, self.mou, None, **self.kw())
        state = self.loop.state()
        res = self.loop.train_backward(self.i['d_out'], want_d_nodes=True, want_d_arcs=self.s.kind == 'edge')
        res.update(k=k, out=out, state=state, info=self.loop.train_recompute_info())
        assert res['info']['state_only'] == recompute and res['info']['replayed'] == (int(k) if recompute else 0), res['info']
        return res

    def weights(self):
        return self.mst.get_weights() + self.mou.get_weights()

    def close(self):
        self.loop.close(); self.graph.close()


def same(a, b, tag=''):
    for key in ('k', 'loss', 'state', 'out', 'bn_batch_state', 'bn_batch_output', 'd_nodes', 'd_arcs'):
        if key in a or key in b:
            if a.get(key) is None and b.get(key) is None: continue
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, key)
    assert len(a['grads_state']) == len(b['grads_state']) and len(a['grads_output']) == len(b['grads_output'])
    for idx, (x, y) in enumerate(zip(a['grads_state'] + a['grads_output'], b['grads_state'] + b['grads_output'])):
        assert x.shape == y.shape and np.array_equal(x, y), (tag, 'gradient', idx)
    assert all(np.isfinite(x).all() for x in a['grads_state'] + a['grads_output']), tag


def check_bit_identity(e, s, want_k=None, want_chain=None, label_gradients=True):
    """step and forward + backward of one spec: off == off, then on == off - the mode switched on a used loop and taken by a fresh one"""
    dev = Dev(e, s)
    off, off2 = dev.step(False), dev.step(False)
    same(off, off2, 'off / off')
    if want_k is not None: assert off['k'] == want_k, off['k']
    # (not a comparison of zeros: the loss reaches every trainable array; without a body net_state has no gradient)
    for idx, x in enumerate(off['grads_output'] + (off['grads_state'] if off['k'] > 0 else [])): assert np.abs(x).max() > 0, ('zero gradient', idx)
    on = dev.step(True)
    same(on, off, 'on / off')
    fresh = Dev(e, s)
    on_fresh = fresh.step(True)
    same(on_fresh, off, 'on (fresh loop) / off')
    if want_chain is not None:
        assert on['info']['cacheless_chain'] == want_chain and on_fresh['info']['cacheless_chain'] == want_chain, (on['info'], on_fresh['info'])
        scratch = dev.step(True, cacheless=False)            # the caching kernels on rewound scratch: the other first pass
        assert scratch['info']['cacheless_chain'] == 0
        same(scratch, off, 'on with the caching kernels / off')
    if label_gradients:
        fb_off, fb_off2 = dev.forward_backward(False), dev.forward_backward(False)
        same(fb_off, fb_off2, 'forward + backward: off / off')
        fb_on = fresh.forward_backward(True)
        same(fb_on, fb_off, 'forward + backward: on / off')
        assert fb_on['d_nodes'] is not None and (fb_on['d_arcs'] is not None) == (s.kind == 'edge')
        if off['k'] > 0 or s.d == 0: assert np.abs(fb_on['d_nodes']).max() > 0
    after = dev.step(False)                                  # and off again behind it
    same(after, off, 'off behind on / off')
    dev.close(); fresh.close()
    return off


@pytest.fixture(scope='module')
def e():
    from GNN import _engine
    return _engine


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------------------------------
FORMS = [pytest.param(A, 0, id='a-mlp_fwd-builds-input'), pytest.param(B, 0, id='b-per-layer-dropout-between'),
         pytest.param(C_, 0, id='c-wide-layer'), pytest.param(D, 1, id='d-chain3')]


@pytest.mark.parametrize('s,chain', FORMS)
def test_bit_identity_per_form(e, s, chain):
    off = check_bit_identity(e, s, want_k=s.max_it, want_chain=chain)
    assert off['bn_batch_state'].shape[0] == s.max_it


@pytest.mark.parametrize('s,chain', FORMS)
def test_form_is_the_one_the_shape_is_there_for(e, s, chain):
    """The forward form of every layer as gnn_train_forms decides it from the shapes alone (host code), so that the table above tests what it says"""
    dims, acts = [in_s_of(s)] + list(s.layers), [s.act] * len(s.layers)
    f = e.train_forms(dims, acts, rates=list(s.rates) if s.rates else None, n_rows=s.n, producer_dropout=True)
    want = {A: 'mlp_fwd', B: 'per_op', C_: 'wide', D: 'chain3'}[s]
    assert f['forward'] == [want] * len(s.layers) and f['build_input'] == (s is A), f


VARIANTS = [
    pytest.param(A._replace(bn=False), id='a-no-bn'),
    pytest.param(D._replace(bn=False), id='d-no-bn'),
    pytest.param(A._replace(rates=(0.25, 0.0, 0.0)), id='a-dropout-first-own'),
    pytest.param(A._replace(rates=(0.25, 0.0, 0.0), inject=True), id='a-dropout-first-injected'),
    pytest.param(D._replace(rates=(0.25, 0.0, 0.0, 0.0)), id='d-dropout-first-own'),
    pytest.param(D._replace(rates=(0.25, 0.0, 0.0, 0.0), inject=True), id='d-dropout-first-injected'),
    pytest.param(A._replace(rates=(0.0, 0.25, 0.0)), id='a-dropout-between'),
    pytest.param(D._replace(rates=(0.0, 0.0, 0.25, 0.0)), id='d-dropout-between'),
    pytest.param(A._replace(rates=(0.0, 0.0, 0.25)), id='a-dropout-before-bn'),
    pytest.param(D._replace(rates=(0.0, 0.0, 0.0, 0.25)), id='d-dropout-before-bn'),
    pytest.param(A._replace(rates=(0.0, 0.0, -0.25), bn=False), id='a-alpha-dropout-last-no-bn'),
    pytest.param(A._replace(bn_out=True), id='a-bn-behind-net_output'),
    pytest.param(D._replace(bn_out=True), id='d-bn-behind-net_output'),
    pytest.param(A_D, id='a-state-dim-2'),
    pytest.param(D_0, id='d-labels-as-state'),
    pytest.param(A._replace(kind='graph'), id='a-graph'),
    pytest.param(D._replace(kind='graph'), id='d-graph'),
    pytest.param(A._replace(kind='edge', al=1), id='a-edge'),
    pytest.param(D._replace(kind='edge'), id='d-edge'),
]


@pytest.mark.parametrize('s', VARIANTS)
def test_bit_identity_variants(e, s):
    check_bit_identity(e, s, want_k=s.max_it)


def _threshold_for(e, s, accept):
    """A threshold at which the step with the mode OFF stops where `accept` wants it: the first of a geometric grid from 2 down in steps of 10 % (the net is a
    contraction, the relative change falls from body to body)"""
    seen = []
    for thr in 2.0 * 0.9 ** np.arange(80):
        dev = Dev(e, s, thr=float(thr))
        k = int(dev.step(False)['k'])
        dev.close()
        if accept(k): return float(thr), k
        seen.append(k)
    raise AssertionError(f'no threshold of the grid stops the loop where the test wants it: k = {seen}')


STOPS = [pytest.param(A_D._replace(bn=False, max_it=12, gain=0.8), id='a'), pytest.param(D._replace(bn=False, act='tanh', max_it=12, gain=0.8), id='d')]


@pytest.mark.parametrize('s', STOPS)
def test_stops_inside_the_first_chunk(e, s):
    thr, k = _threshold_for(e, s, lambda k: 1 < k < 5)
    check_bit_identity(e, s._replace(thr=thr), want_k=k, label_gradients=False)


@pytest.mark.parametrize('s', STOPS)
def test_max_iter_spans_more_than_one_chunk(e, s):
    """threshold 0: all 12 bodies run - a fresh loop looks at the gates behind 5, 10 and 12 of them, a used one (k_hint) behind all 12"""
    check_bit_identity(e, s, want_k=12, label_gradients=False)


@pytest.mark.parametrize('s', STOPS)
def test_one_body(e, s):
    """State rows of norm 100 and a tanh net: body 0 moves every node by more than 3 times the norm of ones, body 1 by about its own norm"""
    check_bit_identity(e, s._replace(far=True, thr=3.0), want_k=1)


@pytest.mark.parametrize('s', STOPS)
def test_no_body_allowed(e, s):
    check_bit_identity(e, s._replace(max_it=0), want_k=0)


@pytest.mark.parametrize('s', [pytest.param(A, id='a'), pytest.param(D, id='d'), pytest.param(B, id='b')])
def test_three_armed_steps_train_the_same_weights(e, s):
    """Flow: Adam on the device behind each of three steps - both nets' weights and moving statistics afterwards"""
    runs = {}
    for name, recompute in (('off', False), ('off2', False), ('on', True)):
        dev = Dev(e, s)
        losses = [dev.step(recompute, armed=True)['loss'] for _ in range(3)]
        runs[name] = (losses, dev.weights())
        dev.close()
    assert len(set(runs['off'][0])) == 3                     # the weights moved
    for other in ('off2', 'on'):
        assert runs[other][0] == runs['off'][0], other
        for x, y in zip(runs[other][1], runs['off'][1]):
            assert x.shape == y.shape and np.array_equal(x, y), other


# ---- 2. arena -----------------------------------------------------------------------------------------------------------------------------------------
def test_arena_keeps_the_states_and_one_body():
    """A net that does not contract (gain 3) under BatchNormalization runs all 200 bodies.  state = one state table; body = concat, both Dense
    outputs and xhat.  On: at most 200 x 3 state tables (table, gate and statistics slots, allocation granularity) plus 12 bodies (the allowance
    of tests/test_gpu_adjoint.py::test_arena_holds_one_body_whatever_max_iter for one live body and the backward scratch)."""
    from GNN import _engine as e
    n, ds, hidden, max_it = 2000, 16, 32, 200
    s = Spec(n, ds, 3, 1, (hidden, ds), 'tanh', max_it=max_it, thr=1e-3, gain=3.0, seed=81)
    in_s = in_s_of(s)
    state, body = 4 * n * ds, 4 * n * (in_s + hidden + ds + ds)
    used = {}
    for recompute in (True, False):
        dev = Dev(e, s)
        res = dev.step(recompute)
        assert res['k'] == max_it
        used[recompute] = dev.loop.train_arena_bytes()
        dev.close()
    print(f'arena bytes: on {used[True]}, off {used[False]}; state {state}, body {body}')
    assert used[True] <= max_it * 3 * state + 12 * body, (used, state, body)
    assert used[False] >= max_it * body, (used, body)
    assert used[True] < used[False] / 4, used


# ---- 3. interactions ----------------------------------------------------------------------------------------------------------------------------------
def test_fixed_point_mode_ignores_the_setting(e):
    s = A_D._replace(bn=False, max_it=30, thr=1e-3)
    dev = Dev(e, s)
    assert dev.loop.set_gradient_mode('fixed_point') == 1
    kw = dict(dropout_state=dev.i['rates'], dropout_output=[0.0, 0.0], seed=11)
    step = lambda: dev.loop.train_step(dev.mst, dev.mou, None, dev.i['targets'], dev.i['weights'], 0, None, **kw)
    alone, alone2 = step(), step()
    same(alone, alone2, 'fixed point / fixed point')
    assert dev.loop.set_train_recompute(True) is False
    both = step()
    assert dev.loop.train_recompute_info() == dict(state_only=False, replayed=0, cacheless_chain=0)
    same(both, alone, 'fixed point with the mode on / fixed point')
    assert both['adjoint_iterations'] == alone['adjoint_iterations']
    assert dev.loop.set_gradient_mode('unrolled') == 0 and dev.loop.set_train_recompute(True) is True
    dev.close()


def test_persistent_forward_is_not_taken(e):
    """A MUTAG-sized batch (about 570 rows, 16 -> 16 -> 8): the loop would take the persistent training forward, the mode keeps it to launches"""
    s = Spec(570, 8, 3, 2, (16, 8), 'selu', max_it=4, seed=5)
    dev = Dev(e, s)
    assert dev.loop.set_train_persistent(True) is True
    persistent = dev.step(False)
    assert dev.loop.train_info()['persistent']
    on = dev.step(True)
    assert not dev.loop.train_info()['persistent'] and dev.loop.train_info()['workgroups'] == 0
    assert dev.loop.set_train_persistent(False) is False
    off, off2 = dev.step(False), dev.step(False)
    assert not dev.loop.train_info()['persistent']
    same(off, off2, 'off / off')
    same(on, off, 'on with the persistent forward allowed / per-launch step')
    same(persistent, off, 'persistent / per-launch step')
    dev.close()


def test_train_mask_after_a_state_only_forward(e):
    s = A._replace(rates=(0.25, 0.0, 0.0))
    dev = Dev(e, s)
    kw = dict(dev.kw(), dropout_output=[0.25, 0.0])
    dev.loop.set_train_recompute(False)
    dev.loop.train_forward(dev.mst, dev.mou, None, **kw)
    m0, m1 = dev.loop.train_mask(0, 1, 0), dev.loop.train_mask(1, 0, 0)
    assert m0.shape == (s.n, in_s_of(s)) and 0 < m0.mean() < 1
    dev.loop.set_train_recompute(True)
    dev.loop.train_forward(dev.mst, dev.mou, None, **kw)
    with pytest.raises(e.EngineError, match='gnn_loop_set_train_recompute'):
        dev.loop.train_mask(0, 1, 0)
    assert np.array_equal(dev.loop.train_mask(1, 0, 0), m1)
    assert dev.loop.train_forms(0) == dev.loop.train_forms(0) and dev.loop.train_forms(1)
    dev.loop.set_train_recompute(False)
    dev.loop.train_forward(dev.mst, dev.mou, None, **kw)
    assert np.array_equal(dev.loop.train_mask(0, 1, 0), m0)
    dev.close()


def test_default_step_behind_a_recomputing_step_is_a_fresh_loops(e):
    for s in (A, D):
        used, fresh = Dev(e, s), Dev(e, s)
        used.step(True)
        behind, first = used.step(False), fresh.step(False)
        same(behind, first, 'off behind on / off on a fresh loop')
        assert used.loop.train_arena_bytes() == fresh.loop.train_arena_bytes()
        used.close(); fresh.close()


# ---- 4. LGNN ------------------------------------------------------------------------------------------------------------------------------------------
def _sequential(net):
    from GNN.MLP import Sequential, Dense, BatchNormalization
    layers = [Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)) for l in range(len(net['activations']))]
    if net['batch_normalization']: layers.append(BatchNormalization())
    seq = Sequential(layers)
    seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
    return seq


@functools.lru_cache(maxsize=None)
def _lgnn_inputs():
    rng = np.random.default_rng(91)
    n, nl, al, d = G.N_SMALL, 3, 2, 4
    arcs = G.directed_graph(1012, n, degrees=True, al=al)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]                    # (source, destination)-sorted, as GraphObject lists are
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    set_mask = rng.random(n) < 0.8
    targets = np.eye(T)[rng.integers(0, T, n)].astype(np.float32)
    weights = rng.uniform(0.5, 1.5, n).astype(np.float32)
    nets, s0 = [], []
    for i in range(2):
        ins, ls = orc.get_inout_dims('state', nl, al, T, 'n', d, [7], layer=i, get_state=True, get_output=True)
        ino, lo = orc.get_inout_dims('output', nl, al, T, 'n', d, None, layer=i, get_state=True, get_output=True)
        nets.append((make_mlp(rng, ins, ls, 'tanh', gain=0.5, batch_normalization=True, bn_random=True),
                     make_mlp(rng, ino, lo, 'tanh', out_activation='softmax', batch_normalization=False)))
        s0.append((0.1 * rng.standard_normal((n, d))).astype(np.float32))
    return dict(arcs=arcs, nodes=nodes, set_mask=set_mask, targets=targets, weights=weights, nets=nets, s0=s0, d=d)


def _lgnn_step(mode, recompute):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject, GraphTensor
    i = _lgnn_inputs()
    seen = []
    gnns = []
    for st, ou in i['nets']:
        m = GNNnodeBased(net_state=_sequential(st), net_output=_sequential(ou), optimizer=None, loss_function=None, loss_arguments=None,
                         state_vect_dim=i['d'], max_iteration=3, threshold=0.0, addressed_problem='c')
        inner = m._device_loop

        def device_loop(dev_graph, inner=inner):
            loop = inner(dev_graph)
            seen.append(loop)
            return loop

        m._device_loop = device_loop
        gnns.append(m)
    lgnn = LGNN(gnns, True, True, optimizers.SGD(0.0), losses.categorical_crossentropy, None, 'c')
    lgnn.training_mode = mode
    lgnn.set_train_recompute(recompute)
    go = GraphObject(arcs=i['arcs'], nodes=i['nodes'], targets=i['targets'], set_mask=i['set_mask'], sample_weights=i['weights'], problem_based='n',
                     aggregation_mode='average')
    res = lgnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=i['s0'])
    assert len(seen) == 2
    assert list(res['k']) == [3, 3]
    for loop in seen:
        info = loop.train_recompute_info()
        assert info['state_only'] == recompute and info['replayed'] == (3 if recompute else 0), info
    return res


@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_lgnn_joint_step(mode):
    off, off2, on = _lgnn_step(mode, False), _lgnn_step(mode, False), _lgnn_step(mode, True)
    for other, tag in ((off2, 'off / off'), (on, 'on / off')):
        assert np.array_equal(np.asarray(other['loss']), np.asarray(off['loss'])), tag
        assert np.array_equal(np.asarray(other['k']), np.asarray(off['k'])), tag
        for li in range(2):
            assert np.array_equal(other['outs'][li], off['outs'][li]), (tag, li)
            for x, y in zip(other['grads_state'][li] + other['grads_output'][li], off['grads_state'][li] + off['grads_output'][li]):
                assert x.shape == y.shape and np.array_equal(x, y), (tag, li)
    assert np.abs(on['grads_state'][0][0]).max() > 0 and np.abs(on['grads_output'][0][0]).max() > 0
