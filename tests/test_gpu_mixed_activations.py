"""A net_state whose LAST layer has an activation of its own (['selu', 'selu', 'tanh'], ['relu', 'sigmoid'], ['tanh', 'linear'], ... - the
reference's MLP takes one activation per Dense layer, MLP.py:18, :33) on the three fast inference paths: the fused iteration kernel in both
arithmetic modes, and the persistent small-graph loop on 16- and 32-node tiles.  The kernels apply the hidden activation where a deeper
layer consumes the previous accumulators and the last one only in the final epilogue, which for such a net switches (wave-uniformly) over
the activation named in the kernel arguments.

Bar, as for nets with one activation (tests/test_gpu_parity.py): impl 1, impl 0 and the persistent launch are BIT-IDENTICAL to the C oracle
(k, state, output); impl 2 has the same k and max |state - oracle| < 2e-6 max(1, max |oracle state|) in both piece formats.  Every case
was rehearsed on the NumPy oracle: it converges, float32 and float64 agree on k, and they differ by at most 0.22 of that bound.

A case draws everything from ONE generator in the order graph, net_state, net_output, initial state (_case)."""
import functools
import itertools

import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

ACTS = ['linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid']
PAIRS = [(i, a, b) for i, (a, b) in enumerate(itertools.product(ACTS, ACTS)) if a != b]


def _engine():
    from GNN import _engine
    return _engine


def _case(rng, n, d, nl, al, hidden, act, last, gain):
    arcs = random_arcs(rng, n, 3 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    ds, nlc = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nlc), list(hidden) + [ds], activation=act, out_activation=last, bn_random=True, gain=gain)
    ou = make_mlp(rng, ds + nlc, [2], 'softmax', bn_random=True)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d > 0 else None
    return g, st, ou, s0


@functools.lru_cache(maxsize=None)
def _seeded(seed, n, d, nl, al, hidden, act, last, gain, acts=None):
    """The case of a seed, built once and shared by the tests that run it; acts: the whole activation list of net_state when it is not
    (hidden..., last)."""
    g, st, ou, s0 = _case(np.random.default_rng(seed), n, d, nl, al, hidden, act, last, gain)
    if acts is not None: st['activations'] = list(acts)
    return g, st, ou, s0


@functools.lru_cache(maxsize=None)
def _oracle(key, thr=0.01, max_it=30):
    g, st, ou, s0 = _seeded(*key)
    return corc.loop_node(g, st, ou, key[2], max_it, thr, s0)


def _device(e, key):
    g, st, ou, s0 = _seeded(*key)
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    graph = e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'],
                    np.logical_and(g['set_mask'], g['output_mask']))
    return graph, e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True), s0


def _bound(sc):
    return 2e-6 * max(1.0, float(np.max(np.abs(sc))))


def _check_split(loop, kc, sc, what):
    """impl 2 in both piece formats: the oracle's k, states within the bound"""
    for pieces in (2, 3):
        assert loop.set_pieces(pieces) == pieces
        assert loop.set_impl(2) == 2, what
        k = loop.run()
        s = loop.state()
        err = float(np.max(np.abs(s - sc)))
        print(f'{what} pieces {pieces}: k {k} (oracle {kc}), max |state - oracle| {err:.3e}, bound {_bound(sc):.3e}')
        assert k == kc and err < _bound(sc), (what, pieces, k, kc, err, int(np.isnan(s).sum()))
    loop.set_pieces(2)


def _check_bodies(e, key, what, fused=True):
    """One launch per body: impl 1 and impl 0 bit-identical to the C oracle, impl 2 within the bound.  Returns the open loop (impl 2)."""
    kc, sc, oc = _oracle(key)
    graph, mst, mou, s0 = _device(e, key)
    loop = e.Loop(graph, mst, mou, key[2], 30, 0.01)
    assert loop.set_persistent(False) is False
    assert loop.set_impl(1) == (1 if fused else 0), what        # (the parent commit answers 0 for a net whose last activation differs)
    if s0 is not None: loop.set_state0(s0)
    k = loop.run()
    assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), (what, 'impl 1', k, kc)
    assert loop.set_impl(0) == 0
    k = loop.run()
    assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), (what, 'impl 0', k, kc)
    if fused: _check_split(loop, kc, sc, what)
    return loop


def _check_persistent(e, key, what, gates=((0.01, 30),), also_bodies=False):
    """The persistent launch: both impls (exact arithmetic in either) bit-identical to the C oracle, twice on one handle"""
    graph, mst, mou, s0 = _device(e, key)
    for thr, max_it in gates:
        kc, sc, oc = _oracle(key, thr, max_it)
        for impl in (1, 2):
            loop = e.Loop(graph, mst, mou, key[2], max_it, thr)
            assert loop.set_impl(impl) == impl, what
            assert loop.set_persistent(True) is True, what
            if s0 is not None: loop.set_state0(s0)
            for _ in range(2):
                k = loop.run()
                assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), (what, thr, max_it, impl, k, kc)
            if also_bodies and impl == 1:
                assert loop.set_persistent(False) is False
                k = loop.run()
                assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), (what, 'one launch per body')
            loop.close()
    graph.close()


# ---- A: every ordered pair of two different activations at the smallest generic shape ---------------------------------------------------
def _key_a(i, a, b):
    return (9000 + i, 333, 8, 3, 2, (16,), a, b, 0.5)


@pytest.mark.parametrize('i,a,b', PAIRS, ids=[f'{a}-{b}' for _, a, b in PAIRS])
def test_every_pair_one_launch_per_body(i, a, b):
    e = _engine()
    assert 3 <= _oracle(_key_a(i, a, b))[0] <= 9
    _check_bodies(e, _key_a(i, a, b), f'({a}, {b})').close()


@pytest.mark.parametrize('i,a,b', PAIRS, ids=[f'{a}-{b}' for _, a, b in PAIRS])
def test_every_pair_persistent_launch(i, a, b):
    """333 nodes: 21 tiles of 16 nodes (k_small16; the launch takes 16-node tiles up to 4,096 nodes), the last one partial; the gates leave
    at the oracle's body, after exactly seven bodies, and before the first."""
    _check_persistent(_engine(), _key_a(i, a, b), f'({a}, {b})', gates=((0.01, 30), (0.0, 7), (0.01, 0)))


# ---- B: one case per tile pair and kernel family ------------------------------------------------------------------------------------------
CASES_B = {   # seed: (n, d, nl, al, hidden, act, last, gain), k of the oracle
    9100: ((4113, 64, 3, 1, (128, 128), 'selu', 'tanh', 0.5), 5),       # full-tile kernel, 129 tiles (last partial), folded SELU -> tanh epilogue
    9101: ((4113, 64, 3, 1, (128,), 'relu', 'sigmoid', 0.5), 3),        # two layers, tiles (4, 2)
    9104: ((333, 40, 3, 2, (48,), 'elu', 'sigmoid', 0.5), 3),           # tiles (2, 2)
    9105: ((333, 68, 3, 2, (96,), 'tanh', 'relu', 0.5), 4),             # tiles (4, 4), generic gather
    9102: ((970, 0, 14, 3, (32, 32), 'selu', 'tanh', 0.6), 6),          # MUTAG shape: persistent, 16-node tiles, three layers
    9103: ((5000, 20, 2, 1, (16,), 'tanh', 'linear', 0.6), 5),          # persistent, 32-node tiles, 128-byte exchange rows
}


def _key_b(seed):
    return (seed,) + CASES_B[seed][0]


@pytest.mark.parametrize('seed', sorted(CASES_B))
def test_tile_pairs_and_kernel_families(seed):
    e = _engine()
    key, k_expected = _key_b(seed), CASES_B[seed][1]
    kc, sc, oc = _oracle(key)
    assert kc == k_expected
    f = e.fused_net_form(_dims(key), _seeded(*key)[1]['activations'], key[3] if key[2] else 0)
    assert f['covered'] and f['mixed'] and f['hidden'] == key[6] and f['last'] == key[7]
    loop = _check_bodies(e, key, f'seed {seed}')
    if seed == 9100:
        # in the wave pair's size range (129 tiles <= 4 x CUs), but the pair is for nets with one activation: one wave per tile whatever is asked
        assert (f['NT'], f['NTL']) == (4, 2)
        assert loop.set_tile_form(0) == 1 and loop.set_tile_form(2) == 1 and loop.set_tile_form(0) == 1
        for form, used in ((1, 1), (0, 2)):
            assert loop.set_gather_form(form) == used
            assert loop.set_impl(1) == 1
            k = loop.run()
            assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), ('gather form', form)
            _check_split(loop, kc, sc, f'seed {seed}, gather form {form}')
    loop.close()
    if seed in (9102, 9103):
        _check_persistent(e, key, f'seed {seed}', also_bodies=True)


def _dims(key):
    _, n, d, nl, al, hidden = key[:6]
    ds, nlc = (d if d else nl), (nl if d else 0)
    return [al + 2 * (ds + nlc)] + list(hidden) + [ds]


# ---- C: two different hidden activations still fall back, with the same bits ------------------------------------------------------------------
def test_two_hidden_activations_fall_back_to_the_per_op_kernels():
    e = _engine()
    key = (9200, 333, 8, 3, 2, (16, 16), 'tanh', 'tanh', 0.5, ('relu', 'tanh', 'tanh'))
    assert not e.fused_net_form(_dims(key), ['relu', 'tanh', 'tanh'], 3)['covered']
    loop = _check_bodies(e, key, "('relu', 'tanh', 'tanh')", fused=False)
    assert loop.set_impl(2) == 0 and loop.set_persistent(True) is False and loop.set_tile_form(0) == 0
    loop.close()


# ---- D: fold boundaries of the split arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,hidden,act,last,k_expected', [(9106, (128,), 'tanh', 'selu', 7), (9107, (128, 128), 'selu', 'linear', 5)])
def test_fold_boundaries_of_the_split_arithmetic(seed, hidden, act, last, k_expected):
    """('tanh', 'selu'): nothing is folded and SELU is the epilogue's activation; ('selu', 'selu', 'linear'): two folded layers feed a linear
    epilogue.  The default path as a user gets it - gate and range words readable, the oracle's k - then impl 2 in both piece formats.
    Rehearsed on the C oracles (float32 / float64): k 7 and 5 in both, states 0.28 and 0.19 of the bound apart."""
    e = _engine()
    key = (seed, 4113, 64, 3, 1, hidden, act, last, 0.5)
    kc, sc, oc = _oracle(key)
    assert kc == k_expected
    graph, mst, mou, s0 = _device(e, key)
    loop = e.Loop(graph, mst, mou, 64, 30, 0.01)
    loop.set_state0(s0)
    k = loop.run()                                              # nothing set: the default path
    (gate_rerun, gate_total), (range_rerun, range_total) = loop.gate_info(), loop.range_info()
    assert k == kc and gate_total >= int(gate_rerun) and range_total >= int(range_rerun)
    assert np.max(np.abs(loop.state() - sc)) < _bound(sc)
    _check_split(loop, kc, sc, f'({act}, .., {last})')
    loop.close()
    graph.close()


# ---- E: sharded ------------------------------------------------------------------------------------------------------------------------------------
def test_sharded_rows_match_the_unsharded_run():
    """Two ranks of a loopback group (row all-gather between the bodies), the two-layer ('relu', 'sigmoid') net at n = 1000: owned rows and
    outputs bit-equal to the unsharded run on impl 1 (and so to the C oracle)."""
    e = _engine()
    key = (9101, 1000) + CASES_B[9101][0][1:]
    g, st, ou, s0 = _seeded(*key)
    kc, sc, oc = _oracle(key)
    graph, mst, mou, _ = _device(e, key)
    whole = e.Loop(graph, mst, mou, 64, 30, 0.01)
    assert whole.set_impl(1) == 1
    whole.set_state0(s0)
    ku, su, ou_ = whole.run(), whole.state(), whole.output()
    assert ku == kc and np.array_equal(su, sc) and np.array_equal(ou_, oc)
    n, world = 1000, 2
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    mask = np.logical_and(g['set_mask'], g['output_mask'])
    comms, loops = e.Comm.loopback(world), []
    for r in range(world):
        rb, nr, ip, src, w, aw, al_ = e.shard_csr(n, r, world, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]])
        lp = e.Loop(e.Graph(n, ip, src, w, aw, al_, g['nodes'], mask[rb:rb + nr], row_begin=rb), mst, mou, 64, 30, 0.01, comms[r])
        assert lp.set_impl(1) == 1
        lp.set_state0(s0[rb:rb + nr])
        loops.append(lp)
    k = e.Loop.run_group(loops)
    assert k == ku
    assert np.array_equal(np.concatenate([lp.state() for lp in loops]), su) and np.array_equal(np.concatenate([lp.output() for lp in loops]), ou_)
    for lp in loops: lp.close()
    for c in comms: c.close()


# ---- F: the Python surface --------------------------------------------------------------------------------------------------------------------------
def test_mlp_with_a_list_of_activations_takes_the_fused_path():
    from GNN import GNN_utils as utils, losses
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    from GNN.graph_class import GraphTensor
    np.random.seed(9300)
    go = utils.randomGraph(60, 3, 1, 2, 0.2)
    gt = GraphTensor.fromGraphObject(go)
    rng = np.random.default_rng(9300)
    d = 8
    st = make_mlp(rng, 1 + 2 * (d + 3), [16, d], activation='selu', out_activation='tanh', gain=0.5)
    ou = make_mlp(rng, d + 3, [2], 'softmax')

    def build(net):
        w = net['weights']
        m = MLP(w[0].shape[0], [w[2 * i].shape[1] for i in range(len(net['activations']))], net['activations'], 'zeros', 'zeros', batch_normalization=True)
        m.set_weights(w)
        return m
    gnn = GNNnodeBased(build(st), build(ou), None, losses.categorical_crossentropy, None, d, 20, 0.01, 'c')
    gnn.impl = 1
    s0 = (0.1 * rng.standard_normal((60, d))).astype(np.float32)
    k, s, o = gnn.Loop(gt, state0=s0)
    g = orc.make_graph_dict(np.asarray(go.arcs, np.float32), np.asarray(go.nodes, np.float32), 'average')
    kc, sc, oc = corc.loop_node(g, st, ou, d, 20, 0.01, s0)
    assert k == kc and np.array_equal(s, sc) and np.array_equal(o, oc)
    k64, s64, o64 = orc.loop_node(g, st, ou, d, 20, 0.01, s0, np.float64)
    assert k == k64 and np.max(np.abs(s - s64)) < 1e-5 and np.max(np.abs(o - o64)) < 1e-5
    assert gnn._device_loop(gt.device_graph(gnn.device)).set_impl(1) == 1       # the model's own device loop: on the fused path
    gnn.impl = 2
    k2, s2, _ = gnn.Loop(gt, state0=s0)
    assert k2 == kc and np.max(np.abs(s2 - sc)) < _bound(sc)
