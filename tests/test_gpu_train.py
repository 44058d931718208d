"""One training step on the device (gnn_loop_train_step) against the float64 training oracle: loss, iteration count,
gradients of every trainable array, BatchNormalization batch statistics.  Tolerance-based (float32, atomically accumulated
weight gradients; BatchNormalization right after a softmax is ill-conditioned): 1e-3 relative to the largest entry of each gradient array."""
import numpy as np
import pytest

from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu


def _by_source_csr(g, n):
    indptr, src, w = g['adjT']
    dst = np.repeat(np.arange(n), np.diff(indptr))
    order = np.lexsort((dst, src))
    sip = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=sip[1:])
    return sip, dst[order].astype(np.int32), np.asarray(w, np.float32)[order]


@pytest.mark.parametrize('d,graph_based,act,loss,alpha', [(8, False, 'tanh', 'categorical_crossentropy', False), (0, False, 'selu', 'categorical_crossentropy', False),
                                                            (5, True, 'sigmoid', 'mean_squared_error', False), (0, True, 'relu', 'categorical_crossentropy', False),
                                                            (8, False, 'selu', 'categorical_crossentropy_from_logits', True)])
def test_train_step_matches_oracle(d, graph_based, act, loss, alpha):
    """alpha: AlphaDropout (negative rates on the C ABI); *_from_logits: loss_kind 2."""
    from GNN import _engine as e
    rng = np.random.default_rng(100 + d)
    n, nl, al, max_it = 500, 3, 2, 6
    arcs = random_arcs(rng, n, 1500, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if graph_based:
        ng = np.zeros((n, 3), np.float32); ng[:200, 0] = 1 / 200; ng[200:350, 1] = 1 / 150; ng[350:, 2] = 1 / 150
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    if not graph_based:
        g['set_mask'] = rng.random(n) < 0.8
    ds, nlc = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nlc), [16, ds], act, gain=0.8, bn_random=True)
    ou = make_mlp(rng, ds + nlc, [9, 2], act, out_activation='softmax', bn_random=True)
    st['dropout'], ou['dropout'] = {0: 0.2}, {0: 0.1, 1: 0.3}
    if alpha: st['alphadropout'] = ou['alphadropout'] = True
    sgn = -1.0 if alpha else 1.0
    kind = {'categorical_crossentropy': 0, 'mean_squared_error': 1, 'categorical_crossentropy_from_logits': 2}[loss]
    mask = g['set_mask'] & g['output_mask']
    m = int(mask.sum())
    in_s = st['weights'][0].shape[0]
    masks_s = [{0: (rng.random((n, in_s)) > 0.2)} for _ in range(max_it)]
    masks_o = {0: rng.random((m, ds + nlc)) > 0.1, 1: rng.random((m, 9)) > 0.3}
    n_t = 3 if graph_based else m
    targets = np.eye(2)[rng.integers(0, 2, n_t)].astype(np.float32)
    weights = rng.uniform(0.5, 1.5, n_t).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
    # threshold 0: the training-mode forward has BatchNormalization batch statistics accumulated with float atomics, whose last
    # bits vary from run to run; a borderline convergence test could then stop one body earlier or later than the float64 oracle.
    # The early stop itself is covered by test_training_forward_stops_at_convergence (no BatchNormalization: deterministic).
    thr = 0.0
    ref = tro.train_step(g, st, ou, d, max_it, thr, s0, masks_s, masks_o, targets, weights, loss=loss, mean=False, graph_based=graph_based)

    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    loop = e.Loop(graph, mst, mou, d, max_it, thr)
    if d:
        loop.set_state0(s0)
    ms = np.concatenate([masks_s[k][0].astype(np.uint8).ravel() for k in range(max_it)])
    mo = np.concatenate([masks_o[0].astype(np.uint8).ravel(), masks_o[1].astype(np.uint8).ravel()])
    ng_csr = None
    if graph_based:
        cols, rows = np.nonzero(ng.T)
        ip = np.zeros(4, np.int32); np.cumsum(np.bincount(cols, minlength=3), out=ip[1:])
        ng_csr = (ip, rows.astype(np.int32), ng[rows, cols])
    res = loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, kind, ng_csr,
                          dropout_state=[sgn * 0.2, 0, 0], dropout_output=[sgn * 0.1, sgn * 0.3, 0], masks_state=ms, masks_output=mo,
                          bn_state=np.concatenate(st['weights'][-4:-2]), bn_output=np.concatenate(ou['weights'][-4:-2]))
    assert res['k'] == ref['k'] and 1 <= res['k'] <= max_it
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for got, want in list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])):
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))
    k = int(res['k'])
    # batch statistics -> the moving averages the caller derives from them
    mov = [np.asarray(v, np.float64).copy() for v in st['weights'][-2:]]
    for it in range(k):
        mov[0] = mov[0] * 0.99 + res['bn_batch_state'][it, 0] * 0.01
        mov[1] = mov[1] * 0.99 + res['bn_batch_state'][it, 1] * 0.01
    np.testing.assert_allclose(mov[0], ref['moving_state'][0], atol=1e-5)
    np.testing.assert_allclose(mov[1], ref['moving_state'][1], atol=1e-5)
    np.testing.assert_allclose(np.asarray(ou['weights'][-2], np.float64) * 0.99 + res['bn_batch_output'][0] * 0.01, ref['moving_output'][0], atol=1e-5)
    # run-to-run determinism: the column reductions and weight gradients add per-chunk partials in a fixed order (no float atomics)
    again = loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, kind, ng_csr,
                            dropout_state=[sgn * 0.2, 0, 0], dropout_output=[sgn * 0.1, sgn * 0.3, 0], masks_state=ms, masks_output=mo,
                            bn_state=np.concatenate(st['weights'][-4:-2]), bn_output=np.concatenate(ou['weights'][-4:-2]))
    assert again['loss'] == res['loss'] and again['k'] == res['k']
    for a_, b_ in zip(again['grads_state'] + again['grads_output'], res['grads_state'] + res['grads_output']):
        assert np.array_equal(a_, b_)
    assert np.array_equal(again['bn_batch_state'], res['bn_batch_state']) and np.array_equal(again['bn_batch_output'], res['bn_batch_output'])
    # engine RNG masks: same call without injected masks must run and give finite numbers (the drawn masks themselves - keep rate,
    # independence, the oracle on them - are tests/test_gpu_dropout_rng.py)
    res2 = loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, kind, ng_csr,
                           dropout_state=[sgn * 0.2, 0, 0], dropout_output=[sgn * 0.1, sgn * 0.3, 0], seed=5,
                           bn_state=np.concatenate(st['weights'][-4:-2]), bn_output=np.concatenate(ou['weights'][-4:-2]))
    assert np.isfinite(res2['loss']) and all(np.isfinite(a).all() for a in res2['grads_state'] + res2['grads_output'])


def test_train_loop_reduces_loss_and_keeps_history():
    """BaseClass.train end to end (reference GNN_BaseClass.py:192-335): Adam on device gradients must fit a learnable
    node-classification task; history bookkeeping, early-stopping restore, graph-based variant, serial LGNN."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(0)
    set_seed(0)
    graphs = []
    for _ in range(6):
        n = 120
        arcs = random_arcs(rng, n, 360, 1)
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        cls = (nodes[:, 0] + 0.5 * nodes[:, 1] > 0).astype(int)          # learnable from the labels
        graphs.append(GraphObject(arcs=arcs, nodes=nodes, targets=np.eye(2)[cls]))
    gTr, gVa = graphs[:4], GraphObject.merge(graphs[4:], problem_based='n', aggregation_mode='average')

    def model(cls_, layer=0):
        st = MLP(1 + 2 * (3 + 2 * (layer > 0)), [8, 3 + 2 * (layer > 0)], 'tanh', 'glorot_normal', 'zeros', dropout_rate=0.1, dropout_pos=0)
        ou = MLP(3 + 2 * (layer > 0), [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
        return cls_(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                    loss_arguments=None, state_vect_dim=0, max_iteration=4, threshold=0.01, addressed_problem='c',
                    extra_metrics={'Acc': lambda yt, yp: float(np.mean(yt == yp))})

    gnn = model(GNNnodeBased)
    before = gnn.test(gVa)
    gnn.train(gTr, 40, gVa, update_freq=5, max_fails=50, verbose=0)
    after = gnn.test(gVa)
    assert after['Loss'] < 0.6 * before['Loss'] and after['Acc'] > 0.85
    h = gnn.history
    assert h['Epoch'] == list(range(0, 40, 5)) and len(h['Loss Tr']) == len(h['Loss Va']) == len(h['Fail']) == 8
    assert h['Best Loss Va'][-1] == min(h['Loss Va']) and h['Loss Tr'][-1] < h['Loss Tr'][0]
    gnn.train(gTr, 5, gVa, update_freq=5, max_fails=50, verbose=0)      # re-entrant: epochs continue (reference :278-279)
    assert gnn.history['Epoch'][-1] == 40
    # graph-based: 2 graphs per batch, targets per graph
    gg = []
    for i in range(8):
        n = 40
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32) + (0.8 if i % 2 else -0.8)
        gg.append(GraphObject(arcs=random_arcs(rng, n, 100, 1), nodes=nodes, targets=np.eye(2)[[i % 2]], problem_based='g'))
    batches = [GraphObject.merge(gg[i:i + 4], problem_based='g', aggregation_mode='average') for i in (0, 4)]
    ggnn = model(GNNgraphBased)
    l0 = ggnn.test(batches)['Loss']
    ggnn.train(batches, 30, None, update_freq=10, verbose=0)
    assert ggnn.test(batches)['Loss'] < 0.7 * l0
    # serial LGNN training (reference LGNN.py:325-340)
    lgnn = LGNN([model(GNNnodeBased, 0), model(GNNnodeBased, 1)], False, True, optimizers.Adam(0.02), losses.categorical_crossentropy, None, 'c')
    lgnn.train(gTr, 10, None, update_freq=5, training_mode='serial', verbose=0)
    assert lgnn.test(gVa)['Loss'] < before['Loss']


@pytest.mark.parametrize('d,graph_based,get_state,get_output,mode,loss', [
    (4, False, True, True, 'parallel', 'mean_squared_error'), (0, False, True, False, 'residual', 'categorical_crossentropy'),
    (3, True, False, True, 'parallel', 'categorical_crossentropy'), (0, True, True, True, 'residual', 'mean_squared_error')])
def test_lgnn_joint_training_step_matches_oracle(d, graph_based, get_state, get_output, mode, loss):
    """LGNN 'parallel' / 'residual' training (reference LGNN.py:201-224, :343-344): gnn_loop_train_forward per layer with the
    device relabelling in between, host loss, gnn_loop_train_backward per layer with the label gradients chained."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased
    from GNN.LGNN import LGNN
    from GNN.MLP import Sequential, Dense, Dropout, BatchNormalization
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(40 + d)
    n, nl, al, t, max_it, L = 300, 3, 2, 2, 3, 3
    arcs = random_arcs(rng, n, 800, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if graph_based:
        ng = np.zeros((n, 2), np.float32); ng[:180, 0] = 1 / 180; ng[180:, 1] = 1 / 120
    set_mask = np.ones(n, bool) if graph_based else rng.random(n) < 0.8
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    g['set_mask'] = set_mask
    m = int(set_mask.sum())
    # GraphObject targets / sample_weights are per output_mask row (all nodes here); set_mask filters them (GNN_BaseClass.py:405-410)
    n_full = 2 if graph_based else n
    targets_full = np.eye(t)[rng.integers(0, t, n_full)].astype(np.float32)
    weights_full = rng.uniform(0.5, 1.5, n_full).astype(np.float32)
    targets, weights = (targets_full, weights_full) if graph_based else (targets_full[set_mask], weights_full[set_mask])

    def sequential(net):
        layers = []
        nd = len(net['activations'])
        for l in range(nd):
            if net['dropout'].get(l): layers.append(Dropout(net['dropout'][l]))
            layers.append(Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)))
        if net['batch_normalization']: layers.append(BatchNormalization())
        seq = Sequential(layers)
        seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
        return seq

    layers, s0, ms, mo, gnns = [], [], [], [], []
    nl_i = nl
    for i in range(L):
        ds, nlc = (d if d else nl_i), (nl_i if d else 0)
        st = make_mlp(rng, al + 2 * (ds + nlc), [10, ds], 'tanh', gain=0.8, bn_random=True)
        if loss == 'categorical_crossentropy':
            ou = make_mlp(rng, ds + nlc, [t], 'tanh', out_activation='softmax')
            ou.update(batch_normalization=False, weights=ou['weights'][:2])
        else:
            ou = make_mlp(rng, ds + nlc, [t], 'tanh', out_activation='softmax', bn_random=True)
        st['dropout'], ou['dropout'] = {0: 0.2}, {0: 0.1}
        layers.append(dict(net_state=st, net_output=ou, state_vect_dim=d, max_iteration=max_it, threshold=0.0))
        s0.append((0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None)
        ms.append([{0: rng.random((n, st['weights'][0].shape[0])) > 0.2} for _ in range(max_it)])
        mo.append({0: rng.random((m, ds + nlc)) > 0.1})
        cls = GNNgraphBased if graph_based else GNNnodeBased
        gnns.append(cls(net_state=sequential(st), net_output=sequential(ou), optimizer=None, loss_function=None, loss_arguments=None,
                        state_vect_dim=d, max_iteration=max_it, threshold=0.0, addressed_problem='c'))
        nl_i = nl + get_state * ds + get_output * t
    ref = tro.lgnn_train_step(g, layers, get_state, get_output, mode, s0, ms, mo, targets, weights, loss=loss, mean=False, graph_based=graph_based)

    loss_fn = losses.categorical_crossentropy if loss == 'categorical_crossentropy' else losses.mean_squared_error
    lgnn = LGNN(gnns, get_state, get_output, optimizers.SGD(0.0), loss_fn, None, 'c')
    lgnn.training_mode = mode
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, NodeGraph=ng,
                     problem_based='g' if graph_based else 'n', aggregation_mode='average')
    gt = GraphTensor.fromGraphObject(go)
    res = lgnn.training_step(gt, mean=False, state0=s0,
                             masks_state=[np.concatenate([mk[0].astype(np.uint8).ravel() for mk in msl]) for msl in ms],
                             masks_output=[mol[0].astype(np.uint8).ravel() for mol in mo])
    assert res['k'] == ref['k']
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for li in range(L):
        np.testing.assert_allclose(res['outs'][li], ref['outs'][li], atol=2e-5)
        for got, want in list(zip(res['grads_state'][li], ref['grads_state'][li])) + list(zip(res['grads_output'][li], ref['grads_output'][li])):
            assert got.shape == want.shape
            assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (li, got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))


def test_lgnn_parallel_training_reduces_loss():
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(1)
    set_seed(1)
    graphs = []
    for _ in range(5):
        n = 100
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        cls = (nodes[:, 0] - 0.5 * nodes[:, 2] > 0).astype(int)
        graphs.append(GraphObject(arcs=random_arcs(rng, n, 300, 1), nodes=nodes, targets=np.eye(2)[cls]))

    def model(layer):
        w = 3 + 2 * (layer > 0)
        st = MLP(1 + 2 * w, [8, w], 'tanh', 'glorot_normal', 'zeros', dropout_rate=0.1, dropout_pos=0)
        ou = MLP(w, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
        return GNNnodeBased(net_state=st, net_output=ou, optimizer=None, loss_function=losses.categorical_crossentropy, loss_arguments=None,
                            state_vect_dim=0, max_iteration=3, threshold=0.01, addressed_problem='c')

    for mode in ('parallel', 'residual'):
        lgnn = LGNN([model(0), model(1), model(1)], False, True, optimizers.Adam(0.02), losses.categorical_crossentropy, None, 'c',
                    extra_metrics={'Acc': lambda yt, yp: float(np.mean(yt == yp))})
        before = lgnn.test(graphs[4])
        lgnn.train(graphs[:4], 30, graphs[4], update_freq=10, max_fails=50, training_mode=mode, verbose=0)
        after = lgnn.test(graphs[4])
        assert after['Loss'] < 0.7 * before['Loss'] and after['Acc'] > 0.8, (mode, before, after)
        with pytest.raises(ValueError):
            lgnn.train(graphs[:4], 1, training_mode='serial', verbose=0)      # the mode of a model cannot change (reference LGNN.py:318-319)


@pytest.mark.parametrize('d', [4, 0])
def test_edge_based_training_step_matches_oracle(d):
    """GNNedgeBased training (reference GNN.py:289-302 under GNN_BaseClass.py:231-247): per-arc readout in training mode and
    its backward pass (both endpoints of every masked arc receive gradient), through GNNedgeBased.training_step."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNedgeBased
    from GNN.MLP import Sequential, Dense, Dropout, BatchNormalization
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(60 + d)
    n, nl, al, max_it = 200, 3, 2, 4
    arcs = random_arcs(rng, n, 600, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    e = len(arcs)
    set_mask = rng.random(e) < 0.75
    targets_full = np.eye(2)[rng.integers(0, 2, e)].astype(np.float32)
    weights_full = rng.uniform(0.5, 1.5, e).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'], g['output_mask'] = set_mask, np.ones(e, bool)
    m = int(set_mask.sum())
    ds, nlc = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nlc), [12, ds], 'tanh', gain=0.8, bn_random=True)
    ou = make_mlp(rng, 2 * (ds + nlc) + al, [7, 2], 'tanh', out_activation='softmax')
    ou.update(batch_normalization=False, weights=ou['weights'][:4])
    st['dropout'], ou['dropout'] = {0: 0.2}, {1: 0.3}
    ms = [{0: rng.random((n, st['weights'][0].shape[0])) > 0.2} for _ in range(max_it)]
    mo = {1: rng.random((m, 7)) > 0.3}
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
    ref = tro.train_step(g, st, ou, d, max_it, 0.0, s0, ms, mo, targets_full[set_mask], weights_full[set_mask], mean=False, edge_based=True)

    def sequential(net):
        layers = []
        for l in range(len(net['activations'])):
            if net['dropout'].get(l): layers.append(Dropout(net['dropout'][l]))
            layers.append(Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)))
        if net['batch_normalization']: layers.append(BatchNormalization())
        seq = Sequential(layers)
        seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
        return seq

    gnn = GNNedgeBased(net_state=sequential(st), net_output=sequential(ou), optimizer=optimizers.SGD(0.0),
                       loss_function=losses.categorical_crossentropy, loss_arguments=None, state_vect_dim=d, max_iteration=max_it,
                       threshold=0.0, addressed_problem='c')
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based='a',
                     aggregation_mode='average')
    res = gnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=s0,
                            masks_state=np.concatenate([mk[0].astype(np.uint8).ravel() for mk in ms]), masks_output=mo[1].astype(np.uint8).ravel())
    assert res['k'] == ref['k'] == max_it
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for got, want in list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])):
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))
    # run-to-run identical: the endpoint gradients are gathered per node in a fixed order (no float atomics) - learning rate 0, same masks
    res2 = gnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=s0,
                             masks_state=np.concatenate([mk[0].astype(np.uint8).ravel() for mk in ms]), masks_output=mo[1].astype(np.uint8).ravel())
    for a, b in zip(res['grads_state'] + res['grads_output'], res2['grads_state'] + res2['grads_output']):
        assert np.array_equal(a, b)
    # and a few Adam steps reduce the loss of a learnable arc task (label = sign of the first arc label)
    cls = (arcs[:, 2] > np.median(arcs[:, 2])).astype(int)
    go2 = GraphObject(arcs=arcs, nodes=nodes, targets=np.eye(2)[cls], problem_based='a', aggregation_mode='average')
    gnn2 = GNNedgeBased(net_state=sequential(dict(st, dropout={})), net_output=sequential(dict(ou, dropout={})), optimizer=optimizers.Adam(0.02),
                        loss_function=losses.categorical_crossentropy, loss_arguments=None, state_vect_dim=d, max_iteration=max_it,
                        threshold=0.01, addressed_problem='c')
    before = gnn2.test(go2)['Loss']
    gnn2.train(go2, 25, None, update_freq=25, verbose=0)
    assert gnn2.test(go2)['Loss'] < 0.7 * before


@pytest.mark.parametrize('d,get_state,get_output,mode', [(4, True, True, 'parallel'), (0, False, True, 'residual')])
def test_edge_lgnn_joint_training_step_matches_oracle(d, get_state, get_output, mode):
    """Edge-based LGNN in 'parallel' / 'residual' mode: the arc-label gradient (gnn_loop_train_backward: d_arc_labels) carries
    layer i + 1's loss back to layer i's outputs (reference LGNN.py:253-254 under GNN_BaseClass.py:231-247)."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNedgeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import Sequential, Dense, Dropout, BatchNormalization
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(90 + d)
    n, nl, al, t, max_it, L = 150, 3, 2, 2, 3, 3
    arcs = random_arcs(rng, n, 400, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    e = len(arcs)
    set_mask = rng.random(e) < 0.75
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'], g['output_mask'] = set_mask, np.ones(e, bool)
    m = int(set_mask.sum())
    targets_full = rng.random((e, t)).astype(np.float32)
    weights_full = rng.uniform(0.5, 1.5, e).astype(np.float32)

    def sequential(net):
        layers = []
        for l in range(len(net['activations'])):
            if net['dropout'].get(l): layers.append(Dropout(net['dropout'][l]))
            layers.append(Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)))
        if net['batch_normalization']: layers.append(BatchNormalization())
        seq = Sequential(layers)
        seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
        return seq

    layers, s0, ms, mo, gnns = [], [], [], [], []
    for i in range(L):
        ins, ls = orc.get_inout_dims('state', nl, al, t, 'a', d, [10], layer=i, get_state=get_state, get_output=get_output)
        ino, lo = orc.get_inout_dims('output', nl, al, t, 'a', d, None, layer=i, get_state=get_state, get_output=get_output)
        st = make_mlp(rng, ins, ls, 'tanh', gain=0.8, bn_random=True)
        ou = make_mlp(rng, ino, lo, 'tanh', out_activation='softmax', bn_random=True)
        st['dropout'], ou['dropout'] = {0: 0.2}, {0: 0.1}
        layers.append(dict(net_state=st, net_output=ou, state_vect_dim=d, max_iteration=max_it, threshold=0.0))
        s0.append((0.1 * rng.standard_normal((n, d))).astype(np.float32) if d else None)
        ms.append([{0: rng.random((n, ins)) > 0.2} for _ in range(max_it)])
        mo.append({0: rng.random((m, ino)) > 0.1})
        gnns.append(GNNedgeBased(net_state=sequential(st), net_output=sequential(ou), optimizer=None, loss_function=None, loss_arguments=None,
                                 state_vect_dim=d, max_iteration=max_it, threshold=0.0, addressed_problem='r'))
    ref = tro.lgnn_train_step(g, layers, get_state, get_output, mode, s0, ms, mo, targets_full[set_mask], weights_full[set_mask],
                              loss='mean_squared_error', mean=False, edge_based=True)
    lgnn = LGNN(gnns, get_state, get_output, optimizers.SGD(0.0), losses.mean_squared_error, None, 'r')
    lgnn.training_mode = mode
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based='a',
                     aggregation_mode='average')
    res = lgnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=s0,
                             masks_state=[np.concatenate([mk[0].astype(np.uint8).ravel() for mk in msl]) for msl in ms],
                             masks_output=[mol[0].astype(np.uint8).ravel() for mol in mo])
    assert res['k'] == ref['k']
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for li in range(L):
        np.testing.assert_allclose(res['outs'][li], ref['outs'][li], atol=2e-5)
        for got, want in list(zip(res['grads_state'][li], ref['grads_state'][li])) + list(zip(res['grads_output'][li], ref['grads_output'][li])):
            assert got.shape == want.shape
            assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (li, got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize('cls_name', ['GNNnodeBased', 'GNNgraphBased', 'GNNedgeBased'])
def test_loop_training_mode_forward(cls_name):
    """Loop(g, training=True) (reference GNN.py:251-280 with Keras layers in training mode): BatchNormalization on batch
    statistics (no Dropout here, so the oracle needs no masks); moving statistics move once per BN call."""
    import GNN.GNN as G
    from GNN import losses
    from GNN.MLP import MLP
    from GNN.graph_class import GraphObject, GraphTensor
    cls = getattr(G, cls_name)
    rng = np.random.default_rng(7)
    n, nl, al, d, t = 120, 3, 2, 5, 2
    arcs = random_arcs(rng, n, 300, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    e = len(arcs)
    pb = {'GNNnodeBased': 'n', 'GNNgraphBased': 'g', 'GNNedgeBased': 'a'}[cls_name]
    g = orc.make_graph_dict(arcs, nodes, 'average')
    kw = {}
    if pb == 'a':
        g['set_mask'], g['output_mask'] = rng.random(e) < 0.8, np.ones(e, bool)
        kw = dict(set_mask=g['set_mask'])
        n_t = e
    elif pb == 'g':
        ng = np.zeros((n, 2), np.float32); ng[:70, 0] = 1 / 70; ng[70:, 1] = 1 / 50
        g['NodeGraph'] = ng
        kw = dict(NodeGraph=ng)
        n_t = 2
    else:
        g['set_mask'] = rng.random(n) < 0.8
        kw = dict(set_mask=g['set_mask'])
        n_t = n
    ins, ls = orc.get_inout_dims('state', nl, al, t, pb, d, [9])
    ino, lo = orc.get_inout_dims('output', nl, al, t, pb, d, None)
    st, ou = make_mlp(rng, ins, ls, 'tanh', gain=0.7, bn_random=True), make_mlp(rng, ino, lo, 'tanh', out_activation='softmax', bn_random=True)
    st['dropout'], ou['dropout'] = {}, {}

    def build(net):
        m = MLP(input_dim=net['weights'][0].shape[0], layers=[w.shape[1] for w in net['weights'][0:2 * len(net['activations']):2]],
                activations=net['activations'], kernel_initializer='zeros', bias_initializer='zeros')
        m.set_weights([np.asarray(w, np.float32) for w in net['weights']])
        return m

    gnn = cls(net_state=build(st), net_output=build(ou), optimizer=None, loss_function=losses.mean_squared_error, loss_arguments=None,
              state_vect_dim=d, max_iteration=4, threshold=0.0, addressed_problem='r')
    go = GraphObject(arcs=arcs, nodes=nodes, targets=rng.random((n_t, t)), problem_based=pb, aggregation_mode='average', **kw)
    gt = GraphTensor.fromGraphObject(go)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    k, state, out = gnn.Loop(gt, training=True, state0=s0)
    ctx = tro.train_forward(g, st, ou, d, 4, 0.0, s0, [{}] * 4, {}, edge_based=pb == 'a')
    want = ctx['out_nodes'] if pb != 'g' else np.asarray(g['NodeGraph'], np.float64).T @ ctx['out_nodes']
    assert k == ctx['k'] == 4
    assert np.max(np.abs(state - ctx['state'])) < 2e-5 and np.max(np.abs(out - want)) < 2e-5
    mm, mv = gnn.net_state.layers[-1].moving_mean, gnn.net_state.layers[-1].moving_variance
    np.testing.assert_allclose(mm, ctx['moving_state'][0], atol=1e-5)
    np.testing.assert_allclose(mv, ctx['moving_state'][1], atol=1e-5)
    it, loss, targs, o2 = gnn.evaluate_single_graph(gt, training=True)          # reference GNN.py:180-199
    assert np.isfinite(loss) and targs.shape == o2.shape
    k_inf, _, out_inf = gnn.Loop(gt, training=False, state0=s0)                  # inference mode still uses the moving statistics
    assert out_inf.shape == out.shape and not np.allclose(out_inf, out, atol=1e-4)


def test_training_forward_after_a_folded_readout():
    """An inference Loop of a small graph-based model folds the graph readout NodeGraph^T . out (reference GNN.py:331-332) into its
    persistent launch from the second Loop on (result in pinned host memory).  A training-mode Loop on the same loop handle rewrites the
    node outputs without going through the inference set-up: its readout must come from ITS outputs, not from the host copy the earlier
    inference run left (round-3 advisor finding: train + evaluate(gTr) + train would have computed loss and gradients from stale outputs)."""
    import GNN.GNN as G
    from GNN import losses
    from GNN.MLP import MLP
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(17)
    n, nl, al, d, t = 120, 3, 2, 5, 2
    arcs = random_arcs(rng, n, 300, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    ng = np.zeros((n, 2), np.float32); ng[:70, 0] = 1 / 70; ng[70:, 1] = 1 / 50
    g['NodeGraph'] = ng
    ins, ls = orc.get_inout_dims('state', nl, al, t, 'g', d, [9])
    ino, lo = orc.get_inout_dims('output', nl, al, t, 'g', d, None)
    st, ou = make_mlp(rng, ins, ls, 'tanh', gain=0.7, bn_random=True), make_mlp(rng, ino, lo, 'tanh', out_activation='softmax', bn_random=True)
    st['dropout'], ou['dropout'] = {}, {}

    def build(net):
        m = MLP(input_dim=net['weights'][0].shape[0], layers=[w.shape[1] for w in net['weights'][0:2 * len(net['activations']):2]],
                activations=net['activations'], kernel_initializer='zeros', bias_initializer='zeros')
        m.set_weights([np.asarray(w, np.float32) for w in net['weights']])
        return m

    gnn = G.GNNgraphBased(net_state=build(st), net_output=build(ou), optimizer=None, loss_function=losses.mean_squared_error, loss_arguments=None,
                          state_vect_dim=d, max_iteration=4, threshold=0.0, addressed_problem='r')
    go = GraphObject(arcs=arcs, nodes=nodes, targets=rng.random((2, t)), problem_based='g', aggregation_mode='average', NodeGraph=ng)
    gt = GraphTensor.fromGraphObject(go)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    k1, _, out1 = gnn.Loop(gt, training=False, state0=s0)          # uploads the NodeGraph
    k2, _, out2 = gnn.Loop(gt, training=False, state0=s0)          # readout inside the persistent launch
    assert np.array_equal(out1, out2)
    k, state, out = gnn.Loop(gt, training=True, state0=s0)
    ctx = tro.train_forward(g, st, ou, d, 4, 0.0, s0, [{}] * 4, {}, edge_based=False)
    want = np.asarray(ng, np.float64).T @ ctx['out_nodes']
    assert k == ctx['k'] == 4
    assert np.max(np.abs(out - want)) < 2e-5, (np.max(np.abs(out - want)), np.max(np.abs(out - out2)))
    assert not np.allclose(out, out2, atol=1e-4)                   # (batch statistics: the training-mode outputs do differ from the inference ones)


def test_regularizers_join_the_device_gradients():
    from GNN import losses, optimizers, regularizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(3)
    set_seed(3)
    n = 80
    go = GraphObject(arcs=random_arcs(rng, n, 200, 1), nodes=(2 * rng.random((n, 3)) - 1).astype(np.float32), targets=np.eye(2)[rng.integers(0, 2, n)])
    gt = GraphTensor.fromGraphObject(go)

    def model(reg):
        set_seed(3)
        st = MLP(1 + 2 * 3, [6, 3], 'tanh', 'glorot_normal', 'zeros', kernel_regularizer=reg, batch_normalization=False)
        ou = MLP(3, [2], 'softmax', 'glorot_normal', 'zeros', bias_regularizer=reg, batch_normalization=False)
        return GNNnodeBased(net_state=st, net_output=ou, optimizer=optimizers.SGD(0.0), loss_function=losses.categorical_crossentropy,
                            loss_arguments=None, state_vect_dim=0, max_iteration=3, threshold=0.0, addressed_problem='c')

    plain, reg = model(None), model(regularizers.l2(0.05))
    a, b = plain.training_step(gt, mean=False), reg.training_step(gt, mean=False)
    w = plain.net_state.get_weights()
    assert b['loss'] > a['loss']
    np.testing.assert_allclose(b['grads_state'][0], a['grads_state'][0] + 0.1 * w[0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b['grads_state'][1], a['grads_state'][1], rtol=1e-5, atol=1e-6)          # bias of net_state: no regularizer
    np.testing.assert_allclose(b['grads_output'][1], a['grads_output'][1] + 0.1 * plain.net_output.get_weights()[1], rtol=1e-5, atol=1e-6)



def test_training_forward_stops_at_convergence():
    """The while-condition of the training-mode Loop (GNN.py:271) with a contractive net and no BatchNormalization / Dropout:
    deterministic on the device, so the executed bodies must equal the float64 oracle's, and be fewer than max_iteration."""
    from GNN import _engine as e
    rng = np.random.default_rng(17)
    n, nl, al, d, max_it = 300, 3, 2, 6, 30
    arcs = random_arcs(rng, n, 900, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    st = make_mlp(rng, al + 2 * (d + nl), [10, d], 'tanh', gain=0.5)
    ou = make_mlp(rng, d + nl, [2], 'tanh', out_activation='softmax')
    for net in (st, ou):
        net.update(batch_normalization=False, weights=net['weights'][:-4], dropout={})
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    targets = np.eye(2)[rng.integers(0, 2, n)].astype(np.float32)
    weights = np.ones(n, np.float32)
    ref = tro.train_step(g, st, ou, d, max_it, 0.02, s0, [{}] * max_it, {}, targets, weights, mean=True)
    assert 2 <= ref['k'] < max_it
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], False), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, d, max_it, 0.02)
    loop.set_state0(s0)
    res = loop.train_step(mst, mou, None, targets, weights, 0)
    assert res['k'] == ref['k']
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    k = ref['k']
    for got, want in zip(res['grads_state'], ref['grads_state']):      # the oracle divided by k (mean=True); the device returns raw sums
        assert np.max(np.abs(got / k - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want)))
    for got, want in zip(res['grads_output'], ref['grads_output']):
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want)))



@pytest.mark.gpu
@pytest.mark.parametrize('opt_name,graph_based', [('Adam', False), ('Adam', True), ('SGD', False)])
def test_device_optimizer_matches_host_optimizer(opt_name, graph_based):
    """gnn_loop_arm_optimizer (weights, slots, gradients stay in HBM) against the NumPy optimizers of GNN/optimizers.py on the
    same gradients: three steps of the same model trained both ways must leave the same weights, BatchNormalization
    moving statistics included (reference GNN_BaseClass.py:243-247)."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(5)
    gg = []
    for i in range(4):
        n = 50
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        tg = np.eye(2)[[i % 2]] if graph_based else np.eye(2)[rng.integers(0, 2, n)]
        gg.append(GraphObject(arcs=random_arcs(rng, n, 150, 1), nodes=nodes, targets=tg, problem_based='g' if graph_based else 'n'))
    batch = GraphObject.merge(gg, problem_based='g' if graph_based else 'n', aggregation_mode='average')

    def model(device_optimizer):
        set_seed(3)
        st = MLP(1 + 2 * 3, [8, 3], 'selu', 'glorot_normal', 'zeros')                       # BatchNormalization on (default)
        ou = MLP(3, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
        opt = optimizers.Adam(0.01) if opt_name == 'Adam' else optimizers.SGD(0.01, momentum=0.9)
        m = (GNNgraphBased if graph_based else GNNnodeBased)(net_state=st, net_output=ou, optimizer=opt, loss_function=losses.categorical_crossentropy,
                                                             loss_arguments=None, state_vect_dim=0, max_iteration=3, threshold=0.001, addressed_problem='c')
        m.device_optimizer = device_optimizer
        return m

    host, dev = model(False), model(True)
    for a, b in zip(host.net_state.get_weights(), dev.net_state.get_weights()):
        assert np.array_equal(a, b)
    for _ in range(3):
        rh = host.training_step(batch, True)
        rd = dev.training_step(batch, True)
        assert rh['k'] == rd['k'] and abs(rh['loss'] - rd['loss']) <= 1e-4 * max(1.0, abs(rh['loss']))
    assert dev.net_state._host_stale                       # nothing has been read back yet
    for net_h, net_d in ((host.net_state, dev.net_state), (host.net_output, dev.net_output)):
        for a, b in zip(net_h.get_weights(), net_d.get_weights()):
            assert np.max(np.abs(a - b)) <= 5e-5 * max(1.0, np.max(np.abs(a)))       # float32 slots on the device, float64 in NumPy
    assert not dev.net_state._host_stale
    # the refreshed host copies and the device agree: an inference Loop after set_weights(get_weights()) gives the same output
    k0, _, out0 = dev.Loop(batch)
    dev.net_state.set_weights(dev.net_state.get_weights())
    k1, _, out1 = dev.Loop(batch)
    assert k0 == k1 and np.array_equal(out0, out1)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_lgnn_device_optimizer_matches_host_optimizer(mode):
    """The joint LGNN step with gnn_loop_optimizer_step per layer (one optimizer step over all layers, reference
    GNN_BaseClass.py:244-247) against the NumPy optimizer on the same gradients: same weights after two steps."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(2)
    n = 90
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    g = GraphObject(arcs=random_arcs(rng, n, 270, 1), nodes=nodes, targets=np.eye(2)[rng.integers(0, 2, n)])

    def build(device_optimizer):
        set_seed(4)

        def model(layer):
            w = 3 + 2 * (layer > 0)
            st = MLP(1 + 2 * w, [8, w], 'tanh', 'glorot_normal', 'zeros')                 # BatchNormalization on
            ou = MLP(w, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
            return GNNnodeBased(net_state=st, net_output=ou, optimizer=None, loss_function=losses.categorical_crossentropy, loss_arguments=None,
                                state_vect_dim=0, max_iteration=3, threshold=0.01, addressed_problem='c')

        lg = LGNN([model(0), model(1)], False, True, optimizers.Adam(0.01), losses.categorical_crossentropy, None, 'c')
        lg.device_optimizer = device_optimizer
        lg.training_mode = mode
        return lg

    host, dev = build(False), build(True)
    for _ in range(2):
        rh, rd = host.training_step(g, True), dev.training_step(g, True)
        assert rh['k'] == rd['k'] and abs(rh['loss'] - rd['loss']) <= 1e-4 * max(1.0, abs(rh['loss']))
    for gh, gd in zip(host.gnns, dev.gnns):
        assert gd.net_state._host_stale
        for net_h, net_d in ((gh.net_state, gd.net_state), (gh.net_output, gd.net_output)):
            for a, b in zip(net_h.get_weights(), net_d.get_weights()):
                assert np.max(np.abs(a - b)) <= 5e-5 * max(1.0, np.max(np.abs(a)))


@pytest.mark.parametrize('n,with_dropout,d,hidden', [(6000, False, 64, (128, 128)), (4500, True, 64, (128, 128)), (4200, False, 64, (100, 96)), (4131, False, 64, (72, 128)), (4300, False, 48, (100, 96))])
def test_wide_layers_on_the_matrix_cores_match_oracle(n, with_dropout, d, hidden):
    """BASELINE configs[2] net shape (state_dim 64, 135 -> 128 -> 128 -> 64) on enough rows for the matrix-core products of the training
    step (gnn_train_wide.hip: k_gemm_f32 forward / d h_in, k_wgrad_f32 weight gradients; gnn_train.hip: k_train_input_rows): loss, k and every gradient array
    against the float64 oracle to 2e-4 of the array's largest entry (1e-3, the bar of the small-shape tests above, with Dropout in the
    net).  Measured on this step (tools/dbg/train_acc.py, profiles/r03_train_c3.txt): split-bf16 products 1.1e-4, f32-MFMA chain 3.1e-4,
    per-op FP32-ALU kernels 2.6e-4 - the bias gradients are the least accurate arrays in all three.  A repeated step gives the same bits
    (per-chunk partials are added in a fixed order).  Without Dropout the backward chain of the three layers runs in ONE pass (k_bwd3_split,
    round 5): also with hidden widths below 128 / a state narrower than 64 (zero-padded feature tiles) and a partial last 32-row tile.
    Whole steps of three bodies at the tolerances of the small-shape tests; the kernels one by one - every instantiation, second tiles, single
    rows, at the float32 noise of the oracle - are in tests/test_gpu_train_forms.py."""
    from GNN import _engine as e
    rng = np.random.default_rng(n)
    nl, al, max_it = 3, 1, 3
    arcs = random_arcs(rng, n, 4 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.9
    # (the added shapes use a SMOOTH activation: a SELU pre-activation next to its kink flips sides between any two float32 evaluation orders, and one flip
    #  among a few thousand rows is a 1e-4 .. 1e-3 gradient error in EVERY implementation - tools/dbg/fwd3_widths.py: per-layer forward 3e-7 / fused 1e-3 on
    #  one shape, 1.9e-4 / 4e-7 on another - so a tight tolerance on SELU tests the seed, not the kernels)
    act = 'selu' if (tuple(hidden) == (128, 128) and d == 64) else 'tanh'
    st = make_mlp(rng, al + 2 * (d + nl), list(hidden) + [d], act, gain=0.7, bn_random=True)
    ou = make_mlp(rng, d + nl, [2], 'softmax', batch_normalization=False)      # (BatchNormalization right after a softmax is ill-conditioned: 3e-3 in float32 whichever kernels run)
    rate = 0.1 if with_dropout else 0.0                     # Dropout behind the first hidden layer: the d h_in epilogue of the wide product
    st['dropout'], ou['dropout'] = ({1: rate} if with_dropout else {}), {}
    mask = g['set_mask'] & g['output_mask']
    m = int(mask.sum())
    masks_s = [({1: rng.random((n, hidden[0])) > rate} if with_dropout else {}) for _ in range(max_it)]
    targets = np.eye(2)[rng.integers(0, 2, m)].astype(np.float32)
    weights = (rng.uniform(0.5, 1.5, m) / m).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    ref = tro.train_step(g, st, ou, d, max_it, 0.0, s0, masks_s, {}, targets, weights, loss='categorical_crossentropy', mean=False, graph_based=False)
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, d, max_it, 0.0)
    loop.set_state0(s0)
    ms = np.concatenate([masks_s[k][1].astype(np.uint8).ravel() for k in range(max_it)]) if with_dropout else None
    runs = []
    for _ in range(2):
        runs.append(loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, 0, None, dropout_state=[0, rate, 0, 0], dropout_output=[0, 0],
                                    masks_state=ms, masks_output=None, bn_state=np.concatenate(st['weights'][-4:-2]), bn_output=None))
    res = runs[0]
    assert res['k'] == ref['k'] == max_it
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    pairs = list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output']))
    scale = max(float(np.max(np.abs(want))) for _, want in pairs)           # the largest gradient entry of the step
    tol = 1e-3 if with_dropout else 2e-4
    for got, want in pairs:
        assert got.shape == want.shape
        # relative to the array's largest entry, but not below a tenth of the step's gradient scale (the small bias / BatchNormalization vectors)
        assert np.max(np.abs(got - want)) <= tol * max(0.1 * scale, np.max(np.abs(want))), (got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)), scale)
    for a, b in zip(runs[0]['grads_state'] + runs[0]['grads_output'], runs[1]['grads_state'] + runs[1]['grads_output']):
        assert np.array_equal(a, b)


def test_train_step_random_shapes():
    """gnn_loop_train_step on 14 seeded random shapes (state width 0 / 1 .. 64, 0 - 2 hidden layers of 1 .. 128 units, smooth activations -
    the kinks of relu / selu make single gradient entries jump between float32 and float64, DESIGN.md section 7 - with and without
    BatchNormalization, 40 .. 9,000 nodes): k, loss and every gradient array against the float64 oracle, and identical bits on a repeated
    step.  With this seed every case has fewer than 4,096 rows or no wide layer: the per-op kernels and k_mlp_fwd run here, no matrix-core
    form does (those: test_wide_layers_on_the_matrix_cores_match_oracle and tests/test_gpu_train_forms.py)."""
    from GNN import _engine as e
    rng = np.random.default_rng(20261006)
    for case in range(14):
        d = int(rng.choice([0, 1, 4, 8, 16, 33, 64]))
        nl = int(rng.integers(1, 6)) if d else int(rng.choice([2, 7, 16]))
        al = int(rng.integers(1, 4))
        hidden = [int(x) for x in rng.choice([1, 9, 32, 64, 100, 128], size=int(rng.integers(0, 3)))]
        n = int(rng.choice([40, 333, 2000, 5000, 9000]))
        act = ['tanh', 'sigmoid', 'linear'][case % 3]
        bn = bool(case % 4 != 3)
        max_it = int(rng.integers(1, 5))
        arcs = random_arcs(rng, n, int(rng.choice([1, 3, 8])) * n, al)
        nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
        g = orc.make_graph_dict(arcs, nodes, str(rng.choice(['average', 'sum', 'normalized'])))
        g['set_mask'] = rng.random(n) < 0.7
        ds, nlc = (d if d else nl), (nl if d else 0)
        st = make_mlp(rng, al + 2 * (ds + nlc), hidden + [ds], act, gain=0.5, bn_random=True, batch_normalization=bn)
        ou = make_mlp(rng, ds + nlc, [2], 'softmax', batch_normalization=False)      # (BatchNormalization behind a softmax leaves [0, 1]: the loss clips, its gradient is ill-conditioned in float32 and float64 alike)
        st['dropout'], ou['dropout'] = {}, {}
        mask = g['set_mask'] & g['output_mask']
        m = int(mask.sum())
        targets = np.eye(2)[rng.integers(0, 2, m)].astype(np.float32)
        weights = (rng.uniform(0.5, 1.5, m) / m).astype(np.float32)
        s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
        ref = tro.train_step(g, st, ou, d, max_it, 0.0, s0, [{} for _ in range(max_it)], {}, targets, weights, loss='categorical_crossentropy', mean=False, graph_based=False)
        graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
        mst, mou = e.Mlp(st['weights'], st['activations'], bn), e.Mlp(ou['weights'], ou['activations'], False)
        loop = e.Loop(graph, mst, mou, d, max_it, 0.0)
        if d: loop.set_state0(s0)
        kw = dict(dropout_state=[0.0] * (len(hidden) + 2), dropout_output=[0.0, 0.0],
                  bn_state=np.concatenate(st['weights'][-4:-2]) if bn else None, bn_output=None)
        res = loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, 0, None, **kw)
        tag = (case, d, nl, al, hidden, n, act, bn, max_it)
        assert res['k'] == ref['k'], tag
        assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss'])), tag
        gscale = max(float(np.max(np.abs(w_))) for w_ in ref['grads_state'] + ref['grads_output'])
        for got, want in list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])):
            assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-3 * max(float(np.max(np.abs(want))), 0.05 * gscale), \
                (tag, got.shape, float(np.max(np.abs(got - want))), float(np.max(np.abs(want))))
        res2 = loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, 0, None, **kw)
        assert all(np.array_equal(a_, b_) for a_, b_ in zip(res['grads_state'] + res['grads_output'], res2['grads_state'] + res2['grads_output'])), tag
        loop.close()
