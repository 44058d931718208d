"""Kernel / bias regularizers and gradient clipping inside the device-side training step (gnn_mlp_set_regularizers,
gnn_loop_set_clipping, gnn_loop_grad_sqnorm / gnn_loop_optimizer_step_scaled) against their NumPy mirrors in GNN/optimizers.py and
GNN/regularizers.py.  net_state is 7 -> 40 -> 3 with BatchNormalization: a gradient vector of 449 entries, i.e. two 256-thread
blocks with a partial last one, array boundaries inside a block and arrays of 3 entries; net_output is 3 -> 2."""
import ctypes as C

import numpy as np
import pytest

from util import random_arcs

pytestmark = pytest.mark.gpu


def _batch(graph_based=False):
    """4 graphs x 50 nodes, 150 arcs each, merged."""
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(5)
    gg = []
    for i in range(4):
        n = 50
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        tg = np.eye(2)[[i % 2]] if graph_based else np.eye(2)[rng.integers(0, 2, n)]
        gg.append(GraphObject(arcs=random_arcs(rng, n, 150, 1), nodes=nodes, targets=tg, problem_based='g' if graph_based else 'n'))
    return GraphTensor.fromGraphObject(GraphObject.merge(gg, problem_based='g' if graph_based else 'n', aggregation_mode='average'))


def _model(opt, device_optimizer=True, graph_based=False, reg=True, seed=3):
    from GNN import losses, regularizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased
    from GNN.MLP import MLP, set_seed
    set_seed(seed)
    st = MLP(1 + 2 * 3, [40, 3], 'tanh', 'glorot_normal', 'zeros', kernel_regularizer=regularizers.l1_l2(1e-3, 5e-2) if reg else None)
    ou = MLP(3, [2], 'softmax', 'glorot_normal', 'zeros', bias_regularizer=regularizers.l2(5e-2) if reg else None, batch_normalization=False)
    assert sum(a.size for a in st.trainable_variables) == 449
    m = (GNNgraphBased if graph_based else GNNnodeBased)(net_state=st, net_output=ou, optimizer=opt, loss_function=losses.categorical_crossentropy,
                                                         loss_arguments=None, state_vect_dim=0, max_iteration=3, threshold=0.001, addressed_problem='c')
    m.device_optimizer = device_optimizer
    return m


def _trainable(m):
    return [np.array(a, np.float32) for a in m.net_state.trainable_variables + m.net_output.trainable_variables]


def _scaled(res):
    """The gradients of a step as the optimizer sees them with mean=True: net_state's divided by k, in float64."""
    return [np.asarray(a, np.float64) / res['k'] for a in res['grads_state']] + [np.asarray(a, np.float64) for a in res['grads_output']]


def _global_norm(arrays):
    return float(np.sqrt(sum(float(np.sum(a * a)) for a in arrays)))


def _same_training(host, dev, batch, steps):
    """The project's bars for device against host (tests/test_gpu_train.py, test_device_optimizer_matches_host_optimizer)."""
    for _ in range(steps):
        rh, rd = host.training_step(batch, True), dev.training_step(batch, True)
        print('k', rh['k'], rd['k'], 'loss', rh['loss'], rd['loss'])
        assert rh['k'] == rd['k'] and abs(rh['loss'] - rd['loss']) <= 1e-4 * max(1.0, abs(rh['loss']))
    assert dev.net_state._host_stale and dev.net_output._host_stale            # the step stayed on the device: nothing read back yet
    assert not host.net_state._host_stale
    for net_h, net_d in ((host.net_state, dev.net_state), (host.net_output, dev.net_output)):
        for a, b in zip(net_h.get_weights(), net_d.get_weights()):
            print('weights', a.shape, float(np.max(np.abs(a - b))))
            assert np.max(np.abs(a - b)) <= 5e-5 * max(1.0, np.max(np.abs(a)))


@pytest.mark.parametrize('opt_name,graph_based', [('Adam', False), ('Adam', True), ('SGD', False), ('SGD', True)])
def test_regularizers_on_the_device_match_the_host(opt_name, graph_based):
    """l1_l2(1e-3, 5e-2) on net_state's kernels, l2(5e-2) on net_output's bias: three steps on the device (k_grad_prepare in front of
    the armed update) against the host path (NumPy penalties, gradients and optimizer)."""
    from GNN import optimizers
    batch = _batch(graph_based)
    opt = lambda: optimizers.Adam(0.01) if opt_name == 'Adam' else optimizers.SGD(0.01, momentum=0.9)
    host, dev = _model(opt(), False, graph_based), _model(opt(), True, graph_based)
    _same_training(host, dev, batch, 3)


def _thresholds(kind, g):
    """The clipping thresholds of the exact check, from the scaled gradients g of the model: every one of them active."""
    if kind == 'global_clipnorm':
        assert _global_norm(g) > 0
        return dict(global_clipnorm=0.5 * _global_norm(g))
    clip = {}
    if kind in ('clipvalue', 'clipvalue+clipnorm'):
        flat = np.abs(np.concatenate([a.ravel() for a in g]))
        clip['clipvalue'] = c = float(np.median(flat))
        assert (flat > c).any() and (flat < c).any()
        g = [np.clip(a, -c, c) for a in g]               # (the norms clipnorm sees are those of the value-clipped arrays)
    if kind in ('clipnorm', 'clipvalue+clipnorm'):
        norms = np.sort([np.sqrt(np.sum(a * a)) for a in g])
        clip['clipnorm'] = c = float(0.5 * (norms[len(norms) // 2 - 1] + norms[len(norms) // 2]))
        assert (norms > c).any() and (norms < c).any()
    return clip


def _clip64(g, clipvalue=None, clipnorm=None, global_clipnorm=None):
    out = []
    for a in g:
        if clipvalue is not None: a = np.minimum(np.maximum(a, -clipvalue), clipvalue)
        if clipnorm is not None: a = a * clipnorm / max(np.sqrt(np.sum(a * a)), clipnorm)
        out.append(a)
    if global_clipnorm is not None:
        out = [a * global_clipnorm / max(_global_norm(out), global_clipnorm) for a in out]
    return out


@pytest.mark.parametrize('kind', ['clipvalue', 'clipnorm', 'global_clipnorm', 'clipvalue+clipnorm'])
def test_clipping_is_the_float64_clip_of_the_raw_gradients(kind):
    """One SGD step with learning rate 1 and no momentum: w_before - w_after IS the clipped gradient.  Bound: 1e-6 max(1, max |w|,
    max |g|) per array - three float32 roundings (the division by k, the factor, the product; <= 3 * 2^-24 relative) plus the one of
    w - g, with margin; the norms themselves are accumulated in double on the device."""
    from GNN import optimizers
    batch = _batch()
    probe = _model(optimizers.SGD(0.0), reg=False)
    g = _scaled(probe.training_step(batch, True))                # learning rate 0: the raw gradients of the model as it is built
    clip = _thresholds(kind, g)
    print(kind, clip)
    m = _model(optimizers.SGD(1.0, momentum=0.0, **clip), reg=False)
    before = _trainable(m)
    m.training_step(batch, True)
    assert m.net_state._host_stale
    after = _trainable(m)
    want = _clip64(g, **clip)
    assert any(np.max(np.abs(a - b)) > 1e-3 * np.max(np.abs(b)) for a, b in zip(want, g) if np.max(np.abs(b)) > 0)     # it did clip
    for w0, w1, gw, gr in zip(before, after, want, g):
        err = float(np.max(np.abs((w0.astype(np.float64) - w1.astype(np.float64)) - gw)))
        bound = 1e-6 * max(1.0, float(np.max(np.abs(w0))), float(np.max(np.abs(gr))))
        print(w0.shape, 'err', err, 'bound', bound)
        assert err <= bound


def test_clipping_with_regularizers_and_adam_matches_the_host():
    from GNN import optimizers
    batch = _batch()
    g = _scaled(_model(optimizers.SGD(0.0)).training_step(batch, True))      # (with the regularizer terms: the step returns them)
    c = 0.5 * _global_norm(g)
    host, dev = _model(optimizers.Adam(0.01, global_clipnorm=c), False), _model(optimizers.Adam(0.01, global_clipnorm=c), True)
    _same_training(host, dev, batch, 3)


def test_lgnn_joint_step_clips_by_the_norm_over_all_layers():
    """One optimizer step over the arrays of every layer (reference GNN_BaseClass.py:244-247): global_clipnorm takes ONE norm over both
    layers (gnn_loop_grad_sqnorm per loop, then gnn_loop_optimizer_step_scaled).  SGD with momentum, not Adam: Adam's update hardly
    depends on the scale of the gradient, so it could not tell the norm over all layers from a norm per layer."""
    from GNN import losses, optimizers, regularizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(2)
    n = 90
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    g = GraphObject(arcs=random_arcs(rng, n, 270, 1), nodes=nodes, targets=np.eye(2)[rng.integers(0, 2, n)])
    lr = 0.01

    def build(device_optimizer, opt):
        set_seed(4)

        def model(layer):
            w = 3 + 2 * (layer > 0)
            reg = regularizers.l2(5e-2) if layer == 1 else None
            st = MLP(1 + 2 * w, [8, w], 'tanh', 'glorot_normal', 'zeros', kernel_regularizer=reg)      # BatchNormalization on
            ou = MLP(w, [2], 'softmax', 'glorot_normal', 'zeros', kernel_regularizer=reg, batch_normalization=False)
            return GNNnodeBased(net_state=st, net_output=ou, optimizer=None, loss_function=losses.categorical_crossentropy, loss_arguments=None,
                                state_vect_dim=0, max_iteration=3, threshold=0.01, addressed_problem='c')

        lg = LGNN([model(0), model(1)], False, True, opt, losses.categorical_crossentropy, None, 'c')
        lg.device_optimizer = device_optimizer
        lg.training_mode = 'parallel'
        return lg

    def per_layer(res):      # [layer][array] scaled gradients (mean=True), float64
        return [[np.asarray(a, np.float64) / k for a in gs] + [np.asarray(a, np.float64) for a in go]
                for gs, go, k in zip(res['grads_state'], res['grads_output'], res['k'])]

    probe = build(False, optimizers.SGD(0.0)).training_step(g, True)          # host path, learning rate 0: the first step's gradients
    layers = per_layer(probe)
    c = 0.5 * _global_norm([a for layer in layers for a in layer])
    assert all(_global_norm(layer) > 0 for layer in layers)
    host, dev = build(False, optimizers.SGD(lr, momentum=0.9, global_clipnorm=c)), build(True, optimizers.SGD(lr, momentum=0.9, global_clipnorm=c))
    start = [[np.array(a, np.float64) for a in gnn.net_state.trainable_variables + gnn.net_output.trainable_variables] for gnn in host.gnns]
    bar = lambda a: 5e-5 * max(1.0, float(np.max(np.abs(a))))
    for step in range(2):
        rh, rd = host.training_step(g, True), dev.training_step(g, True)
        print('k', rh['k'], rd['k'], 'loss', rh['loss'], rd['loss'])
        assert rh['k'] == rd['k'] and abs(rh['loss'] - rd['loss']) <= 1e-4 * max(1.0, abs(rh['loss']))
        if step == 0:
            # the wrong answer: every layer clipped by its OWN norm.  It must lie outside the bar, or this test could not tell the two apart
            missed = False
            for gh, gd, w0, layer in zip(host.gnns, dev.gnns, start, layers):
                assert gd.net_state._host_stale
                f_own = c / max(_global_norm(layer), c)
                right = [np.array(a, np.float64) for a in gh.net_state.trainable_variables + gh.net_output.trainable_variables]
                got = [np.array(a, np.float64) for a in gd.net_state.trainable_variables + gd.net_output.trainable_variables]
                for a0, ga, r, d in zip(w0, layer, right, got):
                    assert np.max(np.abs(r - d)) <= bar(r)
                    missed = missed or float(np.max(np.abs((a0 - lr * f_own * ga) - r))) > bar(r)
            assert missed
    for gh, gd in zip(host.gnns, dev.gnns):
        assert gd.net_state._host_stale and gd.net_output._host_stale
        for net_h, net_d in ((gh.net_state, gd.net_state), (gh.net_output, gd.net_output)):
            for a, b in zip(net_h.get_weights(), net_d.get_weights()):
                print('weights', a.shape, float(np.max(np.abs(a - b))))
                assert np.max(np.abs(a - b)) <= bar(a)


def test_regularized_clipped_training_is_deterministic():
    from GNN import optimizers
    batch = _batch()
    runs = []
    for _ in range(2):
        m = _model(optimizers.Adam(0.01, clipnorm=0.05))
        for _ in range(3):
            m.training_step(batch, True)
        assert m.net_state._host_stale
        runs.append(m.net_state.get_weights() + m.net_output.get_weights())
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_off_means_off_and_bad_arguments_are_refused():
    from GNN import _engine, optimizers
    batch = _batch()
    runs = []
    for switch_off in (False, True):
        m = _model(optimizers.Adam(0.01), reg=False)
        dev_s, dev_o = m.net_state.device_mlp(m.device), m.net_output.device_mlp(m.device)
        loop = m._device_loop(batch.device_graph(m.device))
        assert not hasattr(dev_s, '_reg_set') and not hasattr(loop, '_clip_set')
        if switch_off:      # straight through the C ABI (the Python wrappers skip a call that changes nothing)
            lib = _engine.lib()
            assert lib.gnn_mlp_set_regularizers(dev_s._h, None, None) == 0 and lib.gnn_mlp_set_regularizers(dev_o._h, None, None) == 0
            assert lib.gnn_loop_set_clipping(loop._h, C.c_double(0), C.c_double(0), C.c_double(0)) == 0
        for _ in range(3):
            m.training_step(batch, True)
        assert not hasattr(dev_s, '_reg_set') and not hasattr(loop, '_clip_set')     # the plain model never reached the new entry points
        runs.append(m.net_state.get_weights() + m.net_output.get_weights())
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    lib = _engine.lib()
    bad = (C.c_double * 4)(0.0, -1e-3, 0.0, 0.0)
    zero = (C.c_double * 4)()
    assert lib.gnn_mlp_set_regularizers(dev_s._h, bad, zero) == -1 and lib.gnn_mlp_set_regularizers(dev_s._h, zero, bad) == -1
    assert lib.gnn_mlp_set_regularizers(dev_s._h, (C.c_double * 4)(0.0, float('nan'), 0.0, 0.0), zero) == -1
    assert lib.gnn_mlp_set_regularizers(dev_s._h, zero, None) == -1
    assert lib.gnn_loop_set_clipping(loop._h, C.c_double(0), C.c_double(1), C.c_double(1)) == -1
    assert lib.gnn_loop_set_clipping(loop._h, C.c_double(-1), C.c_double(0), C.c_double(0)) == -1
    assert lib.gnn_loop_set_clipping(loop._h, C.c_double(0), C.c_double(float('inf')), C.c_double(0)) == -1
    with pytest.raises(ValueError):
        dev_s.set_regularizers(([0.0, -1.0, 0.0, 0.0], [0.0] * 4))
    with pytest.raises(ValueError):
        loop.set_clipping(0.0, 1.0, 1.0)
    m.training_step(batch, True)                           # refused calls leave the settings as they were
