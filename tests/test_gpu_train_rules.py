"""The update rules (optimizer kinds 0 - 6), losses (loss kinds 3 - 6, label smoothing, Huber delta) and learning-rate schedules of the
device-side training step against their float64 statements: the host mirrors of GNN/optimizers.py (themselves checked in
tests/test_train_rules_host.py) and `loss64` of that file with the float64 training oracle around it.  Model and batch of the update
tests are those of tests/test_gpu_train_surface.py (449 gradient entries in net_state: two blocks, a partial last one, 3-entry arrays)."""
import ctypes as C

import numpy as np
import pytest

from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from test_gpu_train import _by_source_csr
from test_gpu_train_surface import _batch, _global_norm, _model, _scaled, _trainable
from test_train_rules_host import LOSS_KINDS, edge_rows, loss64, loss_inputs
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu


def _optimizer(name, **kw):
    from GNN import optimizers
    S = optimizers.schedules
    return {'sgd_nesterov': lambda: optimizers.SGD(0.01, momentum=0.9, nesterov=True, **kw),
            'amsgrad': lambda: optimizers.Adam(0.01, amsgrad=True, **kw),
            'rmsprop': lambda: optimizers.RMSprop(0.01, **kw),
            'rmsprop_momentum': lambda: optimizers.RMSprop(0.01, momentum=0.9, **kw),
            'rmsprop_centered': lambda: optimizers.RMSprop(0.01, centered=True, **kw),
            'rmsprop_centered_momentum': lambda: optimizers.RMSprop(0.01, momentum=0.9, centered=True, **kw),
            'adagrad': lambda: optimizers.Adagrad(0.01, **kw),
            'adamax': lambda: optimizers.Adamax(0.01, **kw),
            'adam_schedule': lambda: optimizers.Adam(S.ExponentialDecay(0.01, 2, 0.5, staircase=True), **kw)}[name]()


def _follow(m, mirror, batch, steps):
    """Every device step from the device's own weights and raw gradients: only the float32 roundings of the rule itself separate it from
    the float64 mirror (which keeps its own slots).  Bound per array: 1e-6 max(1, max |w|), as in
    test_clipping_is_the_float64_clip_of_the_raw_gradients."""
    for step in range(steps):
        before = _trainable(m)
        res = m.training_step(batch, True)
        assert m.net_state._host_stale and m.net_output._host_stale          # the step stayed on the device: nothing read back yet
        want = mirror.apply_gradients(zip(_scaled(res), before))
        after = _trainable(m)
        for w0, w1, ww in zip(before, after, want):
            err = float(np.max(np.abs(w1.astype(np.float64) - ww.astype(np.float64))))
            bound = 1e-6 * max(1.0, float(np.max(np.abs(w0))))
            print('step', step, w0.shape, 'moved', float(np.max(np.abs(ww - w0))), 'err', err, 'bound', bound)
            assert err <= bound
        assert any(np.max(np.abs(ww - w0)) > 1e-4 for w0, ww in zip(before, want))       # it did move


@pytest.mark.parametrize('name', ['sgd_nesterov', 'amsgrad', 'rmsprop', 'rmsprop_momentum', 'rmsprop_centered', 'rmsprop_centered_momentum', 'adagrad',
                                  'adamax', 'adam_schedule'])
def test_update_rule_follows_the_float64_mirror_step_by_step(name):
    m = _model(_optimizer(name), reg=False)
    _follow(m, _optimizer(name), _batch(), 4)
    assert m.optimizer.iterations == 4


def test_clipping_composes_with_centered_rmsprop():
    from GNN import optimizers
    batch = _batch()
    c = 0.5 * _global_norm(_scaled(_model(optimizers.SGD(0.0), reg=False).training_step(batch, True)))
    assert c > 0
    _follow(_model(_optimizer('rmsprop_centered', global_clipnorm=c), reg=False), _optimizer('rmsprop_centered', global_clipnorm=c), batch, 4)


@pytest.mark.parametrize('how', ['new optimizer object', 'same object, other kind'])
def test_slots_restart_from_zero(how):
    """A new optimizer object zeroes the device slots through gnn_mlp_reset_optimizer; a step of another kind on the same slots (here:
    the same Adam object switched to amsgrad, which also brings the third slot array in) restarts them inside the library."""
    from GNN import optimizers
    batch = _batch()
    if how == 'new optimizer object':
        m = _model(optimizers.Adagrad(0.01), reg=False)
        for _ in range(2): m.training_step(batch, True)
        m.optimizer = optimizers.RMSprop(0.01, momentum=0.9)
        mirror = optimizers.RMSprop(0.01, momentum=0.9)
    else:
        m = _model(optimizers.Adam(0.01), reg=False)
        for _ in range(2): m.training_step(batch, True)
        m.optimizer.amsgrad = True
        mirror = optimizers.Adam(0.01, amsgrad=True)
        mirror.iterations = 2                                    # the step counter goes on; the moments start again
    _follow(m, mirror, batch, 2)


LOSS_CASES = [('bce', 0.0, 8, False), ('bce_logits', 0.0, 0, True), ('mae', 0.0, 0, False), ('huber', 0.0, 8, False), ('cce', 0.1, 0, False),
              ('cce_logits', 0.1, 8, False), ('bce', 0.2, 0, False)]


@pytest.mark.parametrize('name,smoothing,d,graph_based', LOSS_CASES)
def test_new_losses_match_the_float64_oracle(name, smoothing, d, graph_based):
    """gnn_loop_train_step with the new loss kinds / parameters against oracle.gnn_train_oracle.train_forward, loss64, train_backward.
    Set-up of test_train_step_matches_oracle (Dropout with injected masks, BatchNormalization behind net_state) with T = 3; net_output
    has no BatchNormalization, so that the sigmoid / softmax values reach the loss as probabilities."""
    from GNN import _engine as e
    rng = np.random.default_rng(300 + LOSS_KINDS[name] + d)
    n, nl, al, max_it, T, delta = 500, 3, 2, 4, 3, 0.3
    arcs = random_arcs(rng, n, 1500, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if graph_based:
        ng = np.zeros((n, 3), np.float32); ng[:200, 0] = 1 / 200; ng[200:350, 1] = 1 / 150; ng[350:, 2] = 1 / 150
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    if not graph_based:
        g['set_mask'] = rng.random(n) < 0.8
    ds, nlc = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nlc), [16, ds], 'tanh', gain=0.8, bn_random=True)
    out_act = {'bce': 'sigmoid', 'cce': 'softmax'}.get(name, 'linear')
    ou = make_mlp(rng, ds + nlc, [9, T], 'tanh', batch_normalization=False, out_activation=out_act)
    st['dropout'], ou['dropout'] = {0: 0.2}, {0: 0.1, 1: 0.3}
    mask = g['set_mask'] & g['output_mask']
    m = int(mask.sum())
    in_s = st['weights'][0].shape[0]
    masks_s = [{0: (rng.random((n, in_s)) > 0.2)} for _ in range(max_it)]
    masks_o = {0: rng.random((m, ds + nlc)) > 0.1, 1: rng.random((m, 9)) > 0.3}
    n_t = 3 if graph_based else m
    if name in ('bce', 'bce_logits'): targets = rng.integers(0, 2, (n_t, T)).astype(np.float32)               # multi-hot
    elif name in ('cce', 'cce_logits'): targets = np.eye(T)[rng.integers(0, T, n_t)].astype(np.float32)
    else: targets = rng.uniform(-1, 1, (n_t, T)).astype(np.float32)
    weights = rng.uniform(0.5, 1.5, n_t).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None

    ctx = tro.train_forward(g, st, ou, d, max_it, 0.0, s0, masks_s, masks_o)
    out = ng.astype(np.float64).T @ ctx['out_nodes'] if graph_based else ctx['out_nodes']
    want_loss, d_out = loss64(name, targets, out, weights, smoothing, delta)
    want_s, want_o, _ = tro.train_backward(ctx, ng.astype(np.float64) @ d_out if graph_based else d_out)
    if name == 'huber':
        err = np.abs(out - targets)
        print('huber rows: quadratic', int((err <= delta).sum()), 'linear', int((err > delta).sum()))
        assert (err < delta).any() and (err > delta).any()

    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, d, max_it, 0.0)
    if d:
        loop.set_state0(s0)
    loop.set_loss_params(smoothing, delta)
    ms = np.concatenate([masks_s[k][0].astype(np.uint8).ravel() for k in range(max_it)])
    mo = np.concatenate([masks_o[0].astype(np.uint8).ravel(), masks_o[1].astype(np.uint8).ravel()])
    ng_csr = None
    if graph_based:
        cols, rows = np.nonzero(ng.T)
        ip = np.zeros(4, np.int32); np.cumsum(np.bincount(cols, minlength=3), out=ip[1:])
        ng_csr = (ip, rows.astype(np.int32), ng[rows, cols])
    step = lambda: loop.train_step(mst, mou, _by_source_csr(g, n), targets, weights, LOSS_KINDS[name], ng_csr, dropout_state=[0.2, 0, 0],
                                   dropout_output=[0.1, 0.3, 0], masks_state=ms, masks_output=mo, bn_state=np.concatenate(st['weights'][-4:-2]))
    res = step()
    print(name, 'k', res['k'], ctx['k'], 'loss', res['loss'], want_loss)
    assert res['k'] == ctx['k'] and 1 <= res['k'] <= max_it
    assert abs(res['loss'] - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    for got, want in list(zip(res['grads_state'], want_s)) + list(zip(res['grads_output'], want_o)):
        assert got.shape == want.shape
        print(got.shape, 'err', float(np.max(np.abs(got - want))), 'of', float(np.max(np.abs(want))))
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want)))
    assert any(np.max(np.abs(want)) > 1e-3 for want in want_s)
    again = step()
    assert again['loss'] == res['loss'] and again['k'] == res['k']
    for a_, b_ in zip(again['grads_state'] + again['grads_output'], res['grads_state'] + res['grads_output']):
        assert np.array_equal(a_, b_)


@pytest.mark.parametrize('name,smoothing', [('bce', 0.0), ('bce', 0.2), ('bce_logits', 0.0), ('bce_logits', 0.2), ('mae', 0.0), ('huber', 0.0),
                                            ('cce', 0.1), ('cce_logits', 0.1), ('cce', 0.0), ('mse', 0.0)])
def test_host_loss_helper_matches_the_float64_losses(name, smoothing):
    """gnn_loss_grad_ex (and gnn_loss_grad where the parameters are the defaults) on 64 rows plus the edge rows of the host tests: the
    helper works in double, so d_out agrees to 1e-6 absolutely (it is stored as float32) and the loss to 1e-9 relatively."""
    from GNN import _engine
    rng = np.random.default_rng(11)
    t, o = loss_inputs(name if name != 'mse' else 'mae', rng, 64)
    delta = 0.5                                                   # (the Huber edge rows sit at |e| == 0.5)
    if name in edge_rows():
        t, o = np.concatenate([t, edge_rows()[name][0]]), np.concatenate([o, edge_rows()[name][1]])
    w = rng.uniform(0.5, 1.5, len(t)).astype(np.float32)
    want_loss, want_d = loss64(name, t, o, w, smoothing, delta)
    loss, d = _engine.loss_grad(LOSS_KINDS[name], t, o, w, smoothing, delta)
    print(name, smoothing, 'loss', loss, want_loss, 'd_out err', float(np.max(np.abs(d - want_d))))
    assert abs(loss - want_loss) <= 1e-9 * abs(want_loss) and np.max(np.abs(d - want_d)) <= 1e-6
    if name in edge_rows():
        n_edge = len(edge_rows()[name][0])
        if name != 'huber': assert np.all(d[-n_edge:] == 0.0)
        else: assert np.array_equal(d[-1], (w[-1] * np.array([0.5, -0.5, 0.5]) / 3).astype(np.float32))
    if smoothing == 0.0:                                          # the plain entry point: the same with delta 1
        lib, fp = _engine.lib(), lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        d1, loss1 = np.zeros_like(o), C.c_double()
        assert lib.gnn_loss_grad(C.c_int(LOSS_KINDS[name]), C.c_int64(len(o)), C.c_int(3), fp(t), fp(o), fp(w), C.byref(loss1), fp(d1)) == 0
        want_loss, want_d = loss64(name, t, o, w, 0.0, 1.0)
        assert abs(loss1.value - want_loss) <= 1e-9 * abs(want_loss) and np.max(np.abs(d1 - want_d)) <= 1e-6


def test_sigmoid_model_trains_with_smoothed_bce_and_a_scheduled_rmsprop(tmp_path):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(0)
    set_seed(0)
    graphs = []
    for _ in range(6):
        n = 120
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        cls = (nodes[:, 0] + 0.5 * nodes[:, 1] > 0).astype(int)
        graphs.append(GraphObject(arcs=random_arcs(rng, n, 360, 1), nodes=nodes, targets=np.eye(2)[cls]))
    gTr, gVa = graphs[:4], GraphObject.merge(graphs[4:], problem_based='n', aggregation_mode='average')
    st = MLP(1 + 2 * 3, [8, 3], 'tanh', 'glorot_normal', 'zeros', dropout_rate=0.1, dropout_pos=0)
    ou = MLP(3, [2], 'sigmoid', 'glorot_normal', 'zeros', batch_normalization=False)
    sched = optimizers.schedules.InverseTimeDecay(0.02, 5, 0.5)
    gnn = GNNnodeBased(net_state=st, net_output=ou, optimizer=optimizers.RMSprop(sched), loss_function=losses.binary_crossentropy,
                       loss_arguments={'label_smoothing': 0.1}, state_vect_dim=0, max_iteration=4, threshold=0.01, addressed_problem='c',
                       path_writer=str(tmp_path / 'w'))
    first = GraphTensor.fromGraphObject(gTr[0])
    gnn.training_step(first, True)
    assert gnn._device_loop(first.device_graph(gnn.device))._loss_params_set == (0.1, 1.0)       # loss_arguments reached the device loss
    gnn.train(gTr, 30, gVa, update_freq=5, max_fails=50, verbose=0)
    h = gnn.history
    print('Loss Va', h['Loss Va'])
    assert h['Loss Va'][-1] < h['Loss Va'][0] and h['Loss Tr'][-1] < h['Loss Tr'][0]
    assert gnn.optimizer.iterations == 1 + 30 * len(gTr)                                         # the schedule's step count
    loss = gnn.test(gVa)['Loss']
    gnn.save(str(tmp_path / 'm'))
    back = GNNnodeBased.load(str(tmp_path / 'm'), path_writer=str(tmp_path / 'w2'))
    assert back.test(gVa)['Loss'] == loss
    assert back.loss_function is losses.binary_crossentropy and back.loss_args == {'label_smoothing': 0.1}
    assert type(back.optimizer) is optimizers.RMSprop and back.optimizer.get_config() == gnn.optimizer.get_config()
    assert type(back.optimizer.learning_rate) is type(sched) and [back.optimizer.learning_rate(s) for s in range(12)] == [sched(s) for s in range(12)]


@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_lgnn_joint_step_with_adamax_mae_and_a_global_norm(mode):
    """Two layers, one Adamax step over both with ONE global norm (gnn_loop_optimizer_step_scaled, kind 6) and the host helper's
    mean_absolute_error: device against host path, bars of test_gpu_train_surface.py:_same_training."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(2)
    n = 90
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    g = GraphObject(arcs=random_arcs(rng, n, 270, 1), nodes=nodes, targets=rng.uniform(-1, 1, (n, 2)))

    def build(device_optimizer, opt):
        set_seed(4)

        def model(layer):
            w = 3 + 2 * (layer > 0)
            st = MLP(1 + 2 * w, [8, w], 'tanh', 'glorot_normal', 'zeros')      # BatchNormalization on
            ou = MLP(w, [2], 'linear', 'glorot_normal', 'zeros', batch_normalization=False)
            return GNNnodeBased(net_state=st, net_output=ou, optimizer=None, loss_function=losses.mean_absolute_error, loss_arguments=None,
                                state_vect_dim=0, max_iteration=3, threshold=0.01, addressed_problem='r')

        lg = LGNN([model(0), model(1)], False, True, opt, losses.mean_absolute_error, None, 'r')
        lg.device_optimizer = device_optimizer
        lg.training_mode = mode
        return lg

    probe = build(False, optimizers.SGD(0.0)).training_step(g, True)
    c = 0.5 * _global_norm([np.asarray(a, np.float64) / k for gs, k in zip(probe['grads_state'], probe['k']) for a in gs]
                           + [np.asarray(a, np.float64) for go in probe['grads_output'] for a in go])
    assert c > 0
    host, dev = build(False, optimizers.Adamax(0.01, global_clipnorm=c)), build(True, optimizers.Adamax(0.01, global_clipnorm=c))
    for _ in range(3):
        rh, rd = host.training_step(g, True), dev.training_step(g, True)
        print('k', rh['k'], rd['k'], 'loss', rh['loss'], rd['loss'])
        assert rh['k'] == rd['k'] and abs(rh['loss'] - rd['loss']) <= 1e-4 * max(1.0, abs(rh['loss']))
    for gh, gd in zip(host.gnns, dev.gnns):
        assert gd.net_state._host_stale and gd.net_output._host_stale and not gh.net_state._host_stale
        for net_h, net_d in ((gh.net_state, gd.net_state), (gh.net_output, gd.net_output)):
            for a, b in zip(net_h.get_weights(), net_d.get_weights()):
                print('weights', a.shape, float(np.max(np.abs(a - b))))
                assert np.max(np.abs(a - b)) <= 5e-5 * max(1.0, np.max(np.abs(a)))


def test_bad_parameters_are_refused_and_change_nothing():
    from GNN import _engine, optimizers
    batch = _batch()
    runs = []
    for poke in (False, True):
        m = _model(optimizers.RMSprop(0.01), reg=False)
        loop = m._device_loop(batch.device_graph(m.device))
        lib = _engine.lib()
        for step in range(2):
            if poke:
                for bad in ((-0.1, 1.0), (0.0, 0.0), (1.5, 1.0), (float('nan'), 1.0), (0.0, float('inf'))):
                    assert lib.gnn_loop_set_loss_params(loop._h, C.c_double(bad[0]), C.c_double(bad[1])) == -1
                    with pytest.raises(ValueError):
                        loop.set_loss_params(*bad)
                for kind, hyper in ((7, [0.01, 0.9, 0.0, 1e-7]), (-1, [0.01, 0.9, 0.0, 1e-7]), (3, [0.01, 0.9, 0.0, -1e-7]), (3, [0.01, 0.9, -0.5, 1e-7]),
                                    (5, [0.01, -0.1, 1e-7, 0.0]), (6, [0.01, 0.9, 0.999, float('nan')]), (2, [0.01, 0.9, 0.999, float('inf')])):
                    with pytest.raises(ValueError):
                        loop.arm_optimizer(kind, hyper, True)
            res = m.training_step(batch, True)
        assert not hasattr(loop, '_loss_params_set')
        runs.append((res['loss'], m.net_state.get_weights() + m.net_output.get_weights()))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)
    # optimizer kind 7 and loss kind 7 through the entries that take them
    m = _model(optimizers.SGD(0.0), reg=False)
    m.device_optimizer = False
    m.training_step(batch, True)                                # host path: the loop keeps fresh, unapplied gradients
    loop = m._device_loop(batch.device_graph(m.device))
    for kind in (7, -1):
        with pytest.raises(ValueError):
            loop.optimizer_step(kind, [0.01, 0.9, 0.0, 1e-7])
        with pytest.raises(ValueError):
            loop.optimizer_step_scaled(kind, [0.01, 0.9, 0.0, 1e-7], 1.0, 0.5)
    with pytest.raises(ValueError):
        loop.optimizer_step(4, [0.01, 0.9, 0.0, float('nan')])
    loop.optimizer_step(4, [0.01, 0.9, 0.0, 1e-7])               # the refused calls did not use the gradients up
    t, o = loss_inputs('mae', np.random.default_rng(0), 4)
    for kind in (7, -1):
        with pytest.raises(ValueError):
            _engine.loss_grad(kind, t, o, np.ones(4, np.float32))
        with pytest.raises(ValueError):
            loop.train_step(m.net_state.device_mlp(m.device), m.net_output.device_mlp(m.device), None, np.zeros((loop.n_masked, 2), np.float32),
                            np.ones(loop.n_masked, np.float32), kind)
    for bad in ((-0.1, 1.0), (1.5, 1.0), (0.0, 0.0)):
        with pytest.raises(ValueError):
            _engine.loss_grad(5, t, o, np.ones(4, np.float32), *bad)
