"""The fixed-point gradient for a net_state that ends in BatchNormalization on its moving statistics ("frozen": gnn_loop_set_gradient_mode_ex with
GNN_ADJOINT_FROZEN_BN), without a device: the float64 mirror of its semantics (tests/adjoint_bn_mirror.py) against a dense solve of
(I - J^T) z = g with J assembled from the layers' own formulas, against central finite differences of the loss through the inference oracle's
Loop - the independent witness that frozen BatchNormalization is the map the Loop iterates - the convergence of the mirror on every case of the
GPU tests (tests/adjoint_bn_cases.py), the host predicate with the flag on and off, and the Python surface that needs no GPU."""
import json

import numpy as np
import pytest

import adjoint_bn_cases as C
import adjoint_bn_mirror as bm
import adjoint_mirror as am
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs


def _small_problem(seed=3, n=12, ds=3, nl=2, al=1, hidden=(7,), gain=0.4):
    """float64 inputs; net_output without BatchNormalization and Dropout (its training-mode forward is its inference forward)"""
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 2 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.7
    g['set_mask'][0] = True
    st = C.frozen_net(rng, al + 2 * (ds + nl), list(hidden) + [ds], 'tanh', gain)
    st['weights'] = [np.asarray(w, np.float64) for w in st['weights']]
    ou = make_mlp(rng, ds + nl, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    targets = np.eye(2)[rng.integers(0, 2, m)]
    weights = rng.uniform(0.5, 1.5, m)
    s0 = 0.1 * rng.standard_normal((n, ds))
    return g, st, ou, ds, s0, targets, weights


def test_mirror_solves_the_adjoint_system_with_the_column_scale():
    """z of the mirror = the solution of (I - J^T) z = g, to 1e-10.  J is assembled here from the layers' formulas, not from the mirror's backward
    pass: per row the product of diag(act'(z_l)) W_l^T over the Dense layers, scaled per OUTPUT column by s_j = gamma_j / sqrt(var_j + eps), over the
    own-state columns and, through the adjacency, the aggregated-state columns.  The gamma / beta gradients are sum z xhat and sum z with xhat
    from the moving statistics."""
    g, st, ou, ds, s0, targets, weights = _small_problem()
    n = s0.shape[0]
    r = bm.step(g, st, ou, ds, 500, 1e-14, s0, {}, targets, weights, adjoint_max_iter=5000, adjoint_threshold=1e-15)
    assert r['adjoint_converged'] and 3 < r['adjoint_iterations'] < 5000 and 3 < r['k'] < 500
    p = r['state']
    L = len(st['activations'])
    gamma, beta, mean, var = st['weights'][2 * L:2 * L + 4]
    s = gamma / np.sqrt(var + orc.BN_EPS)
    assert np.abs(mean).min() > 0.05 and (s < 0).any() and np.abs(np.abs(s) - 1).max() > 0.3          # a scale that shows
    inp, c_aggs = bm.body_input(g, p, ds, np.float64)
    indptr, src, w = g['adjT']
    A = np.zeros((n, n))
    for row in range(n):
        for e in range(indptr[row], indptr[row + 1]): A[row, src[e]] += w[e]
    J = np.zeros((n, ds, n, ds))
    h_all = np.zeros((n, ds))
    for row in range(n):
        x, Jr = inp[row], np.eye(inp.shape[1])
        for l in range(L):
            a = np.tanh(x @ st['weights'][2 * l] + st['weights'][2 * l + 1])
            Jr = ((1 - a * a)[:, None] * st['weights'][2 * l].T) @ Jr
            x = a
        h_all[row] = x
        Jr = s[:, None] * Jr
        J[row, :, row, :] += Jr[:, :ds]
        for q in range(n): J[row, :, q, :] += A[row, q] * Jr[:, c_aggs:c_aggs + ds]
    # the recorded body's output is the next state of the Loop: the same map (p is its fixed point)
    y = gamma * ((h_all - mean) / np.sqrt(var + orc.BN_EPS)) + beta
    assert np.max(np.abs(y - p)) <= 1e-12 and np.max(np.abs(r['ctx']['body_out'] - y)) <= 1e-14
    Jm = J.reshape(n * ds, n * ds)
    assert np.max(np.abs(np.linalg.eigvals(Jm))) < 1.0
    z = np.linalg.solve(np.eye(n * ds) - Jm.T, r['g'].ravel()).reshape(n, ds)
    assert np.abs(z[np.abs(r['g']).max(axis=1) == 0]).max() > 0            # rows outside the mask receive z through their arcs
    assert np.max(np.abs(r['z'] - z)) <= 1e-10 * np.max(np.abs(z))
    xhat = (h_all - mean) / np.sqrt(var + orc.BN_EPS)
    assert np.max(np.abs(r['grads_state'][2 * L] - np.sum(z * xhat, axis=0))) <= 1e-10 and np.max(np.abs(r['grads_state'][2 * L + 1] - z.sum(axis=0))) <= 1e-10
    # without the scale (or with it twice) z is another vector: percents of its largest entry (J^T z is a fraction of z = g + J^T z), eight orders above the criterion
    for power in (0, 2):
        wrong = np.linalg.solve(np.eye(n * ds) - ((s ** (power - 1))[None, :, None, None] * J).reshape(n * ds, n * ds).T, r['g'].ravel()).reshape(n, ds)
        assert np.max(np.abs(wrong - z)) > 0.01 * np.max(np.abs(z))


def _loss_through_the_inference_loop(g, st, ou, ds, s0, targets, weights):
    k, _, out = orc.loop_node(g, st, ou, ds, 5000, 1e-12, s0, dtype=np.float64)
    assert 3 < k < 5000
    return tro.loss_forward_backward('categorical_crossentropy', targets, out, weights)[0]


def test_mirror_against_finite_differences_through_the_inference_loop():
    """Central differences, in float64, of the loss through the INFERENCE oracle's Loop (oracle/gnn_oracle.py: loop_node, moving statistics folded
    into scale and shift, run to threshold 1e-12) for entries of every W, b, gamma and beta of net_state, against the mirror's gradients.

    Tolerance, from the finite-difference step's own error: with h = 2e-4 the difference between the quotients at h and at h / 2 is three times the
    truncation error of the one at h / 2 (central differences: error ~ h^2); measured here, its largest value over the 30 entries is 1.7e-9.  To
    that the rounding of the quotient is added: the Loop stops when no node moves by more than 1e-12 of its norm (< 1), and it contracts by more
    than a half per body, so each state row is within 1e-12 of the fixed point and the loss within 1e-12 sum |d loss / d p| < 3e-12 (asserted);
    two such evaluations over 2 (h / 2) = 2e-4 give 3e-8.  An entry passes within |q(h) - q(h / 2)| + 3e-8 of q(h / 2).  Measured: the largest
    distance is 5.4e-10 (a third of the step difference, as the h^2 law says), the gradients are up to 0.31 in size, so a missing or doubled
    column scale - a factor between 0.25 and 3 on parts of the sum - is six orders above the bound."""
    g, st, ou, ds, s0, targets, weights = _small_problem(seed=7, n=10, hidden=(5,))
    r = bm.step(g, st, ou, ds, 5000, 1e-12, s0, {}, targets, weights, adjoint_max_iter=5000, adjoint_threshold=1e-14)
    assert r['adjoint_converged'] and r['k'] > 3 and np.abs(r['g']).sum() < 3.0 and np.abs(r['state']).max() < 1.0
    assert abs(r['loss'] - _loss_through_the_inference_loop(g, st, ou, ds, s0, targets, weights)) <= 1e-12
    rng = np.random.default_rng(1)
    L = len(st['activations'])
    h = 2e-4
    worst_step, worst, top = 0.0, 0.0, 0.0
    for ai in range(2 * L + 2):                              # every W, b, then gamma and beta
        arr = st['weights'][ai]
        for _ in range(5):
            idx = tuple(int(rng.integers(0, d)) for d in arr.shape)
            q = []
            for step in (h, h / 2):
                vals = []
                for sign in (1.0, -1.0):
                    net = dict(st, weights=[w.copy() for w in st['weights']])
                    net['weights'][ai][idx] += sign * step
                    vals.append(_loss_through_the_inference_loop(g, net, ou, ds, s0, targets, weights))
                q.append((vals[0] - vals[1]) / (2 * step))
            got = r['grads_state'][ai][idx]
            print(f'array {ai} {idx}: mirror {got:+.10e}  fd(h/2) {q[1]:+.10e}  |fd(h) - fd(h/2)| {abs(q[0] - q[1]):.2e}  distance {abs(got - q[1]):.2e}')
            worst_step, worst, top = max(worst_step, abs(q[0] - q[1])), max(worst, abs(got - q[1])), max(top, abs(got))
            assert abs(got - q[1]) <= abs(q[0] - q[1]) + 3e-8, (ai, idx, got, q)
    print(f'largest |fd(h) - fd(h/2)| {worst_step:.2e}, largest distance {worst:.2e}, largest gradient {top:.2e}')
    assert top > 0.1


def test_mirror_without_batch_normalization_is_the_plain_mirror():
    g, st, ou, ds, s0, targets, weights = _small_problem(seed=9)
    L = len(st['activations'])
    plain = dict(st, weights=st['weights'][:2 * L], batch_normalization=False)
    a = bm.step(g, plain, ou, ds, 50, 1e-6, s0, {}, targets, weights)
    b = am.step(g, plain, ou, ds, 50, 1e-6, s0, {}, targets, weights)
    assert a['k'] == b['k'] and a['adjoint_iterations'] == b['adjoint_iterations'] and np.array_equal(a['z'], b['z'])
    assert all(np.array_equal(x, y) for x, y in zip(a['grads_state'], b['grads_state']))


@pytest.mark.parametrize('case', C.NARROW, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_the_mirror_converges_on_every_small_case(case):
    """What tests/adjoint_bn_cases.py promises for the GPU tests: with its weight gain the Loop and the adjoint iteration of the mirror converge
    (thresholds 1e-2 and 1e-6), after at least three iterations, and the BatchNormalization arrays are in the ranges it names."""
    pb = C.narrow_problem(case)
    L = len(pb['st']['activations'])
    gamma, beta, mean, var = pb['st']['weights'][2 * L:2 * L + 4]
    assert (0.5 <= np.abs(gamma)).all() and (np.abs(gamma) <= 1.5).all() and (np.abs(beta) >= 0.1).all() and (np.abs(mean) >= 0.1).all()
    assert (0.25 <= var).all() and (var <= 4.0).all()
    for thr in (1e-2, 1e-6):
        r = bm.step(pb['g'], pb['st'], pb['ou'], pb['D'], 200, thr, pb['s0'], {}, pb['targets'], pb['weights'])
        assert r['adjoint_converged'] and 3 <= r['adjoint_iterations'] < 200 and 2 <= r['k'] < 200, (thr, r['k'], r['adjoint_iterations'])
    assert (np.abs(r['g']).max(axis=1) == 0).any() and np.abs(r['z']).max() > 0
    # a missing column scale would show: a scale away from 1, gamma and beta gradients well above the noise
    s = gamma / np.sqrt(var + orc.BN_EPS)
    assert np.abs(np.abs(s) - 1).max() > 0.2 and np.abs(r['grads_state'][2 * L]).max() > 1e-3 and np.abs(r['grads_state'][2 * L + 1]).max() > 1e-3


# ---- the host predicate ---------------------------------------------------------------------------------------------------------------------------
def _form(dims, n_rows=100, rates=None, bn=True, frozen_bn=None, act='tanh'):
    from GNN import _engine as e
    return e.adjoint_form(dims, [act] * (len(dims) - 1), n_rows, rates, bn, frozen_bn=frozen_bn)


def test_form_report_with_the_flag_on_and_off():
    off, on = _form((11, 8, 4)), _form((11, 8, 4), frozen_bn='frozen')
    assert off['eligible'] is False and off['reason'] == 'batch_normalization'
    assert on == dict(eligible=True, reason=None, gather='narrow', backward=['adjoint_narrow'] * 2, narrow_refusal=None)
    # the forms are those of the Dense chain: the same report as for the net without BatchNormalization, at every regime
    for dims, n in (((11, 8, 4), 100), ((97, 30, 12), 50), ((135, 128, 128, 64), 4095), ((135, 128, 128, 64), 4096), ((135, 144, 64), 4113), ((31, 32, 14), 0)):
        assert _form(dims, n, frozen_bn='frozen') == _form(dims, n, bn=False) == _form(dims, n, bn=False, frozen_bn='frozen'), (dims, n)
    assert _form((135, 128, 128, 64), 4096, frozen_bn='frozen')['backward'] == ['chain3'] * 3
    # Dropout stays refused with the flag; the flag changes nothing for a net without BatchNormalization
    assert _form((11, 8, 4), rates=[0.0, 0.1, 0.0], frozen_bn='frozen')['reason'] == 'dropout'
    assert _form((11, 8, 4), rates=[0.0, 0.0, 0.2], frozen_bn='frozen')['eligible'] is False
    with pytest.raises(ValueError): _form((11, 8, 4), frozen_bn='batch')
    from GNN import _engine as e
    assert {'gnn_loop_set_gradient_mode_ex', 'gnn_adjoint_form_ex'} <= set(e.EXPORTS) and e.ADJOINT_FROZEN_BN == 1


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------------------
def _model(cls=None, dropout=0.0, bn=True, layer=0):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (3 + extra), [8, 3 + extra], 'tanh', 'glorot_normal', 'zeros', dropout_rate=dropout, dropout_pos=0, batch_normalization=bn)
    ou = MLP(3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=0, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_keyword_validates_and_the_refusals_stay():
    gnn = _model()
    with pytest.raises(NotImplementedError): gnn.set_gradient_mode('fixed_point')                    # as before
    with pytest.raises(NotImplementedError): gnn.set_gradient_mode('fixed_point', batch_normalization=None)
    with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', batch_normalization='batch')
    with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', batch_normalization=True)
    with pytest.raises(TypeError): gnn.set_gradient_mode('fixed_point', None, None, 'frozen')        # keyword only
    assert gnn.gradient_mode == 'unrolled' and gnn.adjoint_batch_normalization is None
    gnn.set_gradient_mode('fixed_point', 30, 1e-4, batch_normalization='frozen')
    assert (gnn.gradient_mode, gnn.adjoint_max_iteration, gnn.adjoint_threshold, gnn.adjoint_batch_normalization) == ('fixed_point', 30, 1e-4, 'frozen')
    with pytest.raises(NotImplementedError): gnn.set_gradient_mode('fixed_point')                    # a later call without the keyword is refused again ...
    assert gnn.adjoint_batch_normalization == 'frozen'                                              # ... and leaves the setting
    with pytest.raises(NotImplementedError, match='Dropout'): _model(dropout=0.1).set_gradient_mode('fixed_point', batch_normalization='frozen')
    with pytest.raises(NotImplementedError): _model(dropout=0.1, bn=False).set_gradient_mode('fixed_point', batch_normalization='frozen')
    free = _model(bn=False)                                   # a net without BatchNormalization takes the keyword: nothing to freeze
    free.set_gradient_mode('fixed_point', batch_normalization='frozen')
    assert free._gradient_config()['batch_normalization'] == 'frozen'


def test_copy_save_load_and_lko_keep_the_keyword(tmp_path):
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    want = dict(mode='fixed_point', max_iteration=25, threshold=1e-3, batch_normalization='frozen')
    for cls in (None, GNNgraphBased, GNNedgeBased):
        gnn = _model(cls)
        gnn.set_gradient_mode('fixed_point', 25, 1e-3, batch_normalization='frozen')
        twin = gnn.copy(copy_weights=False)                  # (what LKO builds its folds' models with)
        assert type(twin) is type(gnn) and twin._gradient_config() == gnn._gradient_config() == want
        path = str(tmp_path / f'model{cls.__name__ if cls else ""}')
        gnn.save(path)
        loaded = type(gnn).load(path)
        assert loaded._gradient_config() == want and loaded.net_state.batch_normalization
        with open(f'{path}/config.json') as f: assert json.load(f)['gradient_mode'] == want


def test_lko_models_keep_the_keyword():
    """LKO trains copies of the model: they are in the frozen mode (copy() is what it calls; the call is checked here without a device)."""
    import inspect
    from GNN import GNN_BaseClass
    assert '.copy(' in inspect.getsource(GNN_BaseClass.BaseClass.LKO)
    gnn = _model()
    gnn.set_gradient_mode('fixed_point', batch_normalization='frozen')
    assert gnn.copy().adjoint_batch_normalization == 'frozen' and gnn.copy()._frozen_state_bn()


def test_a_config_without_the_keyword_is_what_it_was(tmp_path):
    """The key is written only when set: the saved file and _gradient_config() of a model without it are byte for byte those of the parent commit."""
    for bn, mode, text in ((False, ('fixed_point', 25, 1e-3), '"gradient_mode": {"mode": "fixed_point", "max_iteration": 25, "threshold": 0.001}, "label_projection"'),
                           (True, ('unrolled',), '"gradient_mode": {"mode": "unrolled", "max_iteration": null, "threshold": null}, "label_projection"')):
        gnn = _model(bn=bn)
        gnn.set_gradient_mode(*mode)
        assert list(gnn._gradient_config()) == ['mode', 'max_iteration', 'threshold']
        path = str(tmp_path / f'plain{int(bn)}')
        gnn.save(path)
        with open(f'{path}/config.json') as f: raw = f.read()
        assert text in raw and 'batch_normalization' not in raw
        assert type(gnn).load(path)._gradient_config() == gnn._gradient_config() and type(gnn).load(path).adjoint_batch_normalization is None


def test_lgnn_forwards_the_keyword(tmp_path):
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    lgnn = LGNN([_model(), _model(layer=1)], get_state=False, get_output=True, optimizer=optimizers.Adam(0.02),
                loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    with pytest.raises(NotImplementedError): lgnn.set_gradient_mode('fixed_point', 20)
    lgnn.set_gradient_mode('fixed_point', 20, batch_normalization='frozen')
    assert [(g.gradient_mode, g.adjoint_batch_normalization, g.adjoint_max_iteration) for g in lgnn.gnns] == [('fixed_point', 'frozen', 20)] * 2
    assert [g.adjoint_batch_normalization for g in lgnn.copy().gnns] == ['frozen'] * 2
    lgnn.save(str(tmp_path / 'stack'))
    assert [g._gradient_config().get('batch_normalization') for g in LGNN.load(str(tmp_path / 'stack')).gnns] == ['frozen'] * 2
    for mode in ('parallel', 'residual'):                     # the joint steps stay refused
        lgnn.training_mode = mode
        with pytest.raises(NotImplementedError, match='fixed_point'): lgnn.training_step(None, mean=True)
