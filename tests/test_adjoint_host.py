"""Gradient mode 1 ("fixed point") without a device: the host predicate gnn_adjoint_form at both neighbours of every limit it has, the float64
mirror of the mode's semantics (tests/adjoint_mirror.py) against a dense solve of (I - J^T) z = g, and the Python surface that needs no GPU
(validation, copy / save / load, the LGNN modes that refuse)."""
import numpy as np
import pytest

import adjoint_mirror as am
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs


def _form(dims, act='tanh', n_rows=100, rates=None, bn=False):
    from GNN import _engine as e
    return e.adjoint_form(dims, [act] * (len(dims) - 1), n_rows, rates, bn)


def test_refused_nets_name_the_reason():
    assert _form((11, 8, 4)) == dict(eligible=True, reason=None, gather='narrow', backward=['adjoint_narrow'] * 2, narrow_refusal=None)
    assert _form((11, 8, 4), bn=True)['eligible'] is False and _form((11, 8, 4), bn=True)['reason'] == 'batch_normalization'
    for pos in range(3):                      # in front of either Dense layer, and behind the last one
        rates = [0.0, 0.0, 0.0]
        rates[pos] = 0.1
        f = _form((11, 8, 4), rates=rates)
        assert f['eligible'] is False and f['reason'] == 'dropout', pos
    assert _form((11, 8, 4), rates=[0.0, -0.2, 0.0])['reason'] == 'dropout'        # AlphaDropout
    assert _form((11, 8, 4), rates=[0.1, 0, 0], bn=True)['reason'] == 'batch_normalization'


@pytest.mark.parametrize('ds,gather', [(1, 'generic'), (3, 'generic'), (4, 'rows'), (8, 'rows'), (60, 'rows'), (62, 'generic'), (64, 'rows'),
                                        (65, 'generic'), (68, 'generic')])
def test_gather_form_follows_the_state_width(ds, gather):
    """16-byte pieces need Ds % 4 == 0, 16 lanes of them cover Ds <= 64 (state_rows16 without its row count, which does not enter); where the
    one-launch iteration applies - few rows, a concat of at most 96 columns - the gather is inside it."""
    assert _form((2 * ds + 3, 16, ds), n_rows=4096)['gather'] == gather
    for n in (1, 4095):
        f = _form((2 * ds + 3, 16, ds), n_rows=n)
        narrow = 2 * ds + 3 <= 96 and ds <= 64
        assert f['gather'] == ('narrow' if narrow else gather) and (f['narrow_refusal'] is None) == narrow, (n, f)


def test_narrow_form_at_both_neighbours_of_every_limit():
    """The one-launch adjoint iteration: 1 - 3 Dense layers, every width <= 64, concat <= 96, fewer than 4,096 rows (and at least one), no softmax."""
    taken = dict(eligible=True, reason=None, gather='narrow', narrow_refusal=None)
    def check(dims, n, why, act='tanh', **kw):
        f = _form(dims, act, n, **kw)
        if why is None: assert f == dict(taken, backward=['adjoint_narrow'] * (len(dims) - 1)), (dims, n, f)
        else: assert f['narrow_refusal'] == why and 'adjoint_narrow' not in f['backward'] and f['gather'] != 'narrow', (dims, n, f)
    check((96, 64, 64, 32), 100, None); check((96, 64, 65, 32), 100, 'width'); check((96, 65, 64, 32), 100, 'width')      # width 64 | 65
    check((89, 40), 100, None); check((96, 64), 100, None); check((131, 65), 100, 'width')
    check((96, 20, 8), 100, None); check((97, 20, 8), 100, 'concat')                                                       # concat 96 | 97
    check((31, 32, 32, 14), 4095, None); check((31, 32, 32, 14), 4096, 'rows'); check((31, 32, 32, 14), 1, None); check((31, 32, 32, 14), 0, 'rows')
    check((31, 14), 935, None); check((31, 32, 14), 935, None); check((31, 32, 32, 14), 935, None); check((31, 32, 32, 32, 14), 935, 'layers')
    for act in ('linear', 'relu', 'selu', 'elu', 'sigmoid'): check((31, 32, 14), 935, None, act)
    check((31, 32, 14), 935, 'softmax', 'softmax')
    # a refused net is refused whatever its shape; the narrow form is then beside the point but still reported
    assert _form((31, 32, 14), n_rows=935, bn=True)['eligible'] is False and _form((31, 32, 14), n_rows=935, rates=[0, 0.1, 0])['reason'] == 'dropout'


def test_backward_forms_at_the_row_threshold():
    """4,095 | 4,096 rows: below, the row blocks of k_layer_bwd; from there on the forms of the training step's backward pass - the three-layer
    chain (which leaves the aligned rows the gather reads), the wide product per layer, or a mix."""
    wide3 = (135, 128, 128, 64)
    assert _form(wide3, n_rows=4095) == dict(eligible=True, reason=None, gather='rows', backward=['per_op'] * 3, narrow_refusal='width')
    assert _form(wide3, n_rows=4096) == dict(eligible=True, reason=None, gather='rows_aligned', backward=['chain3'] * 3, narrow_refusal='width')
    assert _form((135, 144, 64), n_rows=4095)['backward'] == ['per_op', 'per_op']
    f = _form((135, 144, 64), n_rows=4096)
    assert f['backward'] == ['wide', 'wide'] and f['gather'] == 'rows'
    assert _form((135, 128, 32, 64), n_rows=4096)['backward'] == ['wide', 'per_op', 'per_op']
    assert _form(wide3, n_rows=0)['backward'] == ['per_op'] * 3
    # the forms are those gnn_train_forms reports for the same net: one decision
    from GNN import _engine as e
    for dims in (wide3, (135, 144, 64), (135, 128, 32, 64), (135, 68, 72, 36)):
        for n in (4095, 4096):
            assert _form(dims, n_rows=n)['backward'] == e.train_forms(dims, ['tanh'] * (len(dims) - 1), None, n)['backward'], (dims, n)


def _small_problem(seed=3, n=12, ds=3, nl=2, al=1, act='tanh', gain=0.5):
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 2 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.7
    st = make_mlp(rng, al + 2 * (ds + nl), [7, ds], act, gain=gain, batch_normalization=False)
    ou = make_mlp(rng, ds + nl, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    targets = np.eye(2)[rng.integers(0, 2, m)]
    weights = rng.uniform(0.5, 1.5, m)
    s0 = 0.1 * rng.standard_normal((n, ds))
    return g, st, ou, ds, s0, targets, weights


def test_mirror_solves_the_adjoint_system():
    """z of the mirror = the solution of (I - J^T) z = g with J^T assembled column by column, to 1e-10; and the weight gradients are those of the
    recorded body for that z."""
    g, st, ou, ds, s0, targets, weights = _small_problem()
    n = s0.shape[0]
    r = am.step(g, st, ou, ds, 200, 1e-13, s0, {}, targets, weights, adjoint_max_iter=2000, adjoint_threshold=1e-15)
    assert r['adjoint_converged'] and 3 < r['adjoint_iterations'] < 2000 and 3 < r['k'] < 200
    ctx = r['ctx']
    jt = np.zeros((n * ds, n * ds))
    for i in range(n * ds):
        e = np.zeros(n * ds); e[i] = 1.0
        jt[:, i] = am.jt(ctx, e.reshape(n, ds))[0].ravel()
    assert np.max(np.abs(np.linalg.eigvals(jt))) < 1.0                    # a contraction: the sum converges
    z = np.linalg.solve(np.eye(n * ds) - jt, r['g'].ravel()).reshape(n, ds)
    assert np.abs(r['g']).max() > 0 and (np.abs(r['g']).max(axis=1) == 0).any()      # rows outside the mask carry no g ...
    assert np.abs(z[np.abs(r['g']).max(axis=1) == 0]).max() > 0                      # ... but receive z through their arcs
    assert np.max(np.abs(r['z'] - z)) <= 1e-10 * np.max(np.abs(z))
    want = am.jt(ctx, z)[1]
    for a, b in zip(r['grads_state'], want):
        assert np.max(np.abs(a - b)) <= 1e-10 * max(1.0, np.max(np.abs(b)))


def test_mirror_is_the_unrolled_gradient_in_the_limit():
    """At a fixed point the unrolled gradient over k bodies is the adjoint sum truncated at k - 1 iterations: with the state started AT the fixed
    point (every body is the recorded body) the oracle's train_backward over k bodies and the mirror with k - 1 forced iterations agree."""
    from oracle import gnn_train_oracle as tro
    g, st, ou, ds, s0, targets, weights = _small_problem(seed=5)
    p = am.forward(g, st, ou, ds, 500, 1e-15, s0, {})['state']
    k = 6
    un = tro.train_step(g, st, ou, ds, k, -1.0, p, [{}] * k, {}, targets, weights, mean=False)
    fp = am.step(g, st, ou, ds, 1, -1.0, p, {}, targets, weights, k_forced=1, iterations_forced=k - 1)
    assert un['k'] == k
    # sum over the k bodies of (dF/dw)^T (J^T)^j g, j = 0 .. k - 1, against (dF/dw)^T z_{k-1}: the same sum, since every body sits at p
    for a, b in zip(un['grads_state'], fp['grads_state']):
        assert np.max(np.abs(a - b)) <= 1e-9 * max(1.0, np.max(np.abs(b)))


def test_truncation_and_forced_counts():
    g, st, ou, ds, s0, targets, weights = _small_problem(gain=3.0)          # not a contraction
    r = am.step(g, st, ou, ds, 5, 1e-3, s0, {}, targets, weights, adjoint_max_iter=7)
    assert r['adjoint_iterations'] == 7 and not r['adjoint_converged'] and r['k'] == 5
    r0 = am.step(g, st, ou, ds, 5, 1e-3, s0, {}, targets, weights, iterations_forced=0)
    assert r0['adjoint_iterations'] == 0 and np.array_equal(r0['z'], r0['g'])


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------------
def _model(cls=None, dropout=0.0, bn=False, layer=0):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (3 + extra), [8, 3 + extra], 'tanh', 'glorot_normal', 'zeros', dropout_rate=dropout, dropout_pos=0, batch_normalization=bn)
    ou = MLP(3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=0, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_set_gradient_mode_validates_and_refuses():
    gnn = _model()
    assert gnn.gradient_mode == 'unrolled'
    gnn.set_gradient_mode('fixed_point', max_iteration=30, threshold=1e-4)
    assert (gnn.gradient_mode, gnn.adjoint_max_iteration, gnn.adjoint_threshold) == ('fixed_point', 30, 1e-4)
    with pytest.raises(ValueError): gnn.set_gradient_mode('implicit')
    with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', max_iteration=0)
    with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', threshold=-1.0)
    assert gnn.gradient_mode == 'fixed_point'                              # a refused call leaves the setting
    for bad in (_model(dropout=0.1), _model(bn=True)):
        with pytest.raises(NotImplementedError): bad.set_gradient_mode('fixed_point')
        bad.set_gradient_mode('unrolled')
        assert bad.gradient_mode == 'unrolled'


def test_copy_save_load_keep_the_mode(tmp_path):
    import json
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    for cls in (None, GNNgraphBased, GNNedgeBased):
        gnn = _model(cls)
        gnn.set_gradient_mode('fixed_point', 25, 1e-3)
        twin = gnn.copy(copy_weights=False)
        assert type(twin) is type(gnn) and twin._gradient_config() == gnn._gradient_config() == dict(mode='fixed_point', max_iteration=25, threshold=1e-3)
    path = str(tmp_path / 'model')
    gnn.save(path)
    assert type(gnn).load(path)._gradient_config() == gnn._gradient_config()
    with open(f'{path}/config.json') as f: config = json.load(f)
    del config['gradient_mode']                                            # a model saved before the mode existed
    with open(f'{path}/config.json', 'w') as f: json.dump(config, f)
    assert type(gnn).load(path).gradient_mode == 'unrolled'
    assert _model().copy().gradient_mode == 'unrolled'


def test_lgnn_forwards_the_mode_and_refuses_the_joint_steps(tmp_path):
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    lgnn = LGNN([_model(), _model(layer=1)], get_state=False, get_output=True, optimizer=optimizers.Adam(0.02),
                loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    lgnn.set_gradient_mode('fixed_point', 20)
    assert [g.gradient_mode for g in lgnn.gnns] == ['fixed_point'] * 2 and lgnn.gnns[1].adjoint_max_iteration == 20
    assert [g.gradient_mode for g in lgnn.copy().gnns] == ['fixed_point'] * 2
    lgnn.save(str(tmp_path / 'stack'))
    assert [g.gradient_mode for g in LGNN.load(str(tmp_path / 'stack')).gnns] == ['fixed_point'] * 2
    for mode in ('parallel', 'residual'):
        lgnn.training_mode = mode
        with pytest.raises(NotImplementedError, match='fixed_point'): lgnn.training_step(None, mean=True)
    lgnn.gnns[0].set_gradient_mode('unrolled')                             # any layer in the mode is enough
    with pytest.raises(NotImplementedError): lgnn.training_step(None, mean=True)
