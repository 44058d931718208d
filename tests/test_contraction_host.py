"""The contraction estimate (include/gnn_hip.h: gnn_loop_contraction_estimate) without a device: its float64 mirror (tests/contraction_mirror.py)
against NumPy power iteration on the dense J^T, the convergence of the late entries to the spectral radius, and the Python surface that needs no GPU
(the exported symbols, the methods, the argument refusals of the model method)."""
import numpy as np
import pytest

import contraction_mirror as cm
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs


def _small_problem(seed=3, n=12, ds=3, nl=2, al=1, act='tanh', gain=0.5):
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 2 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.7
    st = make_mlp(rng, al + 2 * (ds + nl), [7, ds], act, gain=gain, batch_normalization=False)
    ou = make_mlp(rng, ds + nl, [2], 'softmax', batch_normalization=False)
    p = 0.1 * rng.standard_normal((n, ds))
    v0 = rng.standard_normal((n, ds))
    return g, st, ou, ds, p, v0


@pytest.mark.parametrize('act,gain', [('tanh', 0.5), ('selu', 2.0)])
def test_mirror_is_power_iteration_on_the_dense_jt(act, gain):
    g, st, ou, ds, p, v0 = _small_problem(act=act, gain=gain)
    ctx = cm.context(g, st, ou, ds, p)
    growth, done, w = cm.power(ctx, v0, 12)
    a = cm.dense_jt(ctx)
    v = v0.ravel() / np.linalg.norm(v0)
    want = np.zeros(12)
    for t in range(12):                       # plain NumPy: normalise, multiply, measure
        u = a @ v
        want[t] = np.linalg.norm(u)
        v = u / want[t]
    assert done == 12 and np.all(want > 0)
    assert np.max(np.abs(growth - want)) <= 1e-10 * np.max(want)
    assert np.max(np.abs(w / np.linalg.norm(w) - v.reshape(w.shape))) <= 1e-10
    dense = cm.power_dense(a, v0, 12)
    assert np.max(np.abs(dense[0] - want)) <= 1e-10 * np.max(want) and dense[1] == 12


def test_late_entries_approach_the_spectral_radius():
    """A J^T with a real dominant eigenvalue and a gap (0.9 against 0.45 at most): after 60 iterations the ratio (0.5)^60 is gone."""
    rng = np.random.default_rng(7)
    n = 30
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    eig = np.concatenate([[0.9], rng.uniform(-0.45, 0.45, n - 1)])
    a = q @ np.diag(eig) @ q.T
    growth, done, _ = cm.power_dense(a, rng.standard_normal(n), 60)
    assert done == 60 and abs(np.max(np.abs(np.linalg.eigvals(a))) - 0.9) < 1e-12
    assert np.max(np.abs(growth[-5:] - 0.9)) < 1e-10
    assert abs(cm.rho(growth, done) - 0.9) < 1e-3 and cm.rho(growth, done) < 1
    # the float32 iteration on the same matrix: the device's precision
    g32, d32, _ = cm.power_dense(a, rng.standard_normal(n), 60, np.float32)
    assert d32 == 60 and g32.dtype == np.float32 and np.max(np.abs(g32[-5:].astype(np.float64) - 0.9)) < 1e-5


def test_mirror_on_a_recorded_body_finds_the_radius():
    g, st, ou, ds, p, v0 = _small_problem(seed=5)
    ctx = cm.context(g, st, ou, ds, p)
    radius = np.max(np.abs(np.linalg.eigvals(cm.dense_jt(ctx))))
    growth, done, _ = cm.power(ctx, v0, 400)
    assert done == 400 and 0 < radius < 1
    assert abs(np.exp(np.mean(np.log(growth[200:]))) - radius) <= 0.02 * radius        # (Gelfand: the geometric mean, whatever the phase)


def test_nilpotent_map_stops():
    """A strictly triangular J^T: (J^T)^4 = 0, the iteration stops with done = 4, later entries 0, rho 0."""
    a = np.diag(np.full(3, 0.5), -1)
    growth, done, w = cm.power_dense(a, np.ones(4), 8)
    assert done == 4 and growth[3] == 0.0 and np.all(growth[:3] > 0) and np.all(growth[4:] == 0) and not w.any()
    assert cm.rho(growth, done) == 0.0


# ---- surface ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    from GNN import _engine as e
    assert 'gnn_loop_contraction_estimate' in e.EXPORTS and 'gnn_loop_contraction_vector' in e.EXPORTS
    assert hasattr(e.lib(), 'gnn_loop_contraction_estimate') and hasattr(e.lib(), 'gnn_loop_contraction_vector')
    assert callable(e.Loop.contraction_estimate) and callable(e.Loop.contraction_vector)


def test_summary_of_a_result():
    from GNN import _engine as e
    r = e.contraction_summary(np.array([0.5, 0.25, 2.0, 0.5, 0.0, 0.0], np.float32), 4, 3.0)
    assert r['done'] == 4 and r['k'] == 3.0 and r['last'] == 0.5 and list(r['growth']) == [0.5, 0.25, 2.0, 0.5]
    assert abs(r['rho'] - 1.0) < 1e-12 and r['contractive'] is False                    # sqrt(2.0 * 0.5)
    z = e.contraction_summary(np.array([0.5, 0.0, 0.0], np.float32), 2, 1.0)
    assert z['rho'] == 0.0 and z['contractive'] is True and z['last'] == 0.0
    none = e.contraction_summary(np.zeros(3, np.float32), 0, 0.0)
    assert none['rho'] == 0.0 and none['done'] == 0 and none['growth'].size == 0 and none['last'] == 0.0


def _model(cls=None, dropout=0.0, state_dim=3):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    st = MLP(1 + 2 * (3 + 2), [8, 3], 'tanh', 'glorot_normal', 'zeros', dropout_rate=dropout, dropout_pos=0, batch_normalization=False)
    ou = MLP(3 + 2, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=state_dim, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_model_method_exists_and_refuses_its_arguments_without_a_device():
    from GNN.GNN import GNNnodeBased, GNNgraphBased, GNNedgeBased
    for cls in (GNNnodeBased, GNNgraphBased, GNNedgeBased):
        assert cls.contraction_estimate is GNNnodeBased.contraction_estimate
        gnn = _model(cls)
        for bad in (0, 1025, -1):
            with pytest.raises(ValueError, match='iterations'): gnn.contraction_estimate(None, iterations=bad)
    with pytest.raises(NotImplementedError, match='state_vect_dim'): _model(state_dim=0).contraction_estimate(None)
    with pytest.raises(NotImplementedError, match='Dropout'): _model(dropout=0.2).contraction_estimate(None)
