"""The Anderson-accelerated adjoint solve (include/gnn_hip.h: gnn_loop_set_adjoint_solver) without a device: its mirror (tests/anderson_mirror.py)
against the dense solve of (I - J^T) z = g, its iteration counts against the plain iteration's (tests/adjoint_mirror.py), the restart of the window,
window 1 and the truncated solve, and the Python surface that needs no GPU.

The bound of the dense comparison is derived, not measured.  The solve ends on a closed gate: |f[r]| <= thr |z_t[r]| for every row r, so |f|_2 <= thr |z_t|_2
over the whole vector.  With z* the solution, z_final = G_t = g + J^T z_t and z* = g + J^T z* give z_final - z* = J^T (z_t - z*), and
(I - J^T)(z_t - z*) = z_t - G_t = -f, hence
    |z_final - z*|_2 <= |J^T|_2 |(I - J^T)^-1|_2 thr |z_t|_2,      |z_t|_2 <= |z_final|_2 / (1 - thr)   (z_t = z_final - f),
both norms taken from the dense matrix.  thr carries ROUND = 1e-12 on top: the gate sees the float64 EVALUATION of f (a few hundred operations per element at
1.1e-16) and the reference is a LAPACK solve of a matrix whose condition number is below 100 here; the term matters only where thr is 0."""
import functools

import numpy as np
import pytest

import adjoint_mirror as am
import anderson_mirror as an
from test_gpu_adjoint import problem

ROUND = 1e-12
THR = 1e-4
# the problems of the measurements that led to the solver (seed 3, tanh, threshold 1e-4), with the spectral radius of J a dense eigenvalue solve gave
TABLE = {'rho0.146': dict(n=37, ds=8, hidden=(9, 6), gain=0.5), 'rho0.836': dict(n=37, ds=8, hidden=(9, 6), gain=1.0),
         'rho0.799': dict(n=83, ds=4, hub=70, isolated=True, gain=1.3), 'rho0.952': dict(n=17, ds=64, hidden=(20,), gain=1.3),
         'rho0.969': dict(n=17, ds=64, hidden=(20,), gain=1.6)}


def dense_jt(ctx):
    """J^T [n Ds, n Ds], column by column from adjoint_mirror.jt (a context of tests/adjoint_bn_mirror.py: from its jt, the same behind the frozen
    BatchNormalization)."""
    operator = an.abm.jt if 'bn' in ctx else am.jt
    n, ds = ctx['state'].shape
    a = np.zeros((n * ds, n * ds))
    for i in range(n * ds):
        e = np.zeros(n * ds)
        e[i] = 1.0
        a[:, i] = operator(ctx, e.reshape(n, ds))[0].ravel()
    return a


def dense_bound(a, thr, z_final):
    thr = thr + ROUND
    eye = np.eye(a.shape[0])
    return np.linalg.norm(a, 2) * np.linalg.norm(np.linalg.inv(eye - a), 2) * thr * np.linalg.norm(z_final) / (1.0 - thr)


@functools.lru_cache(maxsize=None)
def solved(name):
    """The Picard step of a TABLE problem in float64 (its context, g, count), the dense J^T and the dense solution."""
    pb = problem(3, **TABLE[name])
    r = am.step(pb['g'], pb['st'], pb['ou'], pb['D'], 400, THR, pb['s0'], {}, pb['targets'], pb['weights'])
    a = dense_jt(r['ctx'])
    star = np.linalg.solve(np.eye(a.shape[0]) - a, r['g'].ravel()).reshape(r['g'].shape)
    return r, a, star


# ---- 1. the mirror against the dense solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', [1, 3, 8])
@pytest.mark.parametrize('name', list(TABLE))
def test_mirror_against_the_dense_solve(name, window):
    r, a, star = solved(name)
    assert float(name[3:]) == pytest.approx(np.max(np.abs(np.linalg.eigvals(a))), abs=2e-3)        # (the problem is the one that was measured)
    z, it, conv, restarts, grads = an.anderson(r['ctx'], r['g'], 400, THR, window)
    assert conv and restarts == 0 and 2 <= it < 400
    err, bound = np.linalg.norm(z - star), dense_bound(a, THR, z)
    print(f'{name} window {window}: {it} iterations, |z - z*| {err:.3e}, bound {bound:.3e}, Picard {r["adjoint_iterations"]} with {np.linalg.norm(r["z"] - star):.3e}')
    assert err <= bound
    # the weight gradients are those of one pass with z_final
    for got, want in zip(grads, am.jt(r['ctx'], z)[1]): assert np.array_equal(got, want)


# ---- 2. iteration counts ----------------------------------------------------------------------------------------------------------------------------
def test_iteration_counts_against_picard():
    counts = {}
    for name in ('rho0.146', 'rho0.836', 'rho0.952'):
        r, _, _ = solved(name)
        counts[name] = (an.anderson(r['ctx'], r['g'], 400, THR, 5)[1], r['adjoint_iterations'])
        assert r['adjoint_converged']
    print(counts)
    assert counts['rho0.146'][0] <= counts['rho0.146'][1]                 # nothing is lost where the plain iteration is fast
    assert 2 * counts['rho0.836'][0] <= counts['rho0.836'][1]             # (measured: 12 against 47)
    assert 2 * counts['rho0.952'][0] <= counts['rho0.952'][1]             # (measured: 29 against 144)


def test_float32_mirror_is_the_device_definition():
    """dtype float32: vectors and rings in float32, the Gram matrix in float64; on these problems it takes the float64 mirror's counts."""
    for name in ('rho0.146', 'rho0.836'):
        pb = problem(3, **TABLE[name])
        args = (pb['g'], pb['st'], pb['ou'], pb['D'], 400, THR, pb['s0'], {}, pb['targets'], pb['weights'], 5)
        lo, hi = an.step(*args, dtype=np.float32), an.step(*args)
        assert lo['z'].dtype == np.float32 and hi['z'].dtype == np.float64
        assert lo['adjoint_iterations'] == hi['adjoint_iterations'] and lo['adjoint_converged'] and hi['adjoint_converged']
        assert np.max(np.abs(lo['z'] - hi['z'])) <= 1e-3 * np.max(np.abs(hi['z']))
        # iterations_forced: exactly that many, ending as a closed gate does
        forced = an.step(*args, iterations_forced=hi['adjoint_iterations'])
        assert np.array_equal(forced['z'], hi['z']) and forced['adjoint_iterations'] == hi['adjoint_iterations']
        fewer = an.step(*args, iterations_forced=3)
        assert fewer['adjoint_iterations'] == 3 and not fewer['adjoint_converged'] and not np.array_equal(fewer['z'], hi['z'])


# ---- 3. the restart -----------------------------------------------------------------------------------------------------------------------------------
def test_cholesky_refuses_what_restarts_the_window():
    ok, gamma = an.cholesky_solve(np.array([[4.0, 2.0], [2.0, 3.0]]), np.array([2.0, 1.0]))
    assert ok and np.allclose(gamma, np.linalg.solve([[4.0, 2.0], [2.0, 3.0]], [2.0, 1.0]), rtol=1e-14)
    assert an.cholesky_solve(np.zeros((1, 1)), np.zeros(1))[0] is False                                   # a zero pivot
    assert an.cholesky_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2))[0] is False                  # a negative second pivot
    assert an.cholesky_solve(np.array([[np.inf]]), np.ones(1))[0] is False and an.cholesky_solve(np.array([[np.nan]]), np.ones(1))[0] is False
    assert an.cholesky_solve(np.array([[1e-300]]), np.array([1e300]))[0] is False                         # gamma is no float


def test_restart_keeps_the_solve_finite_and_within_the_bound():
    """Threshold 0: the solve runs on until G(z) == z bit for bit.  In front of that the residual stops changing at rounding level, the window's
    difference rows become exactly 0, trace(H) = 0 leaves a zero pivot and the window restarts; the Picard steps behind a restart reach the bitwise
    fixed point.  The case is the first of a few seeds whose float64 mirror does restart and does close its gate (with the arithmetic these lines were
    written on: seed 5, window 2, 25 iterations, one restart)."""
    found = None
    for seed in (5, 0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11):
        pb = problem(seed, n=15, ds=4)
        r = am.step(pb['g'], pb['st'], pb['ou'], pb['D'], 50, THR, pb['s0'], {}, pb['targets'], pb['weights'], adjoint_max_iter=1)
        for window in (2, 1, 3, 5, 8):
            z, it, conv, restarts, _ = an.anderson(r['ctx'], r['g'], 120, 0.0, window)
            assert np.isfinite(z).all()
            if restarts >= 1 and conv and found is None: found = (r['ctx'], r['g'], z, it, restarts)
        if found: break
    assert found is not None, 'no seed restarts and converges: pick another case'
    ctx, g, z, it, restarts = found
    a = dense_jt(ctx)
    star = np.linalg.solve(np.eye(a.shape[0]) - a, g.ravel()).reshape(g.shape)
    assert restarts >= 1 and np.isfinite(z).all() and np.linalg.norm(z - star) <= dense_bound(a, 0.0, z)


# ---- 4. window 1, and the count reaching max_iteration ------------------------------------------------------------------------------------------------
def test_window_one_and_the_truncated_solve():
    r, a, star = solved('rho0.969')
    z, it, conv, restarts, _ = an.anderson(r['ctx'], r['g'], 400, THR, 1)
    assert conv and np.linalg.norm(z - star) <= dense_bound(a, THR, z)
    trace = []
    an.anderson(r['ctx'], r['g'], 12, THR, 1, trace=trace)
    assert [live for live, _, _ in trace] == [1] * 11                      # one slot, rewritten by every iteration behind the first
    for window in (1, 5):
        z, it, conv, restarts, grads = an.anderson(r['ctx'], r['g'], 10, THR, window)
        assert (it, conv) == (10, False) and np.isfinite(z).all()
        # the truncated result is the mixed iterate: what ten forced iterations with final_mix return, and not what a closed gate would
        forced = an.anderson(r['ctx'], r['g'], 400, THR, window, iterations_forced=10, final_mix=True)
        closed = an.anderson(r['ctx'], r['g'], 400, THR, window, iterations_forced=10)
        assert np.array_equal(forced[0], z) and forced[1:4] == (10, False, restarts) and not np.array_equal(closed[0], z)
    assert an.anderson(r['ctx'], r['g'], 0, THR, 3)[:4][1:] == (0, True, 0)
    with pytest.raises(ValueError): an.anderson(r['ctx'], r['g'], 5, THR, 9)
    with pytest.raises(ValueError): an.anderson(r['ctx'], r['g'], 5, THR, 0)


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------------------------------
def _model(cls=None, ds=3, layer=0, bn=False):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (ds + 3 + extra), [8, ds], 'tanh', 'glorot_normal', 'zeros', batch_normalization=bn)
    ou = MLP(ds + 3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=ds, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_symbols_and_engine_methods():
    from GNN import _engine as e
    for name in ('gnn_loop_set_adjoint_solver', 'gnn_loop_adjoint_solver_info'): assert name in e.EXPORTS and hasattr(e.lib(), name)
    assert e.SOLVER_NAMES == {0: 'picard', 1: 'anderson'}
    assert callable(e.Loop.set_adjoint_solver) and callable(e.Loop.adjoint_solver_info)
    # the existing calls keep their symbols
    for name in ('gnn_loop_set_gradient_mode', 'gnn_loop_set_gradient_mode_ex', 'gnn_loop_adjoint_info', 'gnn_adjoint_form', 'gnn_adjoint_form_ex'):
        assert hasattr(e.lib(), name)


def test_keywords_and_their_refusals():
    gnn = _model()
    assert (gnn.adjoint_solver, gnn.anderson_window) == ('picard', 5)
    gnn.set_gradient_mode('fixed_point', adjoint_solver='anderson')
    assert (gnn.adjoint_solver, gnn.anderson_window) == ('anderson', 5)
    gnn.set_gradient_mode('fixed_point', adjoint_solver='anderson', anderson_window=8)
    assert gnn._gradient_config() == dict(mode='fixed_point', max_iteration=None, threshold=None, adjoint_solver='anderson', anderson_window=8)
    for kw in (dict(adjoint_solver='gmres'), dict(adjoint_solver=1), dict(adjoint_solver=None), dict(anderson_window=0), dict(anderson_window=9),
               dict(anderson_window=2.0), dict(anderson_window=True), dict(anderson_window='5')):
        with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', **kw)
        assert (gnn.adjoint_solver, gnn.anderson_window) == ('anderson', 8)           # a refused call leaves the setting
    gnn.set_gradient_mode('fixed_point')
    assert (gnn.adjoint_solver, gnn.anderson_window) == ('picard', 5)                 # the default is Picard
    gnn.set_gradient_mode('unrolled', adjoint_solver='anderson', anderson_window=3)   # stored, without effect, as max_iteration / threshold
    assert (gnn.gradient_mode, gnn.adjoint_solver, gnn.anderson_window) == ('unrolled', 'anderson', 3)
    both = _model(bn=True)
    both.set_gradient_mode('fixed_point', 20, 1e-3, batch_normalization='frozen', label_gradients=True, adjoint_solver='anderson', anderson_window=1)
    assert both._gradient_config() == dict(mode='fixed_point', max_iteration=20, threshold=1e-3, batch_normalization='frozen', label_gradients=True,
                                           adjoint_solver='anderson', anderson_window=1)


def test_copy_lko_save_load_keep_the_solver(tmp_path):
    import json
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    for cls in (None, GNNgraphBased, GNNedgeBased):
        gnn = _model(cls)
        gnn.set_gradient_mode('fixed_point', 25, 1e-3, adjoint_solver='anderson', anderson_window=3)
        want = dict(mode='fixed_point', max_iteration=25, threshold=1e-3, adjoint_solver='anderson', anderson_window=3)
        twin = gnn.copy(copy_weights=False)                               # (LKO builds its models with copy())
        assert type(twin) is type(gnn) and twin._gradient_config() == gnn._gradient_config() == want
        assert (twin.adjoint_solver, twin.anderson_window) == ('anderson', 3)
        path = str(tmp_path / f'model{cls.__name__ if cls else ""}')
        gnn.save(path)
        with open(f'{path}/config.json') as f: assert json.load(f)['gradient_mode'] == want
        back = type(gnn).load(path)
        assert back._gradient_config() == want and (back.adjoint_solver, back.anderson_window) == ('anderson', 3)
    # a model without the keywords: its dict and its file are what they were
    plain = _model()
    plain.set_gradient_mode('fixed_point', 25, 1e-3)
    assert list(plain._gradient_config()) == ['mode', 'max_iteration', 'threshold']
    plain.save(str(tmp_path / 'plain'))
    with open(str(tmp_path / 'plain' / 'config.json')) as f: assert 'anderson' not in f.read()
    assert type(plain).load(str(tmp_path / 'plain')).adjoint_solver == 'picard'


def test_lgnn_forwards_the_solver(tmp_path):
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    lgnn = LGNN([_model(), _model(layer=1)], get_state=False, get_output=True, optimizer=optimizers.Adam(0.02),
                loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    lgnn.set_gradient_mode('fixed_point', 20, label_gradients=True, adjoint_solver='anderson', anderson_window=4)
    assert [(g.gradient_mode, g.adjoint_label_gradients, g.adjoint_solver, g.anderson_window) for g in lgnn.gnns] == [('fixed_point', True, 'anderson', 4)] * 2
    assert [(g.adjoint_solver, g.anderson_window) for g in lgnn.copy().gnns] == [('anderson', 4)] * 2
    lgnn.save(str(tmp_path / 'stack'))
    assert [(g.adjoint_solver, g.anderson_window) for g in LGNN.load(str(tmp_path / 'stack')).gnns] == [('anderson', 4)] * 2
    with pytest.raises(ValueError): lgnn.set_gradient_mode('fixed_point', adjoint_solver='broyden')
    lgnn.set_gradient_mode('fixed_point', 20)
    assert [g.adjoint_solver for g in lgnn.gnns] == ['picard'] * 2
