"""NumPy mirror of the contraction estimate (include/gnn_hip.h: gnn_loop_contraction_estimate) for the tests, built on the fixed-point mirrors
(tests/adjoint_mirror.py through tests/adjoint_bn_mirror.py, whose jt() is J^T with a frozen BatchNormalization inside or without one).  TEST
INFRASTRUCTURE; float64 by default, float32 on request (the noise of the reference itself).

    context      ONE recorded body of net_state at a GIVEN state p (the device's: no gate decision enters a comparison)
    power        w_0 = v0, n_0 = |w_0|;  w_t = (J^T w_{t-1}) * (1 / n_{t-1}), n_t = |w_t|, growth[t - 1] = n_t;  stops where n_t is 0 or not finite
    dense_jt     J^T assembled column by column from jt(), as tests/test_adjoint_host.py assembles it
    power_dense  the same iteration on a dense matrix, in any dtype (float32: the iteration in the device's precision on the float64 J)"""
import numpy as np

import adjoint_bn_mirror as bm


def context(g, net_state, net_output, D, p, dtype=np.float64):
    """The recorded body at p (bm.forward with no body run: state = p)."""
    return bm.forward(g, net_state, net_output, D, 0, -1.0, np.asarray(p, dtype), {}, dtype, k_forced=0)


def _norm(w, dtype):
    return dtype(np.sqrt(np.sum(np.square(w, dtype=dtype), dtype=dtype)))


def power(ctx, v0, iterations):
    """(growth [iterations], done, w_done) in the context's dtype."""
    dtype = ctx['dtype']
    w = np.asarray(v0, dtype)
    n = _norm(w, dtype)
    growth = np.zeros(iterations, dtype)
    for t in range(1, iterations + 1):
        if not (n > 0 and np.isfinite(n)): return growth, t - 1, w
        w = (bm.jt(ctx, w)[0] * (dtype(1) / n)).astype(dtype)
        n = _norm(w, dtype)
        growth[t - 1] = n
    return growth, iterations, w


def dense_jt(ctx):
    n, ds = ctx['state'].shape
    jt = np.zeros((n * ds, n * ds), ctx['dtype'])
    for i in range(n * ds):
        e = np.zeros(n * ds, ctx['dtype']); e[i] = 1
        jt[:, i] = bm.jt(ctx, e.reshape(n, ds))[0].ravel()
    return jt


def power_dense(jt, v0, iterations, dtype=np.float64):
    """The iteration on a dense J^T: (growth, done, w_done as a flat vector)."""
    a = np.asarray(jt, dtype)
    w = np.asarray(v0, dtype).ravel()
    n = _norm(w, dtype)
    growth = np.zeros(iterations, dtype)
    for t in range(1, iterations + 1):
        if not (n > 0 and np.isfinite(n)): return growth, t - 1, w
        w = ((a @ w) * (dtype(1) / n)).astype(dtype)
        n = _norm(w, dtype)
        growth[t - 1] = n
    return growth, iterations, w


def rho(growth, done):
    """exp(mean(log(growth[done // 2 : done]))), 0.0 when a growth entry is 0 (GNN/_engine.py: contraction_summary)."""
    g = np.asarray(growth, np.float64)[:done]
    if done == 0 or np.any(g == 0): return 0.0
    return float(np.exp(np.mean(np.log(g[done // 2:done]))))
