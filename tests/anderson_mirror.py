"""NumPy mirror of the Anderson-accelerated adjoint solve (include/gnn_hip.h: gnn_loop_set_adjoint_solver) for the tests, built on
tests/adjoint_mirror.py: the operator is adjoint_mirror.jt, the gate its gate applied to the residual.  TEST INFRASTRUCTURE.

dtype=np.float64: everything in float64.  dtype=np.float32 is what the device does: vectors, residuals and the rings of difference rows in float32,
gamma rounded to float32 in front of the mix; the Gram matrix, b and the Cholesky solve in float64.

z_0 = g.  Iteration t: G = g + J^T z, f = G - z, gate: a node moves when |f[r]| > threshold |z[r]| (strict).  Closed: z_final = G.  t = 0: z_1 = G.
t >= 1, with hist = difference pairs stored since the last restart: slot s = hist mod m gets dF_s = f - f_prev, dG_s = G - G_prev, live = min(hist + 1, m);
H_ij = dF_i . dF_j, b_i = dF_i . f over the live slots (row and column s of H new, the rest kept); (H + lambda I) gamma = b, lambda = 2^-40 trace(H) / live, by
Cholesky; a pivot that is not > 0 or a value that is not finite restarts (gamma = 0, hist = 0); z_next = G - sum_i gamma_i dG_i over ascending slots."""
import numpy as np

import adjoint_bn_mirror as abm
import adjoint_mirror as am

MAX_WINDOW = 8


def cholesky_solve(a, b):
    """(ok, gamma): the device's solve - lower Cholesky factor row by row, forward and back substitution, all float64; ok False on a pivot that
    is not > 0 or on any value that is not finite."""
    n = len(b)
    low, y, gamma = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    with np.errstate(all='ignore'):
        for i in range(n):
            for j in range(i + 1):
                v = a[i, j]
                for k in range(j): v = v - low[i, k] * low[j, k]
                if i == j:
                    if not v > 0.0 or not np.isfinite(v): return False, np.zeros(n)
                    low[i, i] = np.sqrt(v)
                else:
                    low[i, j] = v / low[j, j]
        for i in range(n):
            v = b[i]
            for k in range(i): v = v - low[i, k] * y[k]
            y[i] = v / low[i, i]
        for i in range(n - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, n): v = v - low[k, i] * gamma[k]
            gamma[i] = v / low[i, i]
        if not np.all(np.isfinite(gamma)) or not np.all(np.isfinite(gamma.astype(np.float32))): return False, np.zeros(n)
    return True, gamma


def anderson(ctx, g_state, max_iter, threshold, window, iterations_forced=None, final_mix=False, trace=None, operator=None):
    """Returns (z_final, iterations, converged, restarts, weight gradients for z_final).  iterations_forced: exactly that many iterations, no gate
    decision; the last of them ends as a closed gate does (z_final = G) unless final_mix, which ends it as the count reaching max_iter with an open
    gate does (z_final = the mixed iterate).  trace: a list that receives (live, gamma, restarted) per mixing iteration.  operator: (ctx, z) -> (J^T z, weight
    gradients); default adjoint_mirror.jt, or for a context of tests/adjoint_bn_mirror.py its jt (adjoint_mirror.jt behind the frozen BatchNormalization)."""
    if operator is None: operator = abm.jt if 'bn' in ctx else am.jt
    if not 1 <= int(window) <= MAX_WINDOW: raise ValueError('window must lie in [1, 8]')
    dtype, m = ctx['dtype'], int(window)
    g = np.asarray(g_state, dtype)
    z = g
    total = max_iter if iterations_forced is None else iterations_forced
    it, converged, restarts, hist = 0, g.shape[0] == 0 or total == 0, 0, 0
    gram = np.zeros((MAX_WINDOW, MAX_WINDOW))
    d_f, d_g = [None] * m, [None] * m
    g_prev = f_prev = None
    for t in range(0 if g.shape[0] else total, total):
        big = (g + operator(ctx, z)[0]).astype(dtype)
        f = big - z
        closed = not bool((np.linalg.norm(f, axis=1) > dtype(threshold) * np.linalg.norm(z, axis=1)).any())
        it = t + 1
        if (closed if iterations_forced is None else (t == total - 1 and not final_mix)):
            z, converged = big, closed
            break
        if t == 0:
            z_next = big
        else:
            s, live = hist % m, min(hist + 1, m)
            d_f[s], d_g[s] = f - f_prev, big - g_prev
            b = np.zeros(live)
            for j in range(live):
                gram[s, j] = gram[j, s] = float(np.dot(d_f[s].ravel().astype(np.float64), d_f[j].ravel().astype(np.float64)))
                b[j] = float(np.dot(d_f[j].ravel().astype(np.float64), f.ravel().astype(np.float64)))
            with np.errstate(all='ignore'):
                lam = float(np.trace(gram[:live, :live])) * 2.0 ** -40 / live
            ok, gamma = (False, np.zeros(live)) if not np.isfinite(lam) else cholesky_solve(gram[:live, :live] + lam * np.eye(live), b)
            if ok: hist += 1
            else: hist, restarts = 0, restarts + 1
            if trace is not None: trace.append((live, gamma.copy(), not ok))
            acc = np.zeros_like(big)
            for j in range(live if ok else 0): acc = dtype(gamma[j]) * d_g[j] + acc
            z_next = big - acc
        g_prev, f_prev, z, converged = big, f, z_next, False
    return z, it, converged, restarts, operator(ctx, z)[1]


def step(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, targets, sample_weights, window, loss='categorical_crossentropy',
         graph_based=False, edge_based=False, adjoint_max_iter=None, adjoint_threshold=None, d_state_extra=None, dtype=np.float64, k_forced=None,
         iterations_forced=None, final_mix=False):
    """adjoint_mirror.step with the Anderson solve in place of the plain iteration (forward and operator of tests/adjoint_bn_mirror.py, which are
    adjoint_mirror's for a net_state without BatchNormalization); the dict also carries restarts."""
    ctx = abm.forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype, edge_based, k_forced)
    out = ctx['out_nodes']
    if graph_based:
        ng = np.asarray(g['NodeGraph'], dtype)
        out = ng.T @ out
    loss_value, d_out = am.tro.loss_forward_backward(loss, targets, out, sample_weights, dtype)
    if graph_based: d_out = ng @ d_out
    g_state, grads_o = am.state_gradient(ctx, d_out, d_state_extra)
    z, it, conv, restarts, grads_s = anderson(ctx, g_state, max_iteration if adjoint_max_iter is None else adjoint_max_iter,
                                              threshold if adjoint_threshold is None else adjoint_threshold, window, iterations_forced, final_mix)
    return dict(k=float(ctx['k']), loss=loss_value, out=out, state=ctx['state'], g=g_state, z=z, grads_state=grads_s, grads_output=grads_o,
                adjoint_iterations=it, adjoint_converged=conv, restarts=restarts, ctx=ctx)
