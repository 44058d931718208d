"""NumPy mirror of gradient mode 1 ("fixed point", include/gnn_hip.h: gnn_loop_set_gradient_mode) for the tests, built from the training oracle's
functions (oracle/gnn_train_oracle.py): forward to p, ONE recorded body at p (mlp_train_forward), the adjoint iteration z <- g + J^T z with
repeated mlp_train_backward, and the weight gradients of the last pass only.  TEST INFRASTRUCTURE; float64 by default, float32 on request (the
noise of the reference itself, tests/test_gpu_adjoint.py)."""
import numpy as np

from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro


def forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype=np.float64, edge_based=False, k_forced=None):
    """Forward of mode 1: the Loop to p (net_state has neither Dropout nor BatchNormalization: its training-mode forward IS the inference
    forward), training-mode net_output on p, and the recorded body at p.  k_forced: run exactly that many bodies (no gate decision)."""
    assert not net_state['batch_normalization'] and not net_state.get('dropout')
    if k_forced is not None: max_iteration, threshold = int(k_forced), -1.0
    ctx = tro.train_forward(g, net_state, net_output, D, max_iteration, threshold, state0, [{}] * max(1, max_iteration), masks_output, dtype=dtype,
                            edge_based=edge_based)
    p = ctx['state']
    nodes = np.asarray(g['nodes'], dtype)
    comps = p if not D else np.concatenate([p, nodes], axis=1)
    agg_nodes = orc.spmm_csr(g['adjT'], nodes, dtype) if D else np.zeros((nodes.shape[0], 0), dtype)
    agg_arcs = orc.spmm_csr(g['arcT'], np.asarray(g['arcs'], dtype)[:, 2:], dtype)
    inp = np.concatenate([comps, orc.spmm_csr(g['adjT'], p, dtype), agg_nodes, agg_arcs], axis=1)
    _, body = tro.mlp_train_forward(inp, net_state, {}, dtype)
    ctx['recorded'] = body
    ctx['c_aggs'] = comps.shape[1]
    return ctx


def state_gradient(ctx, d_out_nodes, d_state_extra=None):
    """(g = d loss / d p, gradients of net_output): the first lines of the oracle's train_backward, the scatter of d feats onto the state."""
    g, dtype = ctx['g'], ctx['dtype']
    n, ds = ctx['state'].shape
    nl = np.asarray(g['nodes']).shape[1]
    mask = ctx['mask']
    d_feats, grads_o = tro.mlp_train_backward(d_out_nodes, ctx['net_output'], ctx['cache_o'], dtype)
    d_state = np.zeros((n, ds), dtype)
    if ctx.get('edge_based'):
        indptr, src, _ = g['adjT']
        dst = np.repeat(np.arange(n), np.diff(indptr))
        wn = ds + (nl if ctx['D'] else 0)
        np.add.at(d_state, dst[mask], d_feats[:, :ds])
        np.add.at(d_state, src[mask], d_feats[:, wn:wn + ds])
    else:
        d_state[mask] = d_feats[:, :ds]
    if d_state_extra is not None: d_state = d_state + np.asarray(d_state_extra, dtype)
    return d_state, grads_o


def jt(ctx, z):
    """(J^T z, weight gradients of the recorded body for the incoming gradient z): J = d body / d state at p over the own-state columns and
    the aggregated-state columns (Adjacency^T . state => d state[src] += w d agg[dst])."""
    g, dtype = ctx['g'], ctx['dtype']
    n, ds = ctx['state'].shape
    indptr, src, w = g['adjT']
    dst = np.repeat(np.arange(n), np.diff(indptr))
    d_inp, grads = tro.mlp_train_backward(z, ctx['net_state'], ctx['recorded'], dtype)
    out = d_inp[:, :ds].copy()
    ca = ctx['c_aggs']
    np.add.at(out, src, np.asarray(w, dtype)[:, None] * d_inp[dst, ca:ca + ds])
    return out, grads


def adjoint(ctx, g_state, max_iter, threshold, iterations_forced=None):
    """z_0 = g, z_{t+1} = g + J^T z_t until no node has |z_{t+1}[r] - z_t[r]| > threshold |z_t[r]| (strict) or max_iter iterations;
    iterations_forced: exactly that many (no gate decision).  Returns (z_final, iterations, converged, weight gradients for z_final)."""
    dtype = ctx['dtype']
    z = np.asarray(g_state, dtype)
    it, converged = 0, z.shape[0] == 0 or max_iter == 0
    total = max_iter if iterations_forced is None else iterations_forced
    while it < total and (iterations_forced is not None or not converged):
        z_new = np.asarray(g_state, dtype) + jt(ctx, z)[0]
        moved = np.linalg.norm(z_new - z, axis=1) > dtype(threshold) * np.linalg.norm(z, axis=1)
        z, it = z_new, it + 1
        converged = not bool(moved.any())
    return z, it, converged, jt(ctx, z)[1]


def step(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, targets, sample_weights, loss='categorical_crossentropy',
         graph_based=False, edge_based=False, adjoint_max_iter=None, adjoint_threshold=None, d_state_extra=None, dtype=np.float64, k_forced=None,
         iterations_forced=None):
    """One training step of mode 1 without the optimizer: dict(k, loss, out, state, g, z, grads_state (NOT divided by k), grads_output,
    adjoint_iterations, adjoint_converged)."""
    ctx = forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype, edge_based, k_forced)
    out = ctx['out_nodes']
    if graph_based:
        ng = np.asarray(g['NodeGraph'], dtype)
        out = ng.T @ out
    loss_value, d_out = tro.loss_forward_backward(loss, targets, out, sample_weights, dtype)
    if graph_based: d_out = ng @ d_out
    g_state, grads_o = state_gradient(ctx, d_out, d_state_extra)
    z, it, conv, grads_s = adjoint(ctx, g_state, max_iteration if adjoint_max_iter is None else adjoint_max_iter,
                                   threshold if adjoint_threshold is None else adjoint_threshold, iterations_forced)
    return dict(k=float(ctx['k']), loss=loss_value, out=out, state=ctx['state'], g=g_state, z=z, grads_state=grads_s, grads_output=grads_o,
                adjoint_iterations=it, adjoint_converged=conv, ctx=ctx)
