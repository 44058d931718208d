"""NumPy mirror of the fixed-point gradient for a net_state that ends in BatchNormalization on its MOVING statistics (include/gnn_hip.h:
gnn_loop_set_gradient_mode_ex with GNN_ADJOINT_FROZEN_BN), built on tests/adjoint_mirror.py and the Dense functions of the training oracle
(oracle/gnn_train_oracle.py).  TEST INFRASTRUCTURE; float64 by default, float32 on request (the noise of the reference itself).

    forward        the INFERENCE Loop to p (oracle/gnn_oracle.py: mlp_forward folds the moving statistics into scale and shift), training-mode
                   net_output on p
    recorded body  the Dense chain at p, then inv_j = 1 / sqrt(var_mov_j + eps), xhat = (h - mean_mov_j) inv_j, y = gamma_j xhat + beta_j
    backward       d gamma_j = sum_r d[r, j] xhat[r, j], d beta_j = sum_r d[r, j], d h = d s_j with s_j = gamma_j inv_j: no mean / variance terms
    adjoint        z <- g + J^T z with that backward pass; the weight gradients (gamma and beta included) of the last pass only

A net_state without BatchNormalization is the mirror of tests/adjoint_mirror.py itself (s = 1, no gamma / beta gradients)."""
import numpy as np

import adjoint_mirror as am
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro


def dense_part(net):
    """The Dense chain of a net as a net of its own (no BatchNormalization), for the training oracle's functions."""
    n = len(net['activations'])
    return dict(weights=list(net['weights'][:2 * n]), activations=list(net['activations']), batch_normalization=False)


def frozen_bn(net, dtype):
    """(gamma, beta, mean, inv, s = gamma inv) of a net's BatchNormalization on its moving statistics; None without one."""
    if not net['batch_normalization']: return None
    n = len(net['activations'])
    gamma, beta, mean, var = (np.asarray(v, dtype) for v in net['weights'][2 * n:2 * n + 4])
    inv = dtype(1) / np.sqrt(var + dtype(orc.BN_EPS))
    return gamma, beta, mean, inv, gamma * inv


def body_input(g, p, D, dtype):
    """The concat of a body at state p, and the column where the aggregated-state block starts."""
    nodes = np.asarray(g['nodes'], dtype)
    comps = p if not D else np.concatenate([p, nodes], axis=1)
    agg_nodes = orc.spmm_csr(g['adjT'], nodes, dtype) if D else np.zeros((nodes.shape[0], 0), dtype)
    agg_arcs = orc.spmm_csr(g['arcT'], np.asarray(g['arcs'], dtype)[:, 2:], dtype)
    return np.concatenate([comps, orc.spmm_csr(g['adjT'], p, dtype), agg_nodes, agg_arcs], axis=1), comps.shape[1]


def forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype=np.float64, edge_based=False, k_forced=None):
    """The inference Loop to p, training-mode net_output on p, the recorded body at p.  k_forced: exactly that many bodies (no gate decision)."""
    assert not net_state.get('dropout')
    if k_forced is not None: max_iteration, threshold = int(k_forced), -1.0
    nodes = np.asarray(g['nodes'], dtype)
    state = np.asarray(state0, dtype) if D else nodes.copy()
    state_old, k = np.ones_like(state), 0
    while bool(np.any(orc.not_converged(state, state_old, threshold))) and k < max_iteration:
        inp, _ = body_input(g, state, D, dtype)
        new = orc.mlp_forward(inp, net_state['weights'], net_state['activations'], net_state['batch_normalization'], dtype)
        k, state, state_old = k + 1, new, state
    mask = np.logical_and(g['set_mask'], g['output_mask'])
    feats = state if not D else np.concatenate([state, nodes], axis=1)
    rows_in = orc.edge_features(g, state, D, dtype) if edge_based else feats[mask]
    out_nodes, cache_o = tro.mlp_train_forward(rows_in, net_output, masks_output, dtype)
    inp, c_aggs = body_input(g, state, D, dtype)
    dense = dense_part(net_state)
    h, body = tro.mlp_train_forward(inp, dense, {}, dtype)
    bn = frozen_bn(net_state, dtype)
    xhat = y = None
    if bn is not None:
        gamma, beta, mean, inv, _ = bn
        xhat = (h - mean) * inv
        y = gamma * xhat + beta
    return dict(g=g, net_state=dense, net_state_full=net_state, net_output=net_output, D=D, k=k, cache_o=cache_o, mask=mask, state=state,
                out_nodes=out_nodes, dtype=dtype, edge_based=edge_based, recorded=body, c_aggs=c_aggs, bn=bn, xhat=xhat, body_out=y if bn is not None else h)


def jt(ctx, z):
    """(J^T z, weight gradients [dW1, db1, ..., (dgamma, dbeta)] of the recorded body for the incoming gradient z)."""
    d = np.asarray(z, ctx['dtype'])
    grads_bn = []
    if ctx['bn'] is not None:
        grads_bn = [np.sum(d * ctx['xhat'], axis=0), np.sum(d, axis=0)]
        d = d * ctx['bn'][4]
    out, grads = am.jt(ctx, d)                       # (ctx['net_state'] is the Dense chain: the mirror of the net without BatchNormalization)
    return out, grads + grads_bn


def adjoint(ctx, g_state, max_iter, threshold, iterations_forced=None):
    """am.adjoint with the frozen BatchNormalization inside J: (z_final, iterations, converged, weight gradients for z_final)."""
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
    """One training step without the optimizer, as am.step: dict(k, loss, out, state, g, z, grads_state, grads_output, adjoint_iterations,
    adjoint_converged)."""
    ctx = forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype, edge_based, k_forced)
    out = ctx['out_nodes']
    if graph_based:
        ng = np.asarray(g['NodeGraph'], dtype)
        out = ng.T @ out
    loss_value, d_out = tro.loss_forward_backward(loss, targets, out, sample_weights, dtype)
    if graph_based: d_out = ng @ d_out
    g_state, grads_o = am.state_gradient(ctx, d_out, d_state_extra)
    z, it, conv, grads_s = adjoint(ctx, g_state, max_iteration if adjoint_max_iter is None else adjoint_max_iter,
                                   threshold if adjoint_threshold is None else adjoint_threshold, iterations_forced)
    return dict(k=float(ctx['k']), loss=loss_value, out=out, state=ctx['state'], g=g_state, z=z, grads_state=grads_s, grads_output=grads_o,
                adjoint_iterations=it, adjoint_converged=conv, ctx=ctx)
