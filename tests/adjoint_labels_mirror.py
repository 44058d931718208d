"""NumPy mirror of the label gradients of the fixed-point gradient modes (include/gnn_hip.h: GNN_ADJOINT_LABEL_GRADIENTS) and of the LGNN joint steps
built on them, for the tests.  Per layer it is tests/adjoint_bn_mirror.py (which is tests/adjoint_mirror.py for a net_state without
BatchNormalization); around the layers it has the structure of oracle.gnn_train_oracle.lgnn_train_step.  TEST INFRASTRUCTURE; float64 by default,
float32 on request (the noise of the reference itself).

With p = F(p, l) the fixed point, l the labels a layer saw, g = d loss / d p and z = g + J^T z:

    d loss / d l = (direct part through net_output / the edge readout) + (d F / d l)^T z

(d F / d l)^T z is the label columns of the recorded body's d concat for the incoming gradient z, scattered as ONE body of the unrolled step: own node
columns directly, aggregated-node columns over the adjacency by source (aggregated_nodes = Adjacency^T . nodes => d nodes[src] += w d agg[dst]),
aggregated-arc columns through ArcNode^T."""
import numpy as np

import adjoint_bn_mirror as abm
import adjoint_mirror as am
from oracle import gnn_train_oracle as tro


def backward(ctx, d_out_nodes, d_state_extra=None, max_iter=50, threshold=1e-3, iterations_forced=None):
    """The backward pass of one fixed-point layer from its forward context (abm.forward): dict(grads_state, grads_output, d_nodes [N, NL], d_arcs
    [E, AL] in original arc order, g, z, adjoint_iterations, adjoint_converged).  D == 0 has no label gradient (the labels are the INITIAL state)."""
    g, dtype, D = ctx['g'], ctx['dtype'], ctx['D']
    assert D, 'state_vect_dim == 0: a fixed point does not depend on its initial state'
    nodes = np.asarray(g['nodes'], dtype)
    n, nl = nodes.shape
    ds = ctx['state'].shape[1]
    al = np.asarray(g['arcs']).shape[1] - 2
    mask = ctx['mask']
    g_state, grads_o = am.state_gradient(ctx, np.asarray(d_out_nodes, dtype).copy(), d_state_extra)
    z, it, conv, grads_s = abm.adjoint(ctx, g_state, max_iter, threshold, iterations_forced)
    indptr, src, w = g['adjT']
    w = np.asarray(w, dtype)
    dst = np.repeat(np.arange(n), np.diff(indptr))
    # ---- direct part: the label columns of net_output's input rows
    d_feats, _ = tro.mlp_train_backward(np.asarray(d_out_nodes, dtype).copy(), ctx['net_output'], ctx['cache_o'], dtype)
    d_nodes = np.zeros((n, nl), dtype)
    d_arcs = np.zeros((np.asarray(g['arcs']).shape[0], al), dtype)
    wn = ds + nl
    if ctx.get('edge_based'):
        np.add.at(d_nodes, dst[mask], d_feats[:, ds:wn])
        np.add.at(d_nodes, src[mask], d_feats[:, wn + ds:2 * wn])
        d_arcs[np.nonzero(mask)[0]] += d_feats[:, 2 * wn:2 * wn + al]
    else:
        d_nodes[mask] += d_feats[:, ds:]
    # ---- (d F / d l)^T z: the label columns of the recorded body's d concat for z
    d = np.asarray(z, dtype).copy()
    if ctx['bn'] is not None: d = d * ctx['bn'][4]
    d_inp, _ = tro.mlp_train_backward(d, ctx['net_state'], ctx['recorded'], dtype)
    c_aggs = ds + nl
    c_aggn = c_aggs + ds
    c_agga = c_aggn + nl
    d_nodes += d_inp[:, ds:ds + nl]
    np.add.at(d_nodes, src, w[:, None] * d_inp[dst, c_aggn:c_aggn + nl])
    ip_a, arc_id, w_a = g['arcT']
    dst_a = np.repeat(np.arange(n), np.diff(ip_a))
    d_arcs[arc_id] += np.asarray(w_a, dtype)[:, None] * d_inp[dst_a, c_agga:c_agga + al]
    return dict(grads_state=grads_s, grads_output=grads_o, d_nodes=d_nodes, d_arcs=d_arcs, g=g_state, z=z, adjoint_iterations=it, adjoint_converged=conv)


def halves(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, d_out_nodes, d_state_extra=None, edge_based=False,
           adjoint_max_iter=None, adjoint_threshold=None, dtype=np.float64, k_forced=None, iterations_forced=None):
    """Forward + backward of one layer for a GIVEN d loss / d out_nodes (the two halves of the C ABI): backward()'s dict with k, state, out."""
    ctx = abm.forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype, edge_based, k_forced)
    r = backward(ctx, d_out_nodes, d_state_extra, max_iteration if adjoint_max_iter is None else adjoint_max_iter,
                 threshold if adjoint_threshold is None else adjoint_threshold, iterations_forced)
    r.update(k=float(ctx['k']), state=ctx['state'], out=ctx['out_nodes'], ctx=ctx)
    return r


def step(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, targets, sample_weights, loss='categorical_crossentropy',
         graph_based=False, edge_based=False, adjoint_max_iter=None, adjoint_threshold=None, dtype=np.float64, k_forced=None, iterations_forced=None):
    """One training step of a single fixed-point GNN with its label gradients: halves()'s dict with loss."""
    ctx = abm.forward(g, net_state, net_output, D, max_iteration, threshold, state0, masks_output, dtype, edge_based, k_forced)
    out = ctx['out_nodes']
    if graph_based:
        ng = np.asarray(g['NodeGraph'], dtype)
        out = ng.T @ out
    loss_value, d_out = tro.loss_forward_backward(loss, targets, out, sample_weights, dtype)
    if graph_based: d_out = ng @ d_out
    r = backward(ctx, d_out, None, max_iteration if adjoint_max_iter is None else adjoint_max_iter,
                 threshold if adjoint_threshold is None else adjoint_threshold, iterations_forced)
    r.update(k=float(ctx['k']), state=ctx['state'], out=out, loss=loss_value, ctx=ctx)
    return r


def lgnn_step(g, layers, get_state, get_output, training_mode, state0, masks_state, masks_output, targets, sample_weights,
              loss='categorical_crossentropy', mean=True, graph_based=False, edge_based=False, dtype=np.float64, k_forced=None, iterations_forced=None):
    """Joint step of an LGNN in 'parallel' / 'residual' mode whose layers are fixed-point (layer dict with fixed_point=True, optional
    adjoint_max_iter / adjoint_threshold) or unrolled (the training oracle's layer).  A fixed-point layer's net_state gradients are NOT divided by
    k under ``mean``.  k_forced / iterations_forced: per-layer lists (None entries: own gates).  Returns dict(k, loss, grads_state, grads_output,
    outs, outs_nodes, states, d_nodes, d_arcs (per layer), g, adjoint_iterations, adjoint_converged (None for an unrolled layer))."""
    assert training_mode in ('parallel', 'residual')
    L = len(layers)
    k_forced = k_forced or [None] * L
    iterations_forced = iterations_forced or [None] * L
    nodes0, arcs0 = np.asarray(g['nodes'], dtype), np.asarray(g['arcs'], dtype)
    nlb, alb = nodes0.shape[1], arcs0.shape[1] - 2
    ng = np.asarray(g['NodeGraph'], dtype) if graph_based else None
    ctxs, outs, cur = [], [], g
    for i, ly in enumerate(layers):
        if ly.get('fixed_point'):
            ctx = abm.forward(cur, ly['net_state'], ly['net_output'], ly['state_vect_dim'], ly['max_iteration'], ly['threshold'], state0[i],
                              masks_output[i], dtype, edge_based, k_forced[i])
        else:
            mi, th = (ly['max_iteration'], ly['threshold']) if k_forced[i] is None else (int(k_forced[i]), -1.0)
            ctx = tro.train_forward(cur, ly['net_state'], ly['net_output'], ly['state_vect_dim'], mi, th, state0[i], masks_state[i], masks_output[i],
                                    dtype=dtype, edge_based=edge_based)
        ctxs.append(ctx)
        outs.append(ng.T @ ctx['out_nodes'] if graph_based else ctx['out_nodes'])
        if i < L - 1:
            extra, cur = [], dict(g)
            if get_state: extra.append(ctx['state'])
            if get_output:
                sc = np.zeros((len(ctx['mask']), ctx['out_nodes'].shape[1]), dtype)
                sc[ctx['mask']] = ctx['out_nodes']
                if edge_based: cur['arcs'] = np.concatenate([arcs0, sc], axis=1)
                else: extra.append(sc)
            cur['nodes'] = np.concatenate([nodes0] + extra, axis=1)
    if training_mode == 'residual':
        loss_value, d = tro.loss_forward_backward(loss, targets, np.mean(outs, axis=0), sample_weights, dtype)
        d_outs = [d / L] * L
    else:
        pairs = [tro.loss_forward_backward(loss, targets, o, sample_weights, dtype) for o in outs]
        loss_value = float(np.mean([p[0] for p in pairs]))
        d_outs = [p[1] / L for p in pairs]
    res = dict(k=[float(c['k']) for c in ctxs], loss=loss_value, outs=outs, grads_state=[None] * L, grads_output=[None] * L, d_nodes=[None] * L,
               d_arcs=[None] * L, adjoint_iterations=[None] * L, adjoint_converged=[None] * L, states=[c['state'] for c in ctxs],
               outs_nodes=[c['out_nodes'] for c in ctxs], g=[None] * L)
    d_state_extra = d_out_extra = None
    for i in reversed(range(L)):
        ctx, ly = ctxs[i], layers[i]
        d_nodes_out = ng @ d_outs[i] if graph_based else d_outs[i]
        if d_out_extra is not None: d_nodes_out = d_nodes_out + d_out_extra
        if ly.get('fixed_point'):
            b = backward(ctx, d_nodes_out, d_state_extra, ly.get('adjoint_max_iter') or ly['max_iteration'],
                         ly['threshold'] if ly.get('adjoint_threshold') is None else ly['adjoint_threshold'], iterations_forced[i])
            gs, go, d_nodes, d_arcs = b['grads_state'], b['grads_output'], b['d_nodes'], b['d_arcs']
            res['adjoint_iterations'][i], res['adjoint_converged'][i], res['g'][i] = b['adjoint_iterations'], b['adjoint_converged'], b['g']
        else:
            gs, go, d_nodes, d_arcs = tro.train_backward(ctx, d_nodes_out, d_state_extra, want_d_arcs=True)
            if mean and ctx['k']: gs = [v / ctx['k'] for v in gs]
        res['grads_state'][i], res['grads_output'][i], res['d_nodes'][i], res['d_arcs'][i] = gs, go, d_nodes, d_arcs
        d_state_extra = d_out_extra = None
        if i > 0:
            prev, c = ctxs[i - 1], nlb
            if get_state:
                d_state_extra = d_nodes[:, c:c + prev['state'].shape[1]]
                c += prev['state'].shape[1]
            if get_output:
                t = prev['out_nodes'].shape[1]
                d_out_extra = d_arcs[prev['mask'], alb:alb + t] if edge_based else d_nodes[prev['mask'], c:c + t]
    return res
