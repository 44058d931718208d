"""Label gradients of the fixed-point gradient modes (include/gnn_hip.h: GNN_ADJOINT_LABEL_GRADIENTS) and the LGNN joint steps built on them, without
a device: the float64 mirror (tests/adjoint_labels_mirror.py) against independent witnesses - a dense solve assembled from the layers' formulas,
central finite differences of the loss through the INFERENCE oracle (oracle/gnn_oracle.py), the zero pattern on a graph without cycles - and the
Python surface that needs no GPU.

Finite-difference tolerance (the derivation of tests/test_adjoint_bn_host.py): an entry passes within |q(h) - q(h / 2)| + STOP of q(h / 2), with q the
central quotient.  |q(h) - q(h / 2)| is three times the truncation error of q(h / 2) (error ~ h^2).  STOP is the stopping error of the Loops: every
Loop stops when no node moves by more than 1e-12 of its norm (< 1, asserted); the map contracts by more than a half per body (asserted on the
movement of the last two bodies), so every state row is within 1e-12 of its fixed point, and the loss within 1e-12 x sum |d loss / d p| summed over the
layers (g of every layer, hand-over included) < 3e-12 (asserted).  Two such evaluations over 2 (h / 2) = 2e-4 give STOP = 3e-8."""
import numpy as np
import pytest

import adjoint_labels_mirror as lm
import train_graph_cases as G
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs

H = 2e-4
STOP = 3e-8
T = 2


# ---- problems -----------------------------------------------------------------------------------------------------------------------------------------
def _graph(kind, seed, n=12, nl=2, al=1, arcs=None):
    """Graph dict of a node- ('n'), graph- ('g': two graphs of n / 2 nodes) or edge-based ('a': the masks are over the arcs) problem, its targets and
    sample weights."""
    rng = np.random.default_rng(seed)
    if arcs is None: arcs = random_arcs(rng, n, 2 * n, al)
    ng = None
    if kind == 'g':
        half = n // 2
        arcs = arcs[(arcs[:, 0] // half) == (arcs[:, 1] // half)]
        ng = np.zeros((n, 2), np.float32)
        ng[np.arange(n), np.arange(n) // half] = 1.0 / half
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    rows = len(arcs) if kind == 'a' else n
    g['set_mask'] = np.ones(rows, bool) if kind == 'g' else rng.random(rows) < 0.7
    g['set_mask'][0] = True
    g['output_mask'] = np.ones(rows, bool)
    m = 2 if kind == 'g' else int(g['set_mask'].sum())
    targets = np.eye(T)[rng.integers(0, T, m)]
    weights = rng.uniform(0.5, 1.5, m) / m
    return g, targets, weights


def _nets(rng, kind, ds, nl, al, hidden=(6,), gain=0.5):
    st = make_mlp(rng, al + 2 * (ds + nl), list(hidden) + [ds], 'tanh', gain=gain, batch_normalization=False)
    ou = make_mlp(rng, 2 * (ds + nl) + al if kind == 'a' else ds + nl, [T], 'softmax', batch_normalization=False)
    return st, ou


def _single(kind, seed, n=12, ds=3, nl=2, al=1):
    g, targets, weights = _graph(kind, seed, n, nl, al)
    rng = np.random.default_rng(seed + 100)
    st, ou = _nets(rng, kind, ds, nl, al)
    return dict(kind=kind, g=g, st=st, ou=ou, ds=ds, s0=0.1 * rng.standard_normal((n, ds)), targets=targets, weights=weights)


def _stack(kind, seed, get_state, get_output, layers=3, n=10, ds=3, nl=2, al=1):
    """A stack of `layers` GNNs: layer i > 0 sees [nodes | state? | scattered output?] (edge-based: the output on the arc labels)."""
    g, targets, weights = _graph(kind, seed, n, nl, al)
    rng = np.random.default_rng(seed + 200)
    out, s0 = [], []
    for i in range(layers):
        nl_i = nl + (i > 0) * (get_state * ds + (get_output and kind != 'a') * T)
        al_i = al + (i > 0) * (get_output and kind == 'a') * T
        st, ou = _nets(rng, kind, ds, nl_i, al_i)
        out.append(dict(net_state=st, net_output=ou, state_vect_dim=ds, max_iteration=5000, threshold=1e-12, fixed_point=True,
                        adjoint_max_iter=5000, adjoint_threshold=1e-14))
        s0.append(0.1 * rng.standard_normal((n, ds)))
    return dict(kind=kind, g=g, layers=out, s0=s0, targets=targets, weights=weights)


# ---- the loss through the inference oracle ------------------------------------------------------------------------------------------------------------
def _loss(kind, targets, out, weights):
    return tro.loss_forward_backward('categorical_crossentropy', targets, out, weights, np.float64)[0]


def _inference_loss(p, g=None, st=None):
    fn = {'n': orc.loop_node, 'g': orc.loop_graph, 'a': orc.loop_edge}[p['kind']]
    _, state, out = fn(p['g'] if g is None else g, p['st'] if st is None else st, p['ou'], p['ds'], 5000, 1e-12, p['s0'], dtype=np.float64)
    assert np.abs(state).max() < 1.0
    return _loss(p['kind'], p['targets'], out, p['weights'])


def _inference_outs(p, layers, get_state, get_output):
    """The outputs of every layer through the inference oracle: oracle.gnn_oracle.lgnn_loop for node- and graph-based stacks; its edge-based
    counterpart is the same walk with loop_edge and update_graph_edge (lgnn_loop has no edge form)."""
    if p['kind'] != 'a':
        return orc.lgnn_loop(p['g'], layers, get_state, get_output, p['kind'] == 'g', p['s0'], dtype=np.float64)[2]
    cur, outs = p['g'], []
    for ly, s0 in zip(layers, p['s0']):
        _, state, out = orc.loop_edge(cur, ly['net_state'], ly['net_output'], ly['state_vect_dim'], ly['max_iteration'], ly['threshold'], s0, np.float64)
        outs.append(out)
        cur = orc.update_graph_edge(p['g'], state, out, get_state, get_output, np.float64)
    return outs


def _joint_loss(p, layers, get_state, get_output, mode):
    outs = _inference_outs(p, layers, get_state, get_output)
    if mode == 'residual': return _loss(p['kind'], p['targets'], np.mean(outs, axis=0), p['weights'])
    return float(np.mean([_loss(p['kind'], p['targets'], o, p['weights']) for o in outs]))


def _contraction(g, st, D, s0):
    """Movement of the last body over the movement of the one before, largest row: the factor by which the Loop contracts near its fixed point."""
    n = np.asarray(g['nodes']).shape[0]
    node_side = dict(g, set_mask=np.ones(n, bool), output_mask=np.ones(n, bool))
    dummy = dict(weights=[np.zeros((D + np.asarray(g['nodes']).shape[1], 1)), np.zeros(1)], activations=['linear'], batch_normalization=False)
    trace = orc.loop_node(node_side, st, dummy, D, 5000, 1e-12, s0, np.float64, return_trace=True)[3]
    assert len(trace) > 6
    a, b = np.linalg.norm(trace[-4] - trace[-5], axis=1).max(), np.linalg.norm(trace[-5] - trace[-6], axis=1).max()
    return a / b


def _quotients(f, h=H):
    """Central quotients of f(sign * step) at h and h / 2"""
    return [(f(step) - f(-step)) / (2 * step) for step in (h, h / 2)]


# ---- 1. dense solve -------------------------------------------------------------------------------------------------------------------------------------
def _dense_label_gradients(p, d_out, dse):
    """d_nodes / d_arc_labels = direct part + (d F / d l)^T (I - J^T)^-1 g with every Jacobian assembled densely from the layers' formulas (tanh Dense
    layers, a softmax head), independent of the mirror's backward passes."""
    g, st, ou, ds = p['g'], p['st'], p['ou'], p['ds']
    edge = p['kind'] == 'a'
    nodes, labels = np.asarray(g['nodes'], np.float64), np.asarray(g['arcs'], np.float64)[:, 2:]
    n, nl = nodes.shape
    e_, al = labels.shape
    ip, src, w = g['adjT']
    dst = np.repeat(np.arange(n), np.diff(ip))
    A = np.zeros((n, n)); np.add.at(A, (dst, src), np.asarray(w, np.float64))
    ipa, arc_id, wa = g['arcT']
    B = np.zeros((n, e_)); np.add.at(B, (np.repeat(np.arange(n), np.diff(ipa)), arc_id), np.asarray(wa, np.float64))
    # the fixed point by plain iteration
    W = [np.asarray(v, np.float64) for v in st['weights']]
    state = np.asarray(p['s0'], np.float64)
    for _ in range(3000):
        inp = np.concatenate([state, nodes, A @ state, A @ nodes, B @ labels], axis=1)
        h1 = np.tanh(inp @ W[0] + W[1])
        state = np.tanh(h1 @ W[2] + W[3])
    inp = np.concatenate([state, nodes, A @ state, A @ nodes, B @ labels], axis=1)
    h1 = np.tanh(inp @ W[0] + W[1]); y = np.tanh(h1 @ W[2] + W[3])
    assert np.max(np.abs(y - state)) < 1e-15
    # per-row Jacobian d y_r / d inp_r [n, ds, in_s]
    jrow = np.einsum('ri,ji,rj,kj->rik', 1 - y ** 2, W[2], 1 - h1 ** 2, W[0])
    c_aggs, c_aggn, c_agga = ds + nl, 2 * ds + nl, 2 * ds + 2 * nl
    eye = np.eye(n)
    J = (np.einsum('rs,rij->risj', eye, jrow[:, :, :ds]) + np.einsum('rs,rij->risj', A, jrow[:, :, c_aggs:c_aggs + ds])).reshape(n * ds, n * ds)
    Fn = (np.einsum('rs,ric->risc', eye, jrow[:, :, ds:ds + nl]) + np.einsum('rs,ric->risc', A, jrow[:, :, c_aggn:c_aggn + nl])).reshape(n * ds, n * nl)
    Fa = np.einsum('ra,ric->riac', B, jrow[:, :, c_agga:c_agga + al]).reshape(n * ds, e_ * al)
    # the head: out = softmax(feats Wo + bo), d feats = ((d out - sum(d out . out)) . out) Wo^T
    Wo, bo = (np.asarray(v, np.float64) for v in ou['weights'][:2])
    mask = g['set_mask'] & g['output_mask']
    F = np.concatenate([state, nodes], axis=1)
    feats = np.concatenate([F[dst], F[src], labels], axis=1)[mask] if edge else F[mask]
    logits = feats @ Wo + bo
    out = np.exp(logits - logits.max(axis=1, keepdims=True)); out /= out.sum(axis=1, keepdims=True)
    d_feats = ((d_out - np.sum(d_out * out, axis=1, keepdims=True)) * out) @ Wo.T
    gs, direct_n, direct_a = np.array(dse, np.float64), np.zeros((n, nl)), np.zeros((e_, al))
    if edge:
        wn = ds + nl
        np.add.at(gs, dst[mask], d_feats[:, :ds]); np.add.at(gs, src[mask], d_feats[:, wn:wn + ds])
        np.add.at(direct_n, dst[mask], d_feats[:, ds:wn]); np.add.at(direct_n, src[mask], d_feats[:, wn + ds:2 * wn])
        direct_a[np.nonzero(mask)[0]] = d_feats[:, 2 * wn:]
    else:
        gs[mask] += d_feats[:, :ds]
        direct_n[mask] = d_feats[:, ds:]
    assert np.max(np.abs(np.linalg.eigvals(J))) < 1.0
    z = np.linalg.solve(np.eye(n * ds) - J.T, gs.ravel())
    return direct_n + (Fn.T @ z).reshape(n, nl), direct_a + (Fa.T @ z).reshape(e_, al), z.reshape(n, ds)


@pytest.mark.parametrize('kind', ['n', 'a'])
def test_mirror_against_the_dense_solve(kind):
    """d_nodes / d_arc_labels of the mirror = direct part + (dF/dl)^T (I - J^T)^-1 g assembled densely, to 1e-10 (the bound of the existing mirror
    tests), with a d_state_extra on every row."""
    p = _single(kind, 31)
    rng = np.random.default_rng(2)
    m = int((p['g']['set_mask'] & p['g']['output_mask']).sum())
    d_out, dse = rng.standard_normal((m, T)), rng.standard_normal(p['s0'].shape)
    r = lm.halves(p['g'], p['st'], p['ou'], p['ds'], 5000, 1e-15, p['s0'], {}, d_out, dse, edge_based=kind == 'a', adjoint_max_iter=5000,
                  adjoint_threshold=1e-16)
    assert r['adjoint_converged'] and r['adjoint_iterations'] > 3
    d_nodes, d_arcs, z = _dense_label_gradients(p, d_out, dse)
    assert np.max(np.abs(r['z'] - z)) <= 1e-10 * np.max(np.abs(z))
    assert np.abs(d_nodes).max() > 0.1 and np.abs(d_arcs).max() > 0.01
    assert np.max(np.abs(r['d_nodes'] - d_nodes)) <= 1e-10 * np.max(np.abs(d_nodes))
    assert np.max(np.abs(r['d_arcs'] - d_arcs)) <= 1e-10 * np.max(np.abs(d_arcs))


# ---- 2. finite differences, single GNN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['n', 'g', 'a'])
def test_label_gradients_against_finite_differences(kind):
    """Five node-label entries and five arc-label entries per model type (tolerance: module docstring).  Measured: the largest |q(h) - q(h / 2)| is
    2.3e-11, the largest distance 6.4e-12 (a third of it, as the h^2 law says), on gradients up to 0.036: six orders above the bound."""
    p = _single(kind, 41)
    g = p['g']
    r = lm.step(g, p['st'], p['ou'], p['ds'], 5000, 1e-12, p['s0'], {}, p['targets'], p['weights'], graph_based=kind == 'g', edge_based=kind == 'a',
                adjoint_max_iter=5000, adjoint_threshold=1e-14)
    assert r['adjoint_converged'] and r['k'] > 3 and np.abs(r['g']).sum() < 3.0 and _contraction(g, p['st'], p['ds'], p['s0']) < 0.5
    assert abs(r['loss'] - _inference_loss(p)) <= 1e-12
    rng = np.random.default_rng(3)
    nodes64, arcs64 = np.asarray(g['nodes'], np.float64), np.asarray(g['arcs'], np.float64)
    worst_step = worst = top = 0.0
    for which, base, grad in (('nodes', nodes64, r['d_nodes']), ('arcs', arcs64, r['d_arcs'])):
        for _ in range(5):
            idx = tuple(int(rng.integers(0, d)) for d in grad.shape)
            def f(step):
                a = base.copy()
                a[idx[0], idx[1] + (2 if which == 'arcs' else 0)] += step
                return _inference_loss(p, g=dict(g, **{which: a}))
            q = _quotients(f)
            got = grad[idx]
            print(f'{kind} {which}{idx}: mirror {got:+.10e}  fd(h/2) {q[1]:+.10e}  |fd(h) - fd(h/2)| {abs(q[0] - q[1]):.2e}  distance {abs(got - q[1]):.2e}')
            worst_step, worst, top = max(worst_step, abs(q[0] - q[1])), max(worst, abs(got - q[1])), max(top, abs(got))
            assert abs(got - q[1]) <= abs(q[0] - q[1]) + STOP, (which, idx, got, q)
    print(f'largest |fd(h) - fd(h/2)| {worst_step:.2e}, largest distance {worst:.2e}, largest gradient {top:.2e}')
    assert top > 0.01


# ---- 3. finite differences, LGNN joint loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['n', 'g', 'a'])
@pytest.mark.parametrize('get_state,get_output', [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_joint_gradients_against_finite_differences(mode, get_state, get_output, kind):
    """The JOINT loss of a 3-layer stack through the inference oracle, for weight entries of every net: four per array of layer 0's net_state - which
    the loss of layers 1 and 2 reaches only through the hand-over of the label gradients - and one per array elsewhere (tolerance: module
    docstring).  Measured over the 18 cases: the largest |q(h) - q(h / 2)| is 1.1e-9, the largest distance 3.7e-10; the largest
    gradient entry of layer 0's net_state is between 3.4e-3 and 8.9e-2 per case."""
    p = _stack(kind, 51, get_state, get_output)
    layers = p['layers']
    r = lm.lgnn_step(p['g'], layers, get_state, get_output, mode, p['s0'], [None] * 3, [{}] * 3, p['targets'], p['weights'], mean=True,
                     graph_based=kind == 'g', edge_based=kind == 'a')
    assert all(r['adjoint_converged']) and min(r['k']) > 3 and sum(np.abs(x).sum() for x in r['g']) < 3.0
    assert abs(r['loss'] - _joint_loss(p, layers, get_state, get_output, mode)) <= 1e-12
    cur = p['g']
    for i, ly in enumerate(layers):           # every layer's Loop contracts by more than a half per body, on the labels it sees
        assert _contraction(cur, ly['net_state'], ly['state_vect_dim'], p['s0'][i]) < 0.5
        if i < 2:
            upd = orc.update_graph_edge if kind == 'a' else orc.update_graph
            cur = upd(p['g'], r['states'][i], r['outs_nodes'][i], get_state, get_output, np.float64)
    rng = np.random.default_rng(4)
    worst_step = worst = top0 = 0.0
    for li in range(3):
        for net, key in (('net_state', 'grads_state'), ('net_output', 'grads_output')):
            for ai, arr in enumerate(layers[li][net]['weights']):
                for _ in range(4 if (li == 0 and net == 'net_state') else 1):
                    idx = tuple(int(rng.integers(0, d)) for d in arr.shape)
                    def f(step):
                        ws = [np.asarray(v, np.float64).copy() for v in layers[li][net]['weights']]
                        ws[ai][idx] += step
                        changed = list(layers)
                        changed[li] = dict(layers[li], **{net: dict(layers[li][net], weights=ws)})
                        return _joint_loss(p, changed, get_state, get_output, mode)
                    q = _quotients(f)
                    got = r[key][li][ai][idx]
                    print(f'layer {li} {net}[{ai}]{idx}: mirror {got:+.10e}  fd(h/2) {q[1]:+.10e}  |fd(h) - fd(h/2)| {abs(q[0] - q[1]):.2e}  distance {abs(got - q[1]):.2e}')
                    worst_step, worst = max(worst_step, abs(q[0] - q[1])), max(worst, abs(got - q[1]))
                    if li == 0 and net == 'net_state': top0 = max(top0, abs(got))
                    assert abs(got - q[1]) <= abs(q[0] - q[1]) + STOP, (li, net, ai, idx, got, q)
    print(f'largest |fd(h) - fd(h/2)| {worst_step:.2e}, largest distance {worst:.2e}, largest gradient of layer 0\'s net_state {top0:.2e}')
    assert top0 > 1e-4


# ---- 4. direction -----------------------------------------------------------------------------------------------------------------------------------------
def dag_problem(seed=61, n=30, ds=3, nl=2, al=1):
    """A directed graph without cycles (every arc goes from a lower to a higher node), and the node `t` that alone carries a state gradient."""
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 2 * n, al, symmetric=False)
    assert (arcs[:, 0] < arcs[:, 1]).all()
    g, targets, weights = _graph('n', seed, n, nl, al, arcs=arcs)
    st, ou = _nets(rng, 'n', ds, nl, al)
    t = 22                                                      # (seven ancestors, eight descendants with the default seed)
    anc = G.predecessors(arcs, [t], n, n)
    desc = G.successors(arcs, [t], n, n)
    assert 3 <= anc.sum() < n - 3 and desc.sum() > 3 and (desc & ~anc).sum() > 2
    return dict(kind='n', g=g, st=st, ou=ou, ds=ds, s0=0.1 * rng.standard_normal((n, ds)), t=t, ancestors=anc, n=n)


def test_label_gradient_reaches_the_ancestors_only():
    """g on one node of a graph without cycles: the rows of d_nodes of its ancestors (and its own) are non-zero, every other row is EXACTLY zero - the
    node's descendants included, which a by-source / by-destination swap would fill instead."""
    p = dag_problem()
    m = int((p['g']['set_mask'] & p['g']['output_mask']).sum())
    dse = np.zeros((p['n'], p['ds'])); dse[p['t']] = [0.7, -0.4, 0.9]
    r = lm.halves(p['g'], p['st'], p['ou'], p['ds'], 200, 1e-13, p['s0'], {}, np.zeros((m, T)), dse, adjoint_max_iter=200, adjoint_threshold=0.0)
    assert r['adjoint_converged']                               # (J is nilpotent: the sum ends after the longest path)
    hit = np.abs(r['d_nodes']).max(axis=1) > 0
    assert np.array_equal(hit, p['ancestors']), (np.nonzero(hit)[0], np.nonzero(p['ancestors'])[0])
    assert np.abs(r['d_nodes'][p['ancestors']]).max(axis=1).min() > 1e-8


# ---- 5. Python surface ------------------------------------------------------------------------------------------------------------------------------------
def _model(cls=None, ds=3, layer=0, bn=False):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (ds + 3 + extra), [8, ds if ds else 3 + extra], 'tanh', 'glorot_normal', 'zeros', batch_normalization=bn)
    ou = MLP(ds + 3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=ds, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_keyword_validation_and_flags():
    from GNN import _engine as e
    assert 'gnn_loop_train_backward_chained' in e.EXPORTS and e.ADJOINT_LABEL_GRADIENTS == 2
    assert (e.KEEP_D_NODES, e.KEEP_D_ARC_LABELS) == (1, 2)
    assert [e.adjoint_flags(None), e.adjoint_flags('frozen'), e.adjoint_flags(None, True), e.adjoint_flags('frozen', True)] == [0, 1, 2, 3]
    with pytest.raises(ValueError): e.adjoint_flags(None, 'yes')
    gnn = _model()
    assert gnn.adjoint_label_gradients is False
    gnn.set_gradient_mode('fixed_point', label_gradients=True)
    assert gnn.adjoint_label_gradients is True and gnn._gradient_config()['label_gradients'] is True
    with pytest.raises(ValueError): gnn.set_gradient_mode('fixed_point', label_gradients=1)
    assert gnn.adjoint_label_gradients is True                            # a refused call leaves the setting
    gnn.set_gradient_mode('fixed_point')
    assert gnn.adjoint_label_gradients is False
    with pytest.raises(NotImplementedError, match='state_vect_dim'): _model(ds=0).set_gradient_mode('fixed_point', label_gradients=True)
    _model(ds=0).set_gradient_mode('unrolled', label_gradients=True)      # (the keyword belongs to the fixed-point mode)
    both = _model(bn=True)
    both.set_gradient_mode('fixed_point', batch_normalization='frozen', label_gradients=True)
    assert both._gradient_config() == dict(mode='fixed_point', max_iteration=None, threshold=None, batch_normalization='frozen', label_gradients=True)
    # gnn_adjoint_form_ex accepts the flag; the forms do not change
    import ctypes as C
    dims, acts, rates, out_a, out_b = np.array([11, 8, 4], np.int32), np.array([4, 4], np.int32), np.zeros(3, np.float32), np.zeros(6, np.int32), np.zeros(6, np.int32)
    ip, fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)), lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert e.lib().gnn_adjoint_form_ex(2, ip(dims), ip(acts), fp(rates), 0, 0, C.c_int64(100), ip(out_a)) == 0
    assert e.lib().gnn_adjoint_form_ex(2, ip(dims), ip(acts), fp(rates), 0, 2, C.c_int64(100), ip(out_b)) == 0 and np.array_equal(out_a, out_b)
    assert e.lib().gnn_adjoint_form_ex(2, ip(dims), ip(acts), fp(rates), 0, 4, C.c_int64(100), ip(out_b)) != 0


def test_copy_lko_save_load_keep_the_keyword(tmp_path):
    import json
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    for cls in (None, GNNgraphBased, GNNedgeBased):
        gnn = _model(cls)
        gnn.set_gradient_mode('fixed_point', 25, 1e-3, label_gradients=True)
        want = dict(mode='fixed_point', max_iteration=25, threshold=1e-3, label_gradients=True)
        twin = gnn.copy(copy_weights=False)                               # (LKO builds its models with copy())
        assert type(twin) is type(gnn) and twin._gradient_config() == gnn._gradient_config() == want and twin.adjoint_label_gradients is True
        path = str(tmp_path / f'model{cls.__name__ if cls else ""}')
        gnn.save(path)
        with open(f'{path}/config.json') as f: assert json.load(f)['gradient_mode'] == want
        assert type(gnn).load(path)._gradient_config() == want


def test_a_config_without_the_keyword_is_what_it_was(tmp_path):
    """The key is written only when set: _gradient_config() and the saved file of a model without it do not name it."""
    import json
    for kw in (dict(), dict(batch_normalization='frozen')):
        gnn = _model(bn=bool(kw))
        gnn.set_gradient_mode('fixed_point', 25, 1e-3, **kw)
        assert list(gnn._gradient_config()) == ['mode', 'max_iteration', 'threshold'] + list(kw)
        path = str(tmp_path / f'plain{len(kw)}')
        gnn.save(path)
        with open(f'{path}/config.json') as f: text = f.read()
        assert 'label_gradients' not in text and json.loads(text)['gradient_mode'] == gnn._gradient_config()
        assert type(gnn).load(path).adjoint_label_gradients is False
    assert 'label_gradients' not in _model()._gradient_config()


def test_lgnn_forwards_the_keyword_and_refuses_without_it(tmp_path):
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    lgnn = LGNN([_model(), _model(layer=1)], get_state=False, get_output=True, optimizer=optimizers.Adam(0.02),
                loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    assert lgnn.device_chain is True
    lgnn.set_gradient_mode('fixed_point', 20, label_gradients=True)
    assert [(g.gradient_mode, g.adjoint_label_gradients, g.adjoint_max_iteration) for g in lgnn.gnns] == [('fixed_point', True, 20)] * 2
    assert [g.adjoint_label_gradients for g in lgnn.copy().gnns] == [True] * 2
    lgnn.save(str(tmp_path / 'stack'))
    assert [g._gradient_config().get('label_gradients') for g in LGNN.load(str(tmp_path / 'stack')).gnns] == [True] * 2
    # one layer without the keyword: both joint modes refuse as before, naming the mode
    lgnn.gnns[1].set_gradient_mode('fixed_point', 20)
    for mode in ('parallel', 'residual'):
        lgnn.training_mode = mode
        with pytest.raises(NotImplementedError, match='fixed_point'): lgnn.training_step(None, mean=True)
    # with it on every fixed-point layer the refusal is gone (the step then fails on the missing batch, not on the mode)
    lgnn.gnns[1].set_gradient_mode('fixed_point', 20, label_gradients=True)
    lgnn.gnns[0].set_gradient_mode('unrolled')                            # a mixed stack is allowed
    with pytest.raises(Exception) as err: lgnn.training_step(None, mean=True)
    assert not isinstance(err.value, NotImplementedError)
