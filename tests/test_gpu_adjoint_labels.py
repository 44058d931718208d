"""Label gradients of the fixed-point gradient modes (gnn_loop_set_gradient_mode_ex with GNN_ADJOINT_LABEL_GRADIENTS), the chained backward pass
(gnn_loop_train_backward_chained) and the LGNN joint steps built on them, on the device against the float64 mirror (tests/adjoint_labels_mirror.py,
held to independent witnesses by tests/test_adjoint_labels_host.py).

Criterion: check_tight of tests/test_gpu_adjoint.py (its MARGIN, FLOOR and ratio file), over every array INCLUDING d_nodes / d_arc_labels: the mirror
is evaluated a second time in float32; an array passes when every element lies within MARGIN x max |mirror_f32 - mirror_f64| over that array plus
FLOOR x max |mirror_f64|.  No gate decision enters a comparison: the mirror runs the device's k bodies and the device's count of adjoint iterations
(per layer, for a stack).  GNN_ADJOINT_RATIOS=<file> appends every line; a line ends in 'floor-only' when the array passes by the floor alone (its
error is above MARGIN x noise): 5 of the 627 arrays measured (profiles/fixed_point_lgnn.txt).  The forward runs on impl 1, as there.

The mixed stack (layer 0 unrolled, with Dropout and training-mode BatchNormalization in net_state) runs under the same criterion, the float32 mirror
running the unrolled layer in float32 as well: none of its arrays needs another bound (largest measured ratio 1.28 over its 32 arrays).
Measured over the module: 627 arrays, largest ratio 6.58 among the 622 that do not need the floor."""
import numpy as np
import pytest

import adjoint_bn_cases as C
import adjoint_labels_mirror as lm
import test_gpu_adjoint as ga
import train_graph_cases as G
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = ga.MARGIN, ga.FLOOR
T = 2


def check_tight(tag, got, want, noisy):
    """The criterion of tests/test_gpu_adjoint.py::check_tight over dicts name -> array (device, mirror float64, mirror float32).  Every line is
    printed and recorded before anything is asserted."""
    assert list(got) == list(want) == list(noisy)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(want[key], np.float64)
        a = np.asarray(a)
        assert a.shape == w.shape, (key, a.shape, w.shape)
        noise = float(np.max(np.abs(np.asarray(noisy[key], np.float64) - w))) if w.size else 0.0
        top = float(np.max(np.abs(w))) if w.size else 0.0
        diff = np.abs(a.astype(np.float64) - w)
        err = float(np.max(diff)) if w.size else 0.0
        ok = (not w.size) or bool(np.all(diff <= MARGIN * noise + FLOOR * top))
        by_floor = ok and w.size and err > MARGIN * noise
        lines.append(f'{tag:44s} {key:18s} err {err:9.3e}  noise {noise:9.3e}  ratio {err / noise if noise > 0 else float("nan"):6.2f}  floor {FLOOR * top:9.3e}  '
                     f'max|ref| {top:9.3e}{"  floor-only" if by_floor else ""}')
        if not ok: bad.append(lines[-1])
    ga.record(lines)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)


def same_bits(a, b):
    assert list(a) == list(b)
    for key in a: assert np.array_equal(a[key], b[key]), key


# ---- C level ------------------------------------------------------------------------------------------------------------------------------------------------
def edge_problem(seed, n, ds, nl=3, al=2, hidden=(7,), gain=0.5):
    """An edge-based problem on a directed, unsorted arc list (tests/train_graph_cases.py): the masks are over the arcs."""
    rng = np.random.default_rng(seed)
    arcs = G.directed_graph(seed, n, degrees=True, al=al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'], g['output_mask'] = G.edge_mask(arcs, n, seed)[0], np.ones(len(arcs), bool)
    st = make_mlp(rng, al + 2 * (ds + nl), list(hidden) + [ds], 'tanh', gain=gain, batch_normalization=False)
    ou = make_mlp(rng, 2 * (ds + nl) + al, [T], 'softmax', batch_normalization=False)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    return dict(g=g, st=st, ou=ou, ds=ds, D=ds, s0=s0, n=n, edge=True)


class Device:
    """The loop of a problem on the device in a fixed-point mode (or unrolled: mode 0), node- or edge-based."""

    def __init__(self, pb, max_iter, thr, mode=1, label_gradients=True, graph=None, own_labels=False):
        from GNN import _engine as e
        g, n = pb['g'], pb['n']
        self.edge = bool(pb.get('edge'))
        labels = np.asarray(g['arcs'])[:, 2:]
        self.owns_graph = graph is None
        if graph is None:
            node_mask = np.ones(n, bool) if self.edge else g['set_mask'] & g['output_mask']
            graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], labels[g['arcT'][1]], g['nodes'], node_mask)
            if self.edge: graph.set_arc_order(g['arcT'][1], labels)
        self.graph = graph
        bn = pb['st']['batch_normalization']
        self.mst = e.Mlp(pb['st']['weights'], pb['st']['activations'], bn)
        self.mou = e.Mlp(pb['ou']['weights'], pb['ou']['activations'], pb['ou']['batch_normalization'])
        self.loop = e.Loop(graph, self.mst, self.mou, pb['D'], max_iter, thr)
        if pb['D']: self.loop.set_state0(pb['s0'])
        if self.edge:
            entry_dst = np.repeat(np.arange(n, dtype=np.int32), np.diff(g['adjT'][0]))
            self.loop.set_edge_readout(entry_dst, None if own_labels else labels, g['set_mask'])
        self.loop.set_impl(1)
        if mode: self.loop.set_gradient_mode(mode, batch_normalization='frozen' if bn else None, label_gradients=label_gradients)
        self.pb, self.mode = pb, mode
        self.m = int((g['set_mask'] & g['output_mask']).sum())

    def forward(self):
        k, out = self.loop.train_forward(self.mst, self.mou, None)
        return k, out, self.loop.state()

    def halves(self, d_out, dse=None):
        k, out, state = self.forward()
        res = self.loop.train_backward(d_out, dse, want_d_nodes=True, want_d_arcs=self.edge)
        return self.result(k, out, state, res)

    def result(self, k, out, state, res):
        r = dict(k=k, arrays=arrays(dict(state=state, out=out, **res), self.edge and res.get('d_arcs') is not None, res.get('d_nodes') is not None))
        if self.mode: r['info'] = self.loop.adjoint_info()
        return r

    def close(self):
        self.loop.close()
        if self.owns_graph: self.graph.close()


def arrays(r, with_arcs, with_nodes=True):
    out = {'state': r['state'], 'out': r['out']}
    if with_nodes: out['d_nodes'] = r['d_nodes']
    if with_arcs: out['d_arcs'] = r['d_arcs']
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def incoming(pb, seed, extra):
    rng = np.random.default_rng(seed)
    m = int((pb['g']['set_mask'] & pb['g']['output_mask']).sum())
    d_out = rng.standard_normal((m, T)).astype(np.float32)
    return d_out, (rng.standard_normal((pb['n'], pb['ds'])).astype(np.float32) if extra else None)


def mirror_halves(pb, max_iter, thr, d_out, dse, k, iterations):
    out = []
    for dt in (np.float64, np.float32):
        r = lm.halves(pb['g'], pb['st'], pb['ou'], pb['D'], max_iter, thr, pb['s0'], {}, d_out, dse, edge_based=bool(pb.get('edge')), dtype=dt,
                      k_forced=k, iterations_forced=iterations)
        out.append(arrays(r, bool(pb.get('edge'))))
    return out


MAX_ITER, THR = 50, 1e-3
# rows 1 (no arc), 15 | 16 | 17 (the 16 rows of a block of the one-launch iteration), 37 with an isolated node, 83 with a 70-arc hub and rows outside the
# mask; NL 1 and 5, AL 0 and 2, Ds 3 and 8; with and without d_state_extra; a frozen BatchNormalization; edge-based on a directed, unsorted list
CASES = {
    'n1': lambda: ga.problem(11, n=1, ds=3),
    'n15_nl1_al0': lambda: ga.problem(12, n=15, ds=3, nl=1, al=0),
    'n16_ds8_al2': lambda: ga.problem(13, n=16, ds=8, nl=5, al=2),
    'n17': lambda: ga.problem(14, n=17, ds=3, nl=5, al=0),
    'n37_isolated': lambda: ga.problem(15, n=37, ds=8, nl=1, al=2, isolated=True),
    'n37_directed': lambda: C.problem(16, n=37, ds=3, nl=5, al=2, gain=0.5, bn=False),
    'n83_hub70': lambda: ga.problem(17, n=83, ds=8, nl=5, al=2, hub=70, isolated=True, mask_p=0.5),
    'n83_hub70_ds3': lambda: ga.problem(18, n=83, ds=3, nl=1, al=0, hub=70, hidden=()),
    'n37_frozen_bn': lambda: C.problem(19, n=37, ds=8, nl=5, al=2),
    'n17_frozen_bn': lambda: C.problem(20, n=17, ds=3, nl=1, al=1),
    'edge37': lambda: edge_problem(21, 37, 4),
    'edge83_ds3': lambda: edge_problem(22, 83, 3, nl=1, al=2),
}
EXTRA = {'n1', 'n16_ds8_al2', 'n37_directed', 'n83_hub70', 'n37_frozen_bn', 'edge37'}       # these cases carry a d_state_extra


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', list(CASES))
def test_label_gradients_tight(case, mode):
    """Every array of forward + backward with d_nodes (edge-based: and d_arc_labels) under the criterion; two identical steps give identical bits."""
    pb = CASES[case]()
    d_out, dse = incoming(pb, 5, case in EXTRA)
    dev = Device(pb, MAX_ITER, THR, mode=mode)
    res, again = dev.halves(d_out, dse), dev.halves(d_out, dse)
    assert res['info']['converged'] and (pb['n'] == 1 or res['info']['iterations'] >= 2), res['info']
    want, noisy = mirror_halves(pb, MAX_ITER, THR, d_out, dse, int(res['k']), res['info']['iterations'])
    assert np.abs(want['d_nodes']).max() > 1e-3 and ('d_arcs' not in want or np.abs(want['d_arcs']).max() > 1e-3)
    check_tight(f'labels {case} mode {mode}', res['arrays'], want, noisy)
    same_bits(res['arrays'], again['arrays'])
    assert again['info'] == res['info'] and again['k'] == res['k']
    dev.close()


@pytest.mark.parametrize('dims,backward,gather', [((135, 128, 128, 64), ['chain3'] * 3, 'rows_aligned'), ((135, 144, 64), ['wide'] * 2, 'rows')],
                         ids=['chain3', 'wide'])
def test_label_columns_of_the_matrix_core_backward_forms(dims, backward, gather):
    """4,113 rows on the three-layer chain (k_bwd3_split) and the wide per-layer products (the shapes of FORMS in tests/test_gpu_adjoint.py): the label
    columns of d concat come from those forms."""
    pb = ga.wide_problem(dims, 4113)
    d_out, dse = incoming(pb, 6, True)
    d_out /= 64; dse /= 64                                     # (gradients of the small cases' size over ~2,900 masked rows)
    dev = Device(pb, 30, 1e-2)
    res = dev.halves(d_out, dse)
    assert res['info']['gather'] == gather and dev.loop.train_forms(0)['backward'] == backward
    want, noisy = mirror_halves(pb, 30, 1e-2, d_out, dse, int(res['k']), res['info']['iterations'])
    check_tight(f'labels {"x".join(map(str, dims))} n4113', res['arrays'], want, noisy)
    dev.close()


@pytest.mark.parametrize('mode', [1, 2])
def test_label_gradient_reaches_the_ancestors_only(mode):
    """g on one node of a graph without cycles: on the device too the rows of d_nodes of its ancestors are non-zero and every other row is EXACTLY zero."""
    from test_adjoint_labels_host import dag_problem
    p = dag_problem()
    pb = dict(g=p['g'], st=p['st'], ou=p['ou'], ds=p['ds'], D=p['ds'], s0=p['s0'].astype(np.float32), n=p['n'])
    m = int((p['g']['set_mask'] & p['g']['output_mask']).sum())
    dse = np.zeros((p['n'], p['ds']), np.float32); dse[p['t']] = [0.7, -0.4, 0.9]
    dev = Device(pb, 200, 1e-6, mode=mode)
    res = dev.halves(np.zeros((m, T), np.float32), dse)
    hit = np.abs(res['arrays']['d_nodes']).max(axis=1) > 0
    assert res['info']['converged'] and np.array_equal(hit, p['ancestors']), (np.nonzero(hit)[0], np.nonzero(p['ancestors'])[0])
    dev.close()


def test_refusals():
    """state_vect_dim == 0 stays refused with the flag; without the flag d_nodes / d_arc_labels and kept label gradients are refused as before."""
    pb = ga.problem(51, n=45, ds=3, nl=3, D=0)
    d_out, dse = incoming(pb, 7, True)
    dev = Device(pb, 40, 1e-3)
    dev.forward()
    with pytest.raises(NotImplementedError, match='state_vect_dim == 0'): dev.loop.train_backward(d_out, dse, want_d_nodes=True)
    with pytest.raises(NotImplementedError, match='state_vect_dim == 0'): dev.loop.train_backward_chained(d_out, keep_label_gradients=True)
    plain = dev.loop.train_backward(d_out, dse)                  # (a refused call spends nothing: the backward pass without labels still runs)
    assert np.abs(plain['grads_state'][0]).max() > 0
    dev.close()
    for pb, arcs in ((ga.problem(52, n=20, ds=4), False), (edge_problem(53, 37, 4), True)):
        d_out, dse = incoming(pb, 8, False)
        dev = Device(pb, 40, 1e-3, label_gradients=False)
        dev.forward()
        with pytest.raises(NotImplementedError, match='returns no d_nodes / d_arc_labels'): dev.loop.train_backward(d_out, want_d_nodes=True)
        if arcs:
            with pytest.raises(NotImplementedError, match='returns no d_nodes / d_arc_labels'): dev.loop.train_backward(d_out, want_d_arcs=True)
        with pytest.raises(NotImplementedError, match='returns no d_nodes / d_arc_labels'): dev.loop.train_backward_chained(d_out, keep_label_gradients=True)
        dev.close()


# ---- chained backward ---------------------------------------------------------------------------------------------------------------------------------------
def pair_problem(seed, edge, get_state, get_output, n=61, ds=4, nl=3, al=2):
    """Two layers on one graph: layer 1 sees [nodes | layer 0's state? | its scattered outputs?] (edge-based: the outputs on the arc labels)."""
    lower = edge_problem(seed, n, ds, nl, al) if edge else C.problem(seed, n=n, ds=ds, nl=nl, al=al, gain=0.5, bn=False)
    lower['edge'] = edge
    rng = np.random.default_rng(seed + 1)
    nl1 = nl + get_state * ds + (get_output and not edge) * T
    al1 = al + (get_output and edge) * T
    st = make_mlp(rng, al1 + 2 * (ds + nl1), [7, ds], 'tanh', gain=0.5, batch_normalization=False)
    ou = make_mlp(rng, 2 * (ds + nl1) + al1 if edge else ds + nl1, [T], 'softmax', batch_normalization=False)
    upper = dict(lower, st=st, ou=ou, s0=(0.1 * rng.standard_normal((n, ds))).astype(np.float32))
    return lower, upper, nl, al


@pytest.mark.parametrize('edge', [False, True], ids=['node', 'edge'])
@pytest.mark.parametrize('mode,get_state,get_output', [(1, True, False), (1, False, True), (1, True, True), (0, True, True)],
                         ids=['fixed_point-state', 'fixed_point-output', 'fixed_point-both', 'unrolled-both'])
def test_chained_backward_equals_the_host_chain(mode, get_state, get_output, edge):
    """train_backward_chained against the pair of train_backward calls chained through host arrays: every gradient array of both layers, bit for bit -
    in the fixed-point mode and (one setting per model type) in the unrolled mode, where the call works as well."""
    lower, upper, nlb, alb = pair_problem(71, edge, get_state, get_output)
    d0 = Device(lower, 30, 1e-3, mode=mode)
    derived = d0.graph.derive_edge(get_state * lower['ds'], get_output * T) if edge else d0.graph.derive(get_state * lower['ds'] + get_output * T)
    d1 = Device(upper, 30, 1e-3, mode=mode, graph=derived, own_labels=True)
    rng = np.random.default_rng(9)
    d_out0, d_out1 = (rng.standard_normal((d0.m, T)).astype(np.float32) for _ in range(2))
    mask = lower['g']['set_mask'] & lower['g']['output_mask']

    def forward():
        d0.forward()
        derived.update_labels(d0.graph, d0.loop, get_state, get_output)
        d1.forward()

    forward()
    r1 = d1.loop.train_backward(d_out1, want_d_nodes=get_state or not edge, want_d_arcs=edge and get_output)
    c = nlb
    dse = extra = None
    if get_state:
        dse = r1['d_nodes'][:, c:c + lower['ds']]
        c += lower['ds']
    if get_output: extra = r1['d_arcs'][mask, alb:alb + T] if edge else r1['d_nodes'][mask, c:c + T]
    r0 = d0.loop.train_backward(d_out0 + extra if extra is not None else d_out0, dse)
    assert (dse is None or np.abs(dse).max() > 0) and (extra is None or np.abs(extra).max() > 0)
    forward()
    from GNN import _engine as e
    keep = (e.KEEP_D_NODES if get_state or (get_output and not edge) else 0) | (e.KEEP_D_ARC_LABELS if get_output and edge else 0)
    c1 = d1.loop.train_backward_chained(d_out1, keep_label_gradients=keep)      # (only what layer 0 reads)
    c0 = d0.loop.train_backward_chained(d_out0, d1.loop, get_state, get_output)
    for host, dev in ((r1, c1), (r0, c0)):
        for key in ('grads_state', 'grads_output'):
            for a, b in zip(host[key], dev[key]): assert np.array_equal(a, b), key
    # a loop that kept nothing, or not the array that is read, cannot be chained from
    forward()
    d1.loop.train_backward(d_out1)
    with pytest.raises(Exception, match='kept no'): d0.loop.train_backward_chained(d_out0, d1.loop, get_state, get_output)
    forward()
    d1.loop.train_backward_chained(d_out1, keep_label_gradients=(e.KEEP_D_NODES | e.KEEP_D_ARC_LABELS) & ~keep if edge else 0)
    with pytest.raises(Exception, match='kept no'): d0.loop.train_backward_chained(d_out0, d1.loop, get_state, get_output)
    d1.close(); derived.close(); d0.close()


def test_chained_backward_checks_its_arguments():
    lower, upper, _, _ = pair_problem(72, False, True, True)
    d0 = Device(lower, 30, 1e-3)
    other = Device(ga.problem(73, n=20, ds=4), 30, 1e-3)       # another row count
    same = Device(lower, 30, 1e-3)                                # the base labels: too narrow to hold a state and outputs
    d_out = np.zeros((d0.m, T), np.float32)
    for nxt in (other, same):
        d0.forward(); nxt.forward()
        nxt.loop.train_backward_chained(np.zeros((nxt.m, T), np.float32), keep_label_gradients=True)
        with pytest.raises(ValueError): d0.loop.train_backward_chained(d_out, nxt.loop, True, True)
    with pytest.raises(ValueError): d0.loop.train_backward_chained(d_out, d0.loop, True, True)
    for d in (d0, other, same): d.close()


# ---- LGNN -------------------------------------------------------------------------------------------------------------------------------------------------
LR = 0.05


def stack(kind, get_state, get_output, layers, mode, device_optimizer=False, device_chain=True, mixed=False, frozen=False, seed=81):
    """An LGNN of fixed-point layers with label gradients (mixed: layer 0 unrolled, with Dropout and BatchNormalization in net_state, four bodies;
    frozen: every net_state ends in a BatchNormalization with the arrays of tests/adjoint_bn_cases.py, run on its moving statistics), its
    batch - about 80 nodes; graph-based: a merged batch of 6 graphs of 14 nodes - and the mirror's inputs."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased, GNNedgeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(seed)
    n, nl, al, ds = (84 if kind == 'g' else 77), 3, 2, 4
    arcs = random_arcs(rng, n, 2 * n, al)
    ng = None
    if kind == 'g':
        arcs = arcs[(arcs[:, 0] // 14) == (arcs[:, 1] // 14)]
        ng = np.zeros((n, 6), np.float32)
        ng[np.arange(n), np.arange(n) // 14] = 1.0 / 14
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    rows = len(arcs) if kind == 'a' else n
    set_mask = np.ones(rows, bool) if kind == 'g' else rng.random(rows) < 0.75
    n_t = 6 if kind == 'g' else rows
    targets_full = np.eye(T)[rng.integers(0, T, n_t)].astype(np.float32)
    weights_full = (rng.uniform(0.5, 1.5, n_t) / n_t * 4).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    g['set_mask'], g['output_mask'] = set_mask, np.ones(rows, bool)
    cls = {'n': GNNnodeBased, 'g': GNNgraphBased, 'a': GNNedgeBased}[kind]
    specs, gnns, s0, ms_dev, ms_ref = [], [], [], [], []
    for i in range(layers):
        nl_i = nl + (i > 0) * (get_state * ds + (get_output and kind != 'a') * T)
        al_i = al + (i > 0) * (get_output and kind == 'a') * T
        unrolled = mixed and i == 0
        if frozen: st = C.frozen_net(rng, al_i + 2 * (ds + nl_i), [9, ds], 'tanh', 0.3)
        else: st = make_mlp(rng, al_i + 2 * (ds + nl_i), [9, ds], 'tanh', gain=0.5, batch_normalization=unrolled, bn_random=unrolled)
        ou = make_mlp(rng, 2 * (ds + nl_i) + al_i if kind == 'a' else ds + nl_i, [T], 'softmax', batch_normalization=False)
        st['dropout'], ou['dropout'] = ({0: 0.2} if unrolled else {}), {}
        max_it, thr = (4, 0.0) if unrolled else (30, 1e-3)
        specs.append(dict(net_state=st, net_output=ou, state_vect_dim=ds, max_iteration=max_it, threshold=thr, fixed_point=not unrolled))
        gnn = cls(net_state=ga._sequential(st), net_output=ga._sequential(ou), optimizer=None, loss_function=losses.categorical_crossentropy,
                  loss_arguments=None, state_vect_dim=ds, max_iteration=max_it, threshold=thr, addressed_problem='c')
        gnn.impl = 1
        if not unrolled: gnn.set_gradient_mode('fixed_point', batch_normalization='frozen' if frozen else None, label_gradients=True)
        gnns.append(gnn)
        s0.append((0.1 * rng.standard_normal((n, ds))).astype(np.float32))
        masks = [{0: rng.random((n, al_i + 2 * (ds + nl_i))) > 0.2} for _ in range(max_it)] if unrolled else None
        ms_ref.append(masks if unrolled else [{}] * max_it)
        ms_dev.append(np.concatenate([mk[0].astype(np.uint8).ravel() for mk in masks]) if unrolled else None)
    lgnn = LGNN(gnns, get_state, get_output, optimizers.SGD(LR), losses.categorical_crossentropy, None, 'c')
    lgnn.training_mode = mode
    lgnn.device_optimizer = device_optimizer
    lgnn.device_chain = device_chain
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based=kind,
                     aggregation_mode='average', NodeGraph=ng)
    sel = np.ones(n_t, bool) if kind == 'g' else set_mask
    return dict(lgnn=lgnn, batch=GraphTensor.fromGraphObject(go), g=g, specs=specs, s0=s0, ms_dev=ms_dev if mixed else None, ms_ref=ms_ref,
                targets=targets_full[sel], weights=weights_full[sel], kind=kind)


def joint_step(s):
    return s['lgnn'].training_step(s['batch'], mean=True, state0=s['s0'], masks_state=s['ms_dev'])


def joint_mirror(s, res, get_state, get_output, mode, dtype):
    """The mirror of a joint step with the device's counts; mean=False: training_step returns the RAW gradients (an unrolled layer's are divided by k
    only where they are applied)."""
    its = [None if v is None else int(v) for v in res['adjoint_iterations']]
    return lm.lgnn_step(s['g'], s['specs'], get_state, get_output, mode, s['s0'], s['ms_ref'], [{}] * len(s['specs']), s['targets'], s['weights'], mean=False,
                        graph_based=s['kind'] == 'g', edge_based=s['kind'] == 'a', dtype=dtype, k_forced=[int(k) for k in res['k']], iterations_forced=its)


def joint_arrays(r):
    out = {}
    for li in range(len(r['grads_state'])):
        out[f'out{li}'] = r['outs'][li]
        for i, a in enumerate(r['grads_state'][li]): out[f'L{li} grads_state[{i}]'] = a
        for i, a in enumerate(r['grads_output'][li]): out[f'L{li} grads_output[{i}]'] = a
    return out


def all_weights(lgnn):
    return [np.array(w) for gnn in lgnn.gnns for w in gnn.net_state.get_weights() + gnn.net_output.get_weights()]


@pytest.mark.parametrize('kind', ['n', 'g', 'a'])
@pytest.mark.parametrize('get_state,get_output', [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_lgnn_joint_step(mode, get_state, get_output, kind):
    """A joint step of a stack of fixed-point layers (three under 'parallel', two under 'residual'): the host-optimizer path returns the raw gradients,
    held to the mirror; plain SGD lands on w - lr g UNDIVIDED although mean=True and every k >= 2; device_chain False gives the same bits; the armed
    device path lands on the same weights to 1e-6."""
    layers = 3 if mode == 'parallel' else 2
    args = (kind, get_state, get_output, layers, mode)
    s = stack(*args)
    before = [gnn.net_state.trainable_variables + gnn.net_output.trainable_variables for gnn in s['lgnn'].gnns]
    before = [[np.array(a) for a in layer] for layer in before]
    res = joint_step(s)
    assert min(res['k']) >= 2 and all(res['adjoint_converged']) and min(res['adjoint_iterations']) >= 2, (res['k'], res['adjoint_iterations'])
    want, noisy = (joint_mirror(s, res, get_state, get_output, mode, dt) for dt in (np.float64, np.float32))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    check_tight(f'lgnn {kind} {mode} s{int(get_state)} o{int(get_output)}', joint_arrays(res), joint_arrays(want), joint_arrays(noisy))
    # layer 0's net_state receives gradient through the hand-over: without it, its gradient would be that of its own loss term alone
    moved = 0.0
    for li, gnn in enumerate(s['lgnn'].gnns):
        after = gnn.net_state.trainable_variables + gnn.net_output.trainable_variables
        for a, b, g_ in zip(after, before[li], res['grads_state'][li] + res['grads_output'][li]):
            assert np.max(np.abs(np.asarray(a, np.float64) - (np.asarray(b, np.float64) - LR * np.asarray(g_, np.float64)))) <= 1e-6
        moved = max(moved, max(float(np.max(np.abs(LR * g_))) for g_ in res['grads_state'][li]))
    assert moved > 1e-3                                         # (a division by k >= 2 would show at 1e-6)
    host = stack(*args, device_chain=False)
    res_h = joint_step(host)
    same_bits(joint_arrays(res), joint_arrays(res_h))
    assert res_h['loss'] == res['loss'] and res_h['adjoint_iterations'] == res['adjoint_iterations']
    armed = stack(*args, device_optimizer=True)
    res_d = joint_step(armed)
    assert res_d['k'] == res['k'] and res_d['adjoint_iterations'] == res['adjoint_iterations']
    for a, b in zip(all_weights(armed['lgnn']), all_weights(s['lgnn'])): assert np.max(np.abs(a - b)) <= 1e-6


@pytest.mark.parametrize('mode', ['parallel', 'residual'])
def test_lgnn_mixed_stack(mode):
    """Layer 0 unrolled with Dropout and BatchNormalization in net_state (four bodies, gradients divided by k under mean), layer 1 fixed-point: the host
    chain carries layer 1's fixed-point label gradient into layer 0's unrolled backward pass.  The tight criterion on every array of both layers."""
    s = stack('n', True, True, 2, mode, mixed=True)
    before = [[np.array(a) for a in gnn.net_state.trainable_variables] for gnn in s['lgnn'].gnns]
    res = joint_step(s)
    assert res['k'][0] == 4.0 and res['k'][1] >= 2 and res['adjoint_iterations'][0] is None and res['adjoint_converged'][1]
    want, noisy = (joint_mirror(s, res, True, True, mode, dt) for dt in (np.float64, np.float32))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    check_tight(f'lgnn mixed {mode}', joint_arrays(res), joint_arrays(want), joint_arrays(noisy))
    # under mean the unrolled layer's net_state gradients are applied divided by its k = 4, the fixed-point layer's undivided
    for li, scale in ((0, 0.25), (1, 1.0)):
        for a, b, g_ in zip(s['lgnn'].gnns[li].net_state.trainable_variables, before[li], res['grads_state'][li]):
            assert np.max(np.abs(np.asarray(a, np.float64) - (np.asarray(b, np.float64) - LR * scale * np.asarray(g_, np.float64)))) <= 1e-6
        assert max(float(np.max(np.abs(LR * g_))) for g_ in res['grads_state'][li]) > 1e-3


@pytest.mark.parametrize('device_chain', [True, False], ids=['device_chain', 'host_chain'])
def test_lgnn_stack_of_frozen_batch_normalization_layers(device_chain):
    """Every net_state ends in BatchNormalization on its moving statistics: the joint step under the tight criterion (gamma and beta gradients
    included), and the moving statistics of net_state stay bit for bit what they were - on the host-optimizer path and on the armed device path,
    which land on the same weights to 1e-6."""
    args = ('n', True, True, 2, 'parallel')
    s = stack(*args, frozen=True, device_chain=device_chain)
    moving = [[np.array(a) for a in gnn.net_state.get_weights()[-2:]] for gnn in s['lgnn'].gnns]
    res = joint_step(s)
    assert min(res['k']) >= 2 and all(res['adjoint_converged']) and min(res['adjoint_iterations']) >= 2, (res['k'], res['adjoint_iterations'])
    want, noisy = (joint_mirror(s, res, True, True, 'parallel', dt) for dt in (np.float64, np.float32))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    assert all(len(gs) == 6 and np.abs(gs[4]).max() > 1e-3 and np.abs(gs[5]).max() > 1e-3 for gs in res['grads_state'])       # gamma, beta train
    check_tight(f'lgnn frozen {"device" if device_chain else "host"} chain', joint_arrays(res), joint_arrays(want), joint_arrays(noisy))
    armed = stack(*args, frozen=True, device_chain=device_chain, device_optimizer=True)
    joint_step(armed)
    for a, b in zip(all_weights(armed['lgnn']), all_weights(s['lgnn'])): assert np.max(np.abs(a - b)) <= 1e-6
    for t in (s, armed):
        for gnn, was in zip(t['lgnn'].gnns, moving):
            for a, b in zip(gnn.net_state.get_weights()[-2:], was): assert np.array_equal(np.asarray(a), b)


def test_lgnn_joint_training_reduces_the_loss():
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.MLP import MLP, set_seed
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(3)
    graphs = []
    for _ in range(3):
        nodes = (2 * rng.random((60, 3)) - 1).astype(np.float32)
        graphs.append(GraphObject(arcs=random_arcs(rng, 60, 150, 1), nodes=nodes, targets=np.eye(2)[(nodes[:, 0] - 0.5 * nodes[:, 2] > 0).astype(int)]))

    def model(layer):
        extra = 2 * (layer > 0)
        st = MLP(1 + 2 * (4 + 3 + extra), [10, 4], 'tanh', 'glorot_normal', 'zeros', batch_normalization=False)
        ou = MLP(4 + 3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
        return GNNnodeBased(net_state=st, net_output=ou, optimizer=None, loss_function=losses.categorical_crossentropy, loss_arguments=None,
                            state_vect_dim=4, max_iteration=15, threshold=0.01, addressed_problem='c')

    for mode in ('parallel', 'residual'):
        set_seed(7)
        lgnn = LGNN([model(0), model(1), model(1)], False, True, optimizers.Adam(0.02), losses.categorical_crossentropy, None, 'c')
        lgnn.set_gradient_mode('fixed_point', label_gradients=True)
        before = lgnn.test(graphs)['Loss']
        lgnn.train(graphs, 8, update_freq=4, training_mode=mode, verbose=0)
        after = lgnn.test(graphs)['Loss']
        assert after < 0.9 * before, (mode, before, after)
