"""The graph side of the training step on directed, unsorted arc lists (tests/train_graph_cases.py), against the float64 oracle: the concat
gathers (k_mlp_fwd building its own input, k_train_input in its three gather paths, k_train_input_rows), the transposed gathers of the backward
pass (k_state_grad_sum, k_state_grad_rows, k_state_grad_rows_al), the label and arc-label gradients (k_nodes_grad, k_arc_grad_readout,
k_arc_grad_agg), the edge-based backward (k_gather_edge_grad over the incidence lists of gnn_loop_set_edge_readout) and the graph readout inside
the step (k_graph_out, k_graph_out_bwd).

Why directed lists: on a symmetric, sorted list the CSR by source and the CSR by destination have identical index arrays, so a kernel that reads one
for the other, or walks the arcs the wrong way, moves no index (tests/test_train_graph_side_host.py shows it).  Every graph here has a hub in both
directions, a node without in-arcs, one without out-arcs, an isolated one, nodes of in-degree and others of out-degree exactly 0, 1, 3, 4, 5, 8, 9,
17 (the edges of the four-arcs-per-step loops), and arcs in random order, so that ArcNode's arc ids are an irregular permutation.

Per case (the table of train_graph_cases.CASES; threshold 0, so all max_iteration bodies run; tanh nets, gain 0.5, no BatchNormalization):
 0. the form: loop.train_forms(0) gives the expected letters and build_input, from which the rule restated in expected_kernels() names the concat
    and the state-gradient kernel (the two are chosen by the same predicates as the forms: rows, state width, Dropout in front of layer 0);
 1. zero pattern, exact (sentinel runs: d_out_nodes = 0, d_state_extra non-zero on the hub, on the node without in-arcs, on the node without
    out-arcs, on rows 31 | 32 and on the last 17 rows): the non-zero rows of d_nodes are the oracle's, which are the k-hop PREDECESSORS of the
    sentinels and not their successors - a kernel that walks the arcs the wrong way fails here whatever the tolerance; d_arcs likewise by arcs;
 2. every array per element: |device - oracle_f64| <= 8 x max |oracle_f32 - oracle_f64| + 2^-22 x max |oracle_f64| over the array (the criterion
    of tests/test_gpu_adjoint.py, set before any measurement here) - state, outputs, d_nodes, d_arcs, every gradient array;
 3. identical bits on a second run of the same loop.

Measured on an MI355X (profiles/train_graph_side.txt; GNN_TRAIN_GRAPH_RATIOS=<file> appends every (case, run, array) error, noise, their ratio and
the share of the bound used): see RESULTS below.

Edge-based cases: the arc mask (about 60 % in) leaves one node without a masked arc, gives the hub >= 30 masked arcs each way (37 nodes: >= 16 of
its 18), and leaves the node without in-arcs / without out-arcs one masked arc each.  d_arcs is compared in ORIGINAL arc order.  A run with
max_iteration 0 and d_out_nodes non-zero on ONE readout row isolates the readout term: exactly that row's arc position receives gradient.

Graph readout: 7 graphs of 1, 63, 64, 65, 130 nodes, an empty one and the rest (37 nodes: 1, 5, 7, 9, 4, empty, rest), non-uniform NodeGraph
weights; T = 1 (sigmoid, mean_squared_error), T = 2, 3 (softmax, categorical_crossentropy).  The engine accepts the empty graph.  Its output row
is 0: mean_squared_error is defined there and the empty graph carries weight like the others; categorical_crossentropy of a zero row is 0 / 0 in
the reference, so in those cases the empty graph has sample weight 0 and the oracle is evaluated on the six others - loss and gradients must not
notice the empty graph.

RESULTS (884 arrays).  No zero pattern differs; every array of every sentinel, edge and graph-readout run and all but one array of the dense runs lie
under the criterion.  The largest share of the bound used is 0.56 (graphs_n4113_T1 one_graph grads_output[1]: error 1.6e-8, 18.5 x a noise of
8.5e-10, under the 2^-22 floor), then 0.54 (input_scalar no_out grads_state[1], ratio 12.2) and 0.53 (rows16/sum hub grads_state[0], ratio 4.6: the
70-term chains of the hub).  d_nodes stays below 0.39 of its bound, d_arcs below 0.36.
Fallen back to 1e-3 of the largest entry (LOOSE_DENSE), dense run only:
  built_rows / normalized, grads_output[1] (net_output's bias gradient, the row of ones in k_layer_bwd's [H | 1]^T dZ): error 3.56e-7 on 0.525,
  228.9 x a noise of 1.6e-9, 2.59 x the bound.  Cause: summation order alone - the entry is a float32 sum over the 29 masked rows of terms up to
  0.82 that cancel (sum of magnitudes 9.87); float32 sums of the same 29 float64 terms in 200 random row orders err by up to 4.8e-7 (median
  6e-8), and the oracle's float32 run happens to land within 1.6e-9.  No index is involved: the same array of the same case passes in the other two
  aggregation modes and in every sentinel run, and the kernel reads no graph array."""
import os

import numpy as np
import pytest

import train_graph_cases as G
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -22
LOOSE = 1e-3                # the bound of tests/test_gpu_train.py, of the array's largest entry
# (case, mode, array) of the DENSE runs whose error is summation order alone and which fall back to LOOSE (module docstring, RESULTS)
LOOSE_DENSE = {('built_rows', 'normalized', 'grads_output[1]'): 'float32 column sum of 29 cancelling terms'}
LETTER = {'per_op': 'P', 'mlp_fwd': 'M', 'wide': 'W', 'chain3': 'C'}

_BUILT = {}


def _engine():
    from GNN import _engine
    return _engine


def built(c, mode='average', edge=False, k=None):
    """Graph, nets, initial state, Dropout masks and the oracle's training-mode forward in float64 and float32: once per (case, mode), shared by
    its runs, never modified."""
    k = c.k if k is None else k
    key = (c.name, mode, edge, k)
    if key not in _BUILT:
        arcs = G.case_graph(c)
        rng = np.random.default_rng(c.seed)
        n, ds, nlc, in_s = c.n, G.ds_of(c), G.nlc_of(c), G.in_s_of(c)
        nodes = (2 * rng.random((n, c.nl)) - 1).astype(np.float32)
        g = orc.make_graph_dict(arcs, nodes, mode)
        if edge:
            g['set_mask'], g['output_mask'] = G.edge_mask(arcs, n, c.seed)[0], np.ones(len(arcs), bool)
        else:
            g['set_mask'] = rng.random(n) < 0.8
        st = make_mlp(rng, in_s, list(c.layers), 'tanh', gain=0.5, batch_normalization=False)
        ou = make_mlp(rng, 2 * (ds + nlc) + c.al if edge else ds + nlc, [2], 'softmax', batch_normalization=False)
        st['dropout'], ou['dropout'] = ({0: c.drop0} if c.drop0 else {}), {}
        masks = [({0: rng.random((n, in_s)) > c.drop0} if c.drop0 else {}) for _ in range(max(k, 1))]
        s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if c.d else None
        ctx = {dt: tro.train_forward(g, st, ou, c.d, k, 0.0, s0, masks, {}, dtype=dt, edge_based=edge) for dt in (np.float64, np.float32)}
        assert ctx[np.float64]['k'] == ctx[np.float32]['k'] == k
        _BUILT[key] = dict(case=c, arcs=arcs, g=g, st=st, ou=ou, masks=masks, s0=s0, ctx=ctx, edge=edge, k=k, m=int(ctx[np.float64]['mask'].sum()))
    return _BUILT[key]


def incoming(b, sset):
    """(d_out_nodes, d_state_extra, sentinel rows or None) of a run"""
    c = b['case']
    n, ds = c.n, G.ds_of(c)
    rng = np.random.default_rng(sum(map(ord, sset)))
    if sset == 'dense':
        return rng.standard_normal((b['m'], 2)).astype(np.float32), rng.standard_normal((n, ds)).astype(np.float32), None
    rows = G.sentinel_rows(c, sset)
    dse = np.zeros((n, ds), np.float32)
    dse[rows] = rng.standard_normal((rows.size, ds)).astype(np.float32)
    return np.zeros((b['m'], 2), np.float32), dse, rows


def src_csr_of(b):
    from test_gpu_train import _by_source_csr
    return _by_source_csr(b['g'], b['case'].n)


def run_device(b, d_out, dse, src_csr=None):
    """train_forward + train_backward on the device, twice on one loop: (forms of net_state, [results of run 1, of run 2])."""
    e = _engine()
    c, g, st, ou, edge = b['case'], b['g'], b['st'], b['ou'], b['edge']
    n, L = c.n, len(c.layers)
    labels = np.asarray(g['arcs'])[:, 2:]
    node_mask = np.ones(n, bool) if edge else g['set_mask']
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], labels[g['arcT'][1]], g['nodes'], node_mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], False), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, c.d, b['k'], 0.0)
    if c.d: loop.set_state0(b['s0'])
    if edge:
        graph.set_arc_order(g['arcT'][1], labels)
        entry_dst = np.repeat(np.arange(n, dtype=np.int32), np.diff(g['adjT'][0]))
        loop.set_edge_readout(entry_dst, labels, g['set_mask'])
    ms = np.concatenate([mk[0].astype(np.uint8).ravel() for mk in b['masks']]) if c.drop0 else None
    src_csr = src_csr_of(b) if src_csr is None else src_csr
    runs = []
    for _ in range(2):
        k, out = loop.train_forward(mst, mou, src_csr, dropout_state=[c.drop0] + [0.0] * L, dropout_output=[0, 0], masks_state=ms)
        forms = loop.train_forms(0)
        state = loop.state()
        res = loop.train_backward(d_out, dse, want_d_nodes=True, want_d_arcs=edge)
        runs.append(dict(k=k, out=out, state=state, d_nodes=res['d_nodes'], d_arcs=res['d_arcs'], grads_state=res['grads_state'],
                         grads_output=res['grads_output']))
    loop.close(); graph.close()
    return forms, runs


def arrays(r):
    """name -> array of one result (device run or oracle), in a fixed order"""
    out = {'state': r['state'], 'out_nodes': r['out'], 'd_nodes': r['d_nodes']}
    if r.get('d_arcs') is not None: out['d_arcs'] = r['d_arcs']
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def oracle(b, d_out, dse, dt):
    ctx = b['ctx'][dt]
    res = tro.train_backward(ctx, d_out.astype(dt), None if dse is None else dse.astype(dt), want_d_arcs=b['edge'])
    return dict(state=ctx['state'], out=ctx['out_nodes'], d_nodes=res[2], d_arcs=res[3] if b['edge'] else None, grads_state=res[0], grads_output=res[1])


def record(lines):
    path = os.environ.get('GNN_TRAIN_GRAPH_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))


def compare(tag, run, got, want, noisy, loose=()):
    """Every array per element under the criterion of the module docstring (the arrays named in `loose`: LOOSE of the largest entry); every
    error, noise and ratio is printed and recorded first."""
    assert list(got) == list(want) == list(noisy)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(want[key], np.float64)
        assert a.shape == w.shape, (key, a.shape, w.shape)
        top = float(np.max(np.abs(w))) if w.size else 0.0
        noise = float(np.max(np.abs(np.asarray(noisy[key], np.float64) - w))) if w.size else 0.0
        diff = np.abs(a.astype(np.float64) - w)
        err = float(np.max(diff)) if w.size else 0.0
        bound = MARGIN * noise + FLOOR * top
        ratio = err / noise if noise > 0 else (0.0 if err == 0 else float('inf'))
        used = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
        lines.append(f'{tag:28s} {run:10s} {key:16s} err {err:9.3e}  noise {noise:9.3e}  ratio {ratio:6.2f}  of bound {used:5.3f}  max|ref| {top:9.3e}')
        if key in loose: bound = LOOSE * top
        if w.size and not np.all(diff <= bound): bad.append(lines[-1])
    record(lines)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)


def same_bits(first, second):
    for key, a in first.items():
        assert np.array_equal(a.view(np.uint32), second[key].view(np.uint32)), key


def check_forms(c, forms):
    got = tuple(''.join(LETTER[x] for x in forms[key]) for key in ('forward', 'backward'))
    assert got == (c.fwd, c.bwd) and forms['build_input'] == c.build, (c.name, forms)
    if c.name in G.EXPECTED_KERNELS: assert G.expected_kernels(c) == G.EXPECTED_KERNELS[c.name]
    # the predicates behind the two graph-side kernels, asked of the engine itself: many rows <=> no k_mlp_fwd for a two-layer net
    e = _engine()
    probe = e.train_forms((G.in_s_of(c), 7, G.ds_of(c)), ['tanh', 'tanh'], None, c.n)
    assert (probe['forward'][0] != 'mlp_fwd') == (c.n >= G.MIN_ROWS)


def nonzero_rows(a):
    return (np.asarray(a) != 0).any(axis=1)


def check_patterns(b, rows, got, want):
    """The exact zero patterns of a sentinel run"""
    c, arcs, k = b['case'], b['arcs'], b['k']
    pred, succ = G.predecessors(arcs, rows, k, c.n), G.successors(arcs, rows, k, c.n)
    dev, ref = nonzero_rows(got['d_nodes']), nonzero_rows(want['d_nodes'])
    assert np.array_equal(dev, ref), (np.nonzero(dev != ref)[0][:20], 'device rows differ from the oracle rows')
    if c.drop0: assert not (ref & ~pred).any() and ref[rows].all()          # (a dropped input column can silence a row: never more than the predecessors)
    else: assert np.array_equal(ref, pred)
    assert not np.array_equal(dev, succ)
    assert not got['d_nodes'][~pred].any()
    if rows.size == 1 and rows[0] == G.NO_IN: assert dev.sum() == 1 and dev[G.NO_IN]
    if rows.size == 1 and rows[0] == G.NO_OUT: assert dev.sum() > 1 and dev[arcs[arcs[:, 1] == G.NO_OUT, 0].astype(int)].all()
    if b['edge']:
        # the aggregate term alone (d_out_nodes = 0): arc a receives gradient iff its destination is within k - 1 arcs in front of a sentinel
        dst = arcs[:, 1].astype(int)
        dev_a, ref_a = nonzero_rows(got['d_arcs']), nonzero_rows(want['d_arcs'])
        assert np.array_equal(dev_a, ref_a), np.nonzero(dev_a != ref_a)[0][:20]
        assert np.array_equal(ref_a, G.predecessors(arcs, rows, k - 1, c.n)[dst])
        assert not np.array_equal(dev_a, G.successors(arcs, rows, k - 1, c.n)[dst])


def one_case(c, mode, sset, edge=False):
    b = built(c, mode, edge)
    d_out, dse, rows = incoming(b, sset)
    forms, runs = run_device(b, d_out, dse)
    check_forms(c, forms)
    got, want, noisy = arrays(runs[0]), arrays(oracle(b, d_out, dse, np.float64)), arrays(oracle(b, d_out, dse, np.float32))
    assert runs[0]['k'] == runs[1]['k'] == b['k']
    if rows is not None:
        check_patterns(b, rows, got, want)
        assert np.abs(want['grads_state[0]']).max() > 0
    compare(f'{c.name}/{mode}', sset, got, want, noisy, loose=[key for (name, md, key) in LOOSE_DENSE if (name, md) == (c.name, mode) and not edge] if sset == 'dense' else ())
    same_bits(got, arrays(runs[1]))


RUNS = [(c, mode, sset) for c in G.CASES for mode in c.modes for sset in ('dense',) + G.sentinel_sets(c)]
EDGE_RUNS = [(c, sset) for c in G.EDGE_CASES for sset in ('dense',) + G.sentinel_sets(c)]


@pytest.mark.parametrize('c,mode,sset', RUNS, ids=[f'{c.name}-{mode}-{sset}' for c, mode, sset in RUNS])
def test_graph_side_against_oracle(c, mode, sset):
    one_case(c, mode, sset)


@pytest.mark.parametrize('c,sset', EDGE_RUNS, ids=[f'{c.name}-{sset}' for c, sset in EDGE_RUNS])
def test_edge_based_graph_side_against_oracle(c, sset):
    one_case(c, 'average', sset, edge=True)


@pytest.mark.parametrize('c', G.EDGE_CASES, ids=[c.name for c in G.EDGE_CASES])
def test_readout_term_reaches_one_arc_position(c):
    """max_iteration 0 (no body, so no aggregate term) and d_out_nodes non-zero on ONE readout row: d_arcs is non-zero at exactly the arc position
    the oracle names - the position of that row's mask entry, in original arc order."""
    b = built(c, 'average', True, k=0)
    m = b['m']
    row = m // 2
    d_out = np.zeros((m, 2), np.float32)
    d_out[row] = [0.75, -1.25]
    _, runs = run_device(b, d_out, None)
    got, want, noisy = arrays(runs[0]), arrays(oracle(b, d_out, None, np.float64)), arrays(oracle(b, d_out, None, np.float32))
    position = int(np.nonzero(b['g']['set_mask'])[0][row])
    assert list(np.nonzero(nonzero_rows(want['d_arcs']))[0]) == [position]
    assert list(np.nonzero(nonzero_rows(got['d_arcs']))[0]) == [position]
    # both endpoints of that entry, and nobody else, receive state gradient (D > 0: label gradient through net_output's input)
    (ip_d, src_c, _), _ = G.csr_pair(b['arcs'], c.n)
    ends = {int(np.repeat(np.arange(c.n), np.diff(ip_d))[position]), int(src_c[position])}
    assert set(np.nonzero(nonzero_rows(got['d_nodes']))[0]) == set(np.nonzero(nonzero_rows(want['d_nodes']))[0]) == ends
    compare(f'{c.name}/k0', 'one_row', got, want, noisy)
    same_bits(got, arrays(runs[1]))


# --- the graph readout inside the step ------------------------------------------------------------------------------------------------------------------
_GRAPH = {}


def graph_setup(n, t):
    if (n, t) not in _GRAPH:
        c = [x for x in G.CASES if x.name == ('built_rows' if n == G.N_SMALL else 'rows16')][0]
        rng = np.random.default_rng(100 * t + c.seed)
        arcs = G.case_graph(c)
        nodes = (2 * rng.random((n, c.nl)) - 1).astype(np.float32)
        ng = G.node_graph(rng, n)
        g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
        st = make_mlp(rng, G.in_s_of(c), list(c.layers), 'tanh', gain=0.5, batch_normalization=False)
        ou = make_mlp(rng, c.d + c.nl, [t], 'sigmoid' if t == 1 else 'softmax', batch_normalization=False)
        st['dropout'], ou['dropout'] = {}, {}
        s0 = (0.1 * rng.standard_normal((n, c.d))).astype(np.float32)
        ngr = ng.shape[1]
        targets = (rng.random((ngr, 1)) if t == 1 else np.eye(t)[rng.integers(0, t, ngr)]).astype(np.float32)
        weights = rng.uniform(0.5, 1.5, ngr).astype(np.float32)
        _GRAPH[(n, t)] = dict(case=c, g=g, ng=ng, st=st, ou=ou, s0=s0, targets=targets, weights=weights)
    return _GRAPH[(n, t)]


def graph_step(s, weights):
    """gnn_loop_train_step with the NodeGraph^T CSR, twice on one loop"""
    e = _engine()
    c, g = s['case'], s['g']
    n = c.n
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], g['nodes'], np.ones(n, bool))
    mst, mou = e.Mlp(s['st']['weights'], s['st']['activations'], False), e.Mlp(s['ou']['weights'], s['ou']['activations'], False)
    loop = e.Loop(graph, mst, mou, c.d, c.k, 0.0)
    loop.set_state0(s['s0'])
    from test_gpu_train import _by_source_csr
    kind = 1 if s['targets'].shape[1] == 1 else 0
    runs = [loop.train_step(mst, mou, _by_source_csr(g, n), s['targets'], weights, kind, G.nodegraph_csr(s['ng'])) for _ in range(2)]
    loop.close(); graph.close()
    return runs


def graph_oracle(s, weights, keep, dt):
    """The oracle's step on the graphs `keep` (columns of NodeGraph, rows of the targets)"""
    c, t = s['case'], s['targets'].shape[1]
    g = dict(s['g'], NodeGraph=s['ng'][:, keep])
    return tro.train_step(g, s['st'], s['ou'], c.d, c.k, 0.0, s['s0'], [{}] * c.k, {}, s['targets'][keep], weights[keep],
                          loss='mean_squared_error' if t == 1 else 'categorical_crossentropy', mean=False, graph_based=True, dtype=dt)


def grad_arrays(r):
    out = {}
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


@pytest.mark.parametrize('n,t', G.GRAPH_CASES)
def test_graph_readout_inside_the_step(n, t):
    s = graph_setup(n, t)
    sizes = G.graph_sizes(n)
    empty = sizes.index(0)
    weights = s['weights'].copy()
    keep = np.arange(len(sizes))
    if t > 1:                                           # categorical_crossentropy of the empty graph's zero row is 0 / 0 in the reference (module docstring)
        weights[empty] = 0.0
        keep = keep[keep != empty]
    runs = graph_step(s, weights)
    ref, ref32 = graph_oracle(s, weights, keep, np.float64), graph_oracle(s, weights, keep, np.float32)
    res = runs[0]
    assert res['k'] == ref['k'] == s['case'].k
    print(f'graphs n={n} T={t} loss {res["loss"]:.7f} oracle {ref["loss"]:.7f}')
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    compare(f'graphs_n{n}_T{t}', 'all', grad_arrays(res), grad_arrays(ref), grad_arrays(ref32))
    assert runs[1]['loss'] == res['loss']
    same_bits(grad_arrays(res), grad_arrays(runs[1]))


@pytest.mark.parametrize('n,t', G.GRAPH_CASES)
def test_one_graph_carries_the_loss(n, t):
    """Sample weight 0 on every graph but one (the 130-node graph - 37 nodes: the 4-node one - first wave of the kernel's second block, in front of the
    empty graph): loss and gradients are the oracle's for that graph ALONE (its NodeGraph column, its target row)."""
    s = graph_setup(n, t)
    only = 4
    assert G.graph_sizes(n)[only] > 0 and G.graph_sizes(n)[only + 1] == 0
    weights = np.zeros_like(s['weights'])
    weights[only] = s['weights'][only]
    runs = graph_step(s, weights)
    keep = np.array([only])
    ref, ref32 = graph_oracle(s, weights, keep, np.float64), graph_oracle(s, weights, keep, np.float32)
    res = runs[0]
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    assert np.abs(ref['grads_output'][0]).max() > 0
    compare(f'graphs_n{n}_T{t}', 'one_graph', grad_arrays(res), grad_arrays(ref), grad_arrays(ref32))
    same_bits(grad_arrays(res), grad_arrays(runs[1]))


# --- the model surface: GraphObject / GraphTensor in front of the same kernels -----------------------------------------------------------------------------
def _sequential(net):
    from GNN.MLP import Sequential, Dense, Dropout, BatchNormalization
    layers = []
    for l in range(len(net['activations'])):
        if net['dropout'].get(l): layers.append(Dropout(net['dropout'][l]))
        layers.append(Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)))
    if net['batch_normalization']: layers.append(BatchNormalization())
    seq = Sequential(layers)
    seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
    return seq


def _sorted_directed(n, al, seed):
    arcs = G.directed_graph(seed, n, degrees=True, al=al)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]                    # (source, destination)-sorted and unique, as GraphObject lists are
    (ip_d, _, arc_id), (ip_s, _) = G.csr_pair(arcs, n)
    assert not np.array_equal(ip_d, ip_s) and not np.array_equal(arc_id, np.arange(len(arcs)))
    return arcs


def _loose(pairs, tag):
    for got, want in pairs:
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= LOOSE * max(1e-3, np.max(np.abs(want))), (tag, got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize('edge', [False, True], ids=['GNNnodeBased', 'GNNedgeBased'])
def test_model_training_step_on_a_directed_graph(edge):
    """GNNnodeBased / GNNedgeBased.training_step on a GraphObject built from a directed list against the oracle's step, at the bound of
    tests/test_gpu_train.py (the Python path adds nothing numerical): adjacency_by_source() and edge_readout_arrays() in front of the kernels."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNedgeBased
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(70 + edge)
    n, nl, al, d, max_it = G.N_SMALL, 3, 2, 4, 3
    arcs = _sorted_directed(n, al, 1012)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    items = len(arcs) if edge else n
    set_mask = G.edge_mask(arcs, n, 5)[0] if edge else rng.random(n) < 0.8
    targets_full = np.eye(2)[rng.integers(0, 2, items)].astype(np.float32)
    weights_full = rng.uniform(0.5, 1.5, items).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'], g['output_mask'] = set_mask, np.ones(items, bool)
    st = make_mlp(rng, al + 2 * (d + nl), [7, d], 'tanh', gain=0.5, batch_normalization=False)
    ou = make_mlp(rng, 2 * (d + nl) + al if edge else d + nl, [2], 'softmax', batch_normalization=False)
    st['dropout'], ou['dropout'] = {}, {}
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    ref = tro.train_step(g, st, ou, d, max_it, 0.0, s0, [{}] * max_it, {}, targets_full[set_mask], weights_full[set_mask], mean=False, edge_based=edge)
    gnn = (GNNedgeBased if edge else GNNnodeBased)(net_state=_sequential(st), net_output=_sequential(ou), optimizer=optimizers.SGD(0.0),
                                                   loss_function=losses.categorical_crossentropy, loss_arguments=None, state_vect_dim=d,
                                                   max_iteration=max_it, threshold=0.0, addressed_problem='c')
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based='a' if edge else 'n',
                     aggregation_mode='average')
    assert np.array_equal(go.arcs, arcs)
    res = gnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=s0)
    assert res['k'] == ref['k'] == max_it
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    _loose(list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])), edge)


def test_edge_lgnn_joint_step_on_a_directed_graph():
    """Edge-based LGNN, 'parallel', two layers: d_arcs of layer 1 carries its loss to layer 0's outputs, through adjacency_by_source(),
    edge_readout_arrays() and the arc order of the device graph - on a directed list, where arc ids, entries and sources all differ."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNedgeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(91)
    n, nl, al, t, d, max_it, L = G.N_SMALL, 3, 2, 2, 4, 3, 2
    arcs = _sorted_directed(n, al, 1012)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    e = len(arcs)
    set_mask = G.edge_mask(arcs, n, 5)[0]
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'], g['output_mask'] = set_mask, np.ones(e, bool)
    targets_full = rng.random((e, t)).astype(np.float32)
    weights_full = rng.uniform(0.5, 1.5, e).astype(np.float32)
    layers, s0, gnns = [], [], []
    for i in range(L):
        ins, ls = orc.get_inout_dims('state', nl, al, t, 'a', d, [7], layer=i, get_state=True, get_output=True)
        ino, lo = orc.get_inout_dims('output', nl, al, t, 'a', d, None, layer=i, get_state=True, get_output=True)
        st = make_mlp(rng, ins, ls, 'tanh', gain=0.5, batch_normalization=False)
        ou = make_mlp(rng, ino, lo, 'tanh', out_activation='softmax', batch_normalization=False)
        st['dropout'], ou['dropout'] = {}, {}
        layers.append(dict(net_state=st, net_output=ou, state_vect_dim=d, max_iteration=max_it, threshold=0.0))
        s0.append((0.1 * rng.standard_normal((n, d))).astype(np.float32))
        gnns.append(GNNedgeBased(net_state=_sequential(st), net_output=_sequential(ou), optimizer=None, loss_function=None, loss_arguments=None,
                                 state_vect_dim=d, max_iteration=max_it, threshold=0.0, addressed_problem='r'))
    ref = tro.lgnn_train_step(g, layers, True, True, 'parallel', s0, [[{}] * max_it] * L, [{}] * L, targets_full[set_mask], weights_full[set_mask],
                              loss='mean_squared_error', mean=False, edge_based=True)
    lgnn = LGNN(gnns, True, True, optimizers.SGD(0.0), losses.mean_squared_error, None, 'r')
    lgnn.training_mode = 'parallel'
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based='a',
                     aggregation_mode='average')
    res = lgnn.training_step(GraphTensor.fromGraphObject(go), mean=False, state0=s0)
    assert res['k'] == ref['k']
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for li in range(L):
        np.testing.assert_allclose(res['outs'][li], ref['outs'][li], atol=2e-5)
        _loose(list(zip(res['grads_state'][li], ref['grads_state'][li])) + list(zip(res['grads_output'][li], ref['grads_output'][li])), li)
    assert np.abs(ref['grads_output'][0][0]).max() > 0
