"""CPU side of tests/test_gpu_train_graph_side.py: what the builders of tests/train_graph_cases.py promise, for every case of the GPU file; the
project's host chain (GraphObject / GraphTensor, adjacency_by_source, edge_readout_arrays) against the oracle's restatement and against a plain
dense transpose on a directed, unsorted arc list; and the oracle's arc-label gradient on such a list, which the GPU file compares against."""
import numpy as np
import pytest

import train_graph_cases as G
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs

ALL = G.CASES + G.EDGE_CASES


def test_symmetric_lists_hide_the_distinction():
    """Why the directed lists exist: on the suite's default arc list both CSRs have the same index arrays."""
    arcs = random_arcs(np.random.default_rng(0), 37, 90, 2)
    (ip_d, src_d, _), (ip_s, dst_s) = G.csr_pair(arcs, 37)
    assert np.array_equal(ip_d, ip_s) and np.array_equal(src_d, dst_s)


@pytest.mark.parametrize('c', ALL, ids=[c.name for c in ALL])
def test_builder_keeps_its_promises(c):
    arcs = G.case_graph(c)
    G.check_directed(arcs, c.n, True)
    assert arcs.shape[1] == 2 + c.al and arcs.dtype == np.float32
    assert 1.5 * c.n <= len(arcs) <= 4.2 * c.n                      # about two arcs per node (more on 37 nodes: the pinned degrees)
    assert np.array_equal(arcs, G.case_graph(c))                    # seeded: the host and the GPU file see the same list
    for sset in G.sentinel_sets(c):
        rows = G.sentinel_rows(c, sset)
        pred, succ = G.predecessors(arcs, rows, c.k, c.n), G.successors(arcs, rows, c.k, c.n)
        assert pred[rows].all() and succ[rows].all()
        assert not np.array_equal(pred, succ) and not pred.all() and not succ.all(), (c.name, sset)
    assert G.predecessors(arcs, [G.NO_IN], c.k, c.n).sum() == 1 and G.successors(arcs, [G.NO_OUT], c.k, c.n).sum() == 1
    assert G.predecessors(arcs, [G.NO_OUT], c.k, c.n).sum() > 1


def test_closures_on_a_chain():
    arcs = np.array([[0, 1], [1, 2], [2, 3], [3, 4]], np.float32)
    assert list(np.nonzero(G.predecessors(arcs, [3], 2, 5))[0]) == [1, 2, 3]
    assert list(np.nonzero(G.successors(arcs, [1], 2, 5))[0]) == [1, 2, 3]
    assert list(np.nonzero(G.predecessors(arcs, [3], 0, 5))[0]) == [3]


def test_case_table_and_kernel_rule_agree():
    """The kernels each case is meant to reach, stated twice: by name in EXPECTED_KERNELS and derived from the engine's rule."""
    for c in G.CASES:
        assert G.expected_kernels(c) == G.EXPECTED_KERNELS[c.name], c.name
        assert G.in_s_of(c) == c.al + 2 * (G.ds_of(c) + G.nlc_of(c))
    assert {k for v in G.EXPECTED_KERNELS.values() for k in v} == {
        'k_mlp_fwd', 'k_train_input float4', 'k_train_input scalar', 'k_train_input scalar+dropout', 'k_train_input_rows',
        'k_state_grad_sum', 'k_state_grad_rows', 'k_state_grad_rows_al'}
    assert G.dims_of([c for c in G.CASES if c.name == 'chain_aligned'][0]) == (135, 128, 128, 64)
    assert G.N_MANY == 128 * 32 + 17 and G.MIN_ROWS - 1 < G.MIN_ROWS <= G.N_MANY


@pytest.mark.parametrize('c', G.EDGE_CASES, ids=[c.name for c in G.EDGE_CASES])
def test_edge_mask_conditions(c):
    arcs = G.case_graph(c)
    mask, lonely = G.edge_mask(arcs, c.n, c.seed)
    G.check_edge_mask(arcs, c.n, mask, lonely)
    assert mask.dtype == bool and len(mask) == len(arcs) and lonely >= 20
    # the arcs that receive gradient through the aggregated arc labels (destination within k - 1 arcs in front of a sentinel) tell the directions apart
    dst = arcs[:, 1].astype(int)
    for sset in G.sentinel_sets(c):
        rows = G.sentinel_rows(c, sset)
        assert not np.array_equal(G.predecessors(arcs, rows, c.k - 1, c.n)[dst], G.successors(arcs, rows, c.k - 1, c.n)[dst]), sset


@pytest.mark.parametrize('n', [G.N_SMALL, G.N_MANY])
def test_graph_sizes(n):
    sizes = G.graph_sizes(n)
    assert len(sizes) == 7 and sum(sizes) == n and sizes.count(0) == 1 and sizes[0] == 1
    z = sizes.index(0)
    assert 0 < z < 6 and sizes[z - 1] > 0 and sizes[z + 1] > 0
    if n == G.N_MANY: assert sizes[:5] == [1, 63, 64, 65, 130]
    ng = G.node_graph(np.random.default_rng(1), n)
    ip, rows, w = G.nodegraph_csr(ng)
    assert list(np.diff(ip)) == sizes and np.array_equal(rows, np.arange(n)) and ip[z] == ip[z + 1]
    assert ((ng > 0).sum(axis=1) == 1).all()                         # every node in one graph
    for gi, sz in enumerate(sizes):
        if sz > 1: assert w[ip[gi]:ip[gi + 1]].min() >= 0.5 / sz and w[ip[gi]:ip[gi + 1]].max() <= 1.5 / sz and np.ptp(w[ip[gi]:ip[gi + 1]]) > 0


@pytest.mark.parametrize('mode', G.ALL_MODES)
def test_host_chain_and_oracle_agree_on_a_directed_list(mode):
    """GraphObject -> GraphTensor.fromGraphObject (the project's host chain) and oracle.make_graph_dict on the same directed, unsorted arcs: the same
    Adjacency^T and ArcNode^T triples; the by-source triple of adjacency_by_source() (and of the GPU tests' _by_source_csr) = the plain
    transpose of the dense adjacency built from the arc list; edge_readout_arrays() = destinations in entry order, labels in list order."""
    from GNN.graph_class import GraphObject, GraphTensor
    n = G.N_SMALL
    arcs = G.directed_graph(1012, n, degrees=True)
    rng = np.random.default_rng(3)
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    mask = rng.random(len(arcs)) < 0.6
    go = GraphObject(arcs=arcs, nodes=nodes, targets=np.zeros((len(arcs), 1)), problem_based='a', set_mask=mask, aggregation_mode=mode)
    assert np.array_equal(go.arcs, arcs)                            # kept as given
    gt = GraphTensor.fromGraphObject(go)
    g = orc.make_graph_dict(arcs, nodes, mode)
    for mine, theirs in ((gt.Adjacency, g['adjT']), (gt.ArcNode, g['arcT'])):
        assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
        assert np.array_equal(np.asarray(mine[2], np.float32), np.asarray(theirs[2], np.float32))
    assert not np.array_equal(gt.ArcNode[1], np.arange(len(arcs)))
    # dense restatement: A[dst, src] = w (Adjacency^T); its rows are the by-destination triple, the rows of its transpose the by-source one
    src, dst = arcs[:, 0].astype(int), arcs[:, 1].astype(int)
    indeg = np.bincount(dst, minlength=n)
    w = {'sum': np.ones(len(arcs)), 'normalized': np.full(len(arcs), 1 / len(arcs)), 'average': 1 / indeg[dst]}[mode].astype(np.float32)
    dense = np.zeros((n, n), np.float32)
    dense[dst, src] = w

    def rows_of(m):
        r, c = np.nonzero(m)
        ip = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=n), out=ip[1:])
        return ip, c, m[r, c]

    for triple, m in ((gt.Adjacency, dense), (gt.adjacency_by_source(), dense.T)):
        ip, inner, val = rows_of(m)
        assert np.array_equal(triple[0], ip) and np.array_equal(triple[1], inner) and np.array_equal(np.asarray(triple[2], np.float32), val)
    assert not np.array_equal(gt.Adjacency[0], gt.adjacency_by_source()[0])
    from test_gpu_train import _by_source_csr
    for a, b in zip(_by_source_csr(g, n), gt.adjacency_by_source()):
        assert np.array_equal(a, b)
    entry_dst, labels, m2 = gt.edge_readout_arrays()
    assert np.array_equal(entry_dst, np.repeat(np.arange(n), indeg)) and np.array_equal(labels, arcs[:, 2:]) and np.array_equal(m2, mask)
    # ArcNode^T: entry q of destination entry_dst[q] is arc arc_id[q] of the list; inside a row it ascends by arc id where Adjacency^T ascends
    # by source, so on an unsorted list the two pair different arcs by position (the reference's pairing, which the step keeps)
    arc_id = gt.ArcNode[1]
    assert np.array_equal(dst[arc_id], entry_dst) and not np.array_equal(src[arc_id], gt.Adjacency[1])
    assert np.array_equal(np.sort(src[arc_id] + n * entry_dst), gt.Adjacency[1] + n * entry_dst)


def test_oracle_arc_gradient_on_a_directed_edge_case():
    """train_backward(want_d_arcs=True) on a directed edge-based case, float64 and float32: every arc with a non-zero ArcNode weight receives
    gradient, and the float32 evaluation differs from the float64 one - the noise the GPU file scales its bound with is not vacuous."""
    c = G.EDGE_CASES[0]
    arcs = G.case_graph(c)
    rng = np.random.default_rng(c.seed)
    n, ds, nlc = c.n, G.ds_of(c), G.nlc_of(c)
    nodes = (2 * rng.random((n, c.nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    mask, _ = G.edge_mask(arcs, n, c.seed)
    g['set_mask'], g['output_mask'] = mask, np.ones(len(arcs), bool)
    st = make_mlp(rng, G.in_s_of(c), list(c.layers), 'tanh', gain=0.5, batch_normalization=False)
    ou = make_mlp(rng, 2 * (ds + nlc) + c.al, [2], 'softmax', batch_normalization=False)
    st['dropout'], ou['dropout'] = {}, {}
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    d_out = rng.standard_normal((int(mask.sum()), 2)).astype(np.float32)
    dse = rng.standard_normal((n, ds)).astype(np.float32)
    res = {}
    for dt in (np.float64, np.float32):
        ctx = tro.train_forward(g, st, ou, c.d, c.k, 0.0, s0, [{}] * c.k, {}, dtype=dt, edge_based=True)
        assert ctx['k'] == c.k
        res[dt] = tro.train_backward(ctx, d_out.astype(dt), dse.astype(dt), want_d_arcs=True)[3]
    d64, d32 = res[np.float64], res[np.float32]
    assert d64.shape == (len(arcs), c.al) and d32.dtype == np.float32
    w_by_arc = np.zeros(len(arcs))
    w_by_arc[g['arcT'][1]] = g['arcT'][2]
    assert (w_by_arc > 0).all() and (np.abs(d64).max(axis=1) > 0).all()
    noise = np.max(np.abs(d32.astype(np.float64) - d64))
    print(f'd_arcs float32 noise {noise:.3e} against max {np.max(np.abs(d64)):.3e}')
    assert noise > 0
