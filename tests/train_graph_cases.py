"""Directed, unsorted graphs and the case table of tests/test_gpu_train_graph_side.py, shared with tests/test_train_graph_side_host.py (which
checks on the CPU what the builders promise).  Inputs only, no reference code.

On a symmetric arc list the CSR by source and the CSR by destination have the same index arrays, so a kernel that walks the wrong one moves
no index.  directed_graph() returns a list on which the two differ everywhere it matters:

    node 0 (HUB)       many in-arcs and many out-arcs (70 each way, n // 2 on graphs too small for that)
    node 1 (NO_IN)     out-arcs only            node 2 (NO_OUT)    in-arcs only            node 3 (ISOLATED)  no arc
    IN_NODES[i]        in-degree exactly DEGREES[i], at least one out-arc        (degrees=True)
    OUT_NODES[i]       out-degree exactly DEGREES[i], at least one in-arc        (degrees=True)

DEGREES are the edges of the four-arcs-per-step gather loops (0 | 1, 3 | 4 | 5, 8 | 9, 17 = four steps and one arc).  No arc has its reverse in
the list but for the few the hub of a small graph forces (37 nodes: 18 + 18 neighbours out of 35 that may have arcs), at most 5 %; the arcs
come in a random order, so ArcNode's arc ids are an irregular permutation."""
from collections import namedtuple

import numpy as np

from util import random_arcs

HUB, NO_IN, NO_OUT, ISOLATED = 0, 1, 2, 3
DEGREES = (0, 1, 3, 4, 5, 8, 9, 17)
IN_NODES = tuple(range(4, 12))
OUT_NODES = tuple(range(12, 20))
HUB_DEGREE = 70
N_SMALL, N_MANY = 37, 4113          # 4,113 = 128 full 32-row tiles + 17 rows, past the 4,096 rows of the many-row kernels
MIN_ROWS = 4096


def hub_degree(n):
    return HUB_DEGREE if n >= 4 * HUB_DEGREE else n // 2


def csr_pair(arcs, n):
    """(indptr by destination, sources in that order, arc ids in that order), (indptr by source, destinations in that order) of an arc list:
    plain NumPy, what the builder's own assertions and the host test look at."""
    src, dst = np.asarray(arcs)[:, 0].astype(np.int64), np.asarray(arcs)[:, 1].astype(np.int64)
    by_dst = np.lexsort((src, dst))
    by_src = np.lexsort((dst, src))
    ip_d, ip_s = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=ip_d[1:])
    np.cumsum(np.bincount(src, minlength=n), out=ip_s[1:])
    return (ip_d, src[by_dst], by_dst), (ip_s, dst[by_src])


def reverse_fraction(arcs):
    pairs = {(int(s), int(d)) for s, d in np.asarray(arcs)[:, :2]}
    return sum((d, s) in pairs for s, d in pairs) / max(1, len(pairs))


def check_directed(arcs, n, degrees):
    """What directed_graph() promises about its result (asserted there, and once more per case by the host test)."""
    arcs = np.asarray(arcs)
    src, dst = arcs[:, 0].astype(np.int64), arcs[:, 1].astype(np.int64)
    assert src.min() >= 0 and dst.min() >= 0 and max(src.max(), dst.max()) < n
    assert not (src == dst).any() and len({(int(s), int(d)) for s, d in zip(src, dst)}) == len(arcs)
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert indeg[NO_IN] == 0 and outdeg[NO_IN] > 0 and outdeg[NO_OUT] == 0 and indeg[NO_OUT] > 0
    assert indeg[ISOLATED] == 0 and outdeg[ISOLATED] == 0
    assert indeg[HUB] >= hub_degree(n) and outdeg[HUB] >= hub_degree(n)
    if degrees:
        assert tuple(indeg[list(IN_NODES)]) == DEGREES and tuple(outdeg[list(OUT_NODES)]) == DEGREES
        assert (outdeg[list(IN_NODES)] > 0).all() and (indeg[list(OUT_NODES)] > 0).all()
    (ip_d, src_d, arc_id), (ip_s, dst_s) = csr_pair(arcs, n)
    assert not np.array_equal(ip_d, ip_s)
    assert not np.array_equal(arc_id, np.arange(len(arcs)))
    assert not np.array_equal(np.lexsort((dst, src)), np.arange(len(arcs)))           # not (source, destination)-sorted either
    assert reverse_fraction(arcs) <= 0.05, reverse_fraction(arcs)


def directed_graph(seed, n, degrees=None, al=2):
    """Unsorted, duplicate-free, self-loop-free, non-symmetric arc list [src, dst, al labels] (float32) with the fixed nodes of the module
    docstring; about two arcs per node.  degrees: anything true pins the in-degrees of IN_NODES and the out-degrees of OUT_NODES to DEGREES."""
    assert n >= 37
    rng = np.random.default_rng(seed)
    base = random_arcs(rng, n, 2 * n, 0, symmetric=False, sort=False)[:, :2].astype(np.int64)      # every unordered pair at most once ...
    flip = rng.random(len(base)) < 0.5                                                               # ... so neither direction has a reverse
    base[flip] = base[flip][:, ::-1]
    fixed = {HUB, NO_IN, NO_OUT, ISOLATED} | (set(IN_NODES) | set(OUT_NODES) if degrees else set())
    have = {(int(s), int(d)) for s, d in base if s not in fixed and d not in fixed}
    indeg, outdeg = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for s, d in have:
        outdeg[s] += 1; indeg[d] += 1
    big = 1 << 30
    cap_in, cap_out = np.full(n, big), np.full(n, big)
    cap_in[[NO_IN, ISOLATED]] = 0
    cap_out[[NO_OUT, ISOLATED]] = 0
    if degrees:
        cap_in[list(IN_NODES)] = DEGREES
        cap_out[list(OUT_NODES)] = DEGREES

    def fill(v, want, incoming):
        """arcs into (incoming) or out of v until it has `want` of them; partners in random order, those without a reverse arc first"""
        deg = indeg if incoming else outdeg
        order = rng.permutation(n)
        for allow_reverse in (False, True):
            for u in order:
                if deg[v] >= want: return
                u = int(u)
                s, d = (u, v) if incoming else (v, u)
                if u == v or (s, d) in have or ((d, s) in have and not allow_reverse): continue
                if outdeg[s] >= cap_out[s] or indeg[d] >= cap_in[d]: continue
                have.add((s, d))
                outdeg[s] += 1; indeg[d] += 1
        assert deg[v] >= want, (v, want, incoming)

    if degrees:                                         # the most demanding nodes first
        for i in reversed(range(len(DEGREES))):
            fill(IN_NODES[i], DEGREES[i], True)
            fill(OUT_NODES[i], DEGREES[i], False)
            if DEGREES[i] == 17:                        # the hub right behind the largest degrees: partners are still plentiful
                fill(HUB, hub_degree(n), True); fill(HUB, hub_degree(n), False)
        for v in IN_NODES: fill(v, 1, False)
        for v in OUT_NODES: fill(v, 1, True)
    fill(HUB, hub_degree(n), True); fill(HUB, hub_degree(n), False)
    fill(NO_IN, 2, False); fill(NO_OUT, 2, True)
    ids = np.array(sorted(have), np.int64)
    ids = ids[rng.permutation(len(ids))]
    lab = 2 * rng.random((len(ids), al)) - 1
    arcs = np.concatenate([ids.astype(np.float64), lab], axis=1).astype(np.float32)
    check_directed(arcs, n, degrees)
    return arcs


def _closure(arcs, n, rows, k, forward):
    arcs = np.asarray(arcs['arcs'] if isinstance(arcs, dict) else arcs)
    a, b = (0, 1) if forward else (1, 0)
    frm, to = arcs[:, a].astype(np.int64), arcs[:, b].astype(np.int64)
    reach = np.zeros(n, bool)
    reach[np.asarray(rows, np.int64)] = True
    for _ in range(k):
        reach[to[reach[frm]]] = True
    return reach


def predecessors(g, rows, k, n=None):
    """Mask of the nodes from which `rows` are reached along at most k arcs (the rows themselves included).  g: arc list or graph dict."""
    return _closure(g, n if n is not None else len(g['nodes']), rows, k, False)


def successors(g, rows, k, n=None):
    """Mask of the nodes reached from `rows` along at most k arcs (the rows themselves included)."""
    return _closure(g, n if n is not None else len(g['nodes']), rows, k, True)


def graph_sizes(n):
    """Node counts of the graphs of a graph-based step on n nodes, in node order: 1, 63, 64, 65 and 130 nodes (one lane, one short of a wave's
    stride, the stride, one more, two strides and two entries), an EMPTY graph between two non-empty ones (a duplicate entry of the CSR's
    row pointers, where the backward's bisection has its tie) and one graph for the rest - 7 graphs: the second block of a four-graphs-per-block
    kernel runs three waves.  On fewer than 324 nodes the same layout in small: 1, 5, 7, 9, 4, empty, rest."""
    head = [1, 63, 64, 65, 130] if n > 323 else [1, 5, 7, 9, 4]
    assert n > sum(head)
    return head + [0, n - sum(head)]


def node_graph(rng, n):
    """NodeGraph [n, 7] of graph_sizes(n): non-uniform weights, random in 0.5 .. 1.5 over the graph's size."""
    sizes = graph_sizes(n)
    ng = np.zeros((n, len(sizes)), np.float32)
    r0 = 0
    for gi, sz in enumerate(sizes):
        if sz: ng[r0:r0 + sz, gi] = rng.uniform(0.5, 1.5, sz) / sz
        r0 += sz
    return ng


def nodegraph_csr(ng):
    """NodeGraph^T as CSR over graphs, as GraphTensor.nodegraph_csr() builds it"""
    cols, rows = np.nonzero(ng.T)
    ip = np.zeros(ng.shape[1] + 1, np.int32)
    np.cumsum(np.bincount(cols, minlength=ng.shape[1]), out=ip[1:])
    return ip, rows.astype(np.int32), ng[rows, cols].astype(np.float32)


# --- the case table ----------------------------------------------------------------------------------------------------------------------------------
# d: state_vect_dim (0: the labels are the state), nl: node-label width, al: arc-label width, layers: net_state; drop0: Dropout rate in front of
# layer 0; k: max_iteration (threshold 0: all of them run); modes: aggregation modes; expected form (loop.train_forms(0)): fwd per layer letter
# (P per-op, M k_mlp_fwd, C k_fwd3_split), bwd (P k_layer_bwd, C k_bwd3_split), build: k_mlp_fwd builds the concat itself;
# input / gather: the kernels the rule of Forward::enqueue_body and the tail of net_backward then pick (derived in expected_kernels below).
Case = namedtuple('Case', 'name n d nl al layers drop0 k modes fwd bwd build seed')
ALL_MODES = ('average', 'sum', 'normalized')
WIDE3 = (128, 128, 64)              # the nets of train_form_cases.WIDE3: concat 135 = 1 + 2 (64 + 3)

CASES = [
    Case('built_rows', N_SMALL, 4, 3, 2, (7, 4), 0.0, 3, ALL_MODES, 'MM', 'PP', True, 111),
    Case('input_float4', N_SMALL, 4, 3, 2, (4,), 0.0, 3, ('average',), 'P', 'P', False, 12),
    Case('input_scalar', N_SMALL, 3, 3, 2, (3,), 0.0, 3, ('average',), 'P', 'P', False, 13),
    Case('input_dropout', N_SMALL, 4, 3, 2, (7, 4), 0.2, 3, ('average',), 'MM', 'PP', False, 14),
    Case('labels_as_state', N_SMALL, 0, 3, 2, (7, 3), 0.0, 3, ('average',), 'MM', 'PP', True, 15),
    Case('rows16', N_MANY, 4, 3, 2, (7, 4), 0.0, 3, ALL_MODES, 'PP', 'PP', False, 16),
    Case('many_scalar', N_MANY, 3, 3, 2, (7, 3), 0.0, 3, ('average',), 'PP', 'PP', False, 17),
    Case('chain_aligned', N_MANY, 64, 3, 1, WIDE3, 0.0, 1, ('average',), 'CCC', 'CCC', False, 18),
    Case('edge_4095', MIN_ROWS - 1, 4, 3, 2, (7, 4), 0.0, 3, ('average',), 'MM', 'PP', True, 19),
]
# edge-based: the two row regimes, with a state of its own and with the labels as state (nl = 4 there: the many-row kernels need Ds % 4 == 0)
EDGE_CASES = [
    Case('edge_built_rows_d4', N_SMALL, 4, 3, 2, (7, 4), 0.0, 3, ('average',), 'MM', 'PP', True, 21),
    Case('edge_built_rows_d0', N_SMALL, 0, 4, 2, (7, 4), 0.0, 3, ('average',), 'MM', 'PP', True, 22),
    Case('edge_rows16_d4', N_MANY, 4, 3, 2, (7, 4), 0.0, 3, ('average',), 'PP', 'PP', False, 123),
    Case('edge_rows16_d0', N_MANY, 0, 4, 2, (7, 4), 0.0, 3, ('average',), 'PP', 'PP', False, 24),
]
# graph readout inside the step: (nodes, T); T = 1: sigmoid head and mean_squared_error, T = 2, 3: softmax and categorical_crossentropy
GRAPH_CASES = [(n, t) for n in (N_SMALL, N_MANY) for t in (1, 2, 3)]


def ds_of(c): return c.d if c.d else c.nl
def nlc_of(c): return c.nl if c.d else 0
def in_s_of(c): return c.al + 2 * (ds_of(c) + nlc_of(c))
def dims_of(c): return (in_s_of(c),) + tuple(c.layers)


def expected_kernels(c):
    """(concat kernel, state-gradient kernel) of a case, restated from the engine's rule: k_mlp_fwd builds the concat where the net decided so;
    else the 16-lanes-per-row kernel on many rows of a state with Ds % 4 == 0, Ds <= 64 and no Dropout in front of layer 0; else k_train_input,
    whose gather takes float4 pieces when Ds % 4 == 0 and no Dropout sits in front, single floats otherwise.  Backward: the aligned-rows gather
    behind k_bwd3_split, the rows gather under the same many-rows condition, else k_state_grad_sum."""
    ds, many = ds_of(c), c.n >= MIN_ROWS
    rows16 = ds % 4 == 0 and ds <= 64 and many
    if c.build: inp = 'k_mlp_fwd'
    elif c.drop0 == 0.0 and rows16: inp = 'k_train_input_rows'
    elif c.drop0 != 0.0: inp = 'k_train_input scalar+dropout'
    else: inp = 'k_train_input float4' if ds % 4 == 0 else 'k_train_input scalar'
    if c.bwd == 'CCC' and rows16: grad = 'k_state_grad_rows_al'
    else: grad = 'k_state_grad_rows' if rows16 else 'k_state_grad_sum'
    return inp, grad


EXPECTED_KERNELS = {
    'built_rows': ('k_mlp_fwd', 'k_state_grad_sum'), 'input_float4': ('k_train_input float4', 'k_state_grad_sum'),
    'input_scalar': ('k_train_input scalar', 'k_state_grad_sum'), 'input_dropout': ('k_train_input scalar+dropout', 'k_state_grad_sum'),
    'labels_as_state': ('k_mlp_fwd', 'k_state_grad_sum'), 'rows16': ('k_train_input_rows', 'k_state_grad_rows'),
    'many_scalar': ('k_train_input scalar', 'k_state_grad_sum'), 'chain_aligned': ('k_train_input_rows', 'k_state_grad_rows_al'),
    'edge_4095': ('k_mlp_fwd', 'k_state_grad_sum'),
}

SENTINELS_SMALL = ('hub', 'no_in', 'no_out')
SENTINELS_MANY = SENTINELS_SMALL + ('tile_edge', 'last17')


def sentinel_sets(c):
    return SENTINELS_MANY if c.n >= MIN_ROWS - 1 else SENTINELS_SMALL


def sentinel_rows(c, sset):
    return {'hub': np.array([HUB]), 'no_in': np.array([NO_IN]), 'no_out': np.array([NO_OUT]), 'tile_edge': np.arange(31, 33),
            'last17': np.arange(c.n - 17, c.n)}[sset]


def case_graph(c):
    """The directed graph of a case (every case pins the degrees)"""
    return directed_graph(1000 + c.seed, c.n, degrees=True, al=c.al)


def edge_mask(arcs, n, seed):
    """Arc mask of the edge-based cases, about 60 % in.  A mask position p selects ENTRY p of Adjacency^T (destination-major order) and arc p
    of the list (the reference pairs them by position), so the endpoints below are those of entry p:
      a lonely node (of the free range, with arcs) has no masked entry;  the hub is destination of >= 30 masked entries and source of >= 30
      (37 nodes: >= 16 of its 18 each way);  NO_IN's only masked entry has it as source;  NO_OUT's only masked entry has it as destination.
    Returns (mask, lonely node); asserted here and in the host test."""
    rng = np.random.default_rng(seed)
    (ip_d, src_c, _), _ = csr_pair(arcs, n)
    dst_c = np.repeat(np.arange(n), np.diff(ip_d))
    mask = rng.random(len(src_c)) < 0.6
    lonely = 20 + int(np.argmax((np.bincount(src_c, minlength=n) + np.bincount(dst_c, minlength=n))[20:] > 0))
    mask[(src_c == HUB) | (dst_c == HUB)] = True
    mask[(src_c == lonely) | (dst_c == lonely)] = False
    for v, ends in ((NO_IN, src_c), (NO_OUT, dst_c)):
        own = np.nonzero(ends == v)[0]
        own = own[(src_c[own] != lonely) & (dst_c[own] != lonely)]
        at_hub = own[(src_c[own] == HUB) | (dst_c[own] == HUB)]          # (its arc with the hub where it has one: the hub keeps its count)
        mask[ends == v] = False
        mask[at_hub[0] if len(at_hub) else own[0]] = True
    check_edge_mask(arcs, n, mask, lonely)
    return mask, lonely


def check_edge_mask(arcs, n, mask, lonely):
    (ip_d, src_c, _), _ = csr_pair(arcs, n)
    dst_c = np.repeat(np.arange(n), np.diff(ip_d))
    as_src, as_dst = np.bincount(src_c[mask], minlength=n), np.bincount(dst_c[mask], minlength=n)
    assert as_src[lonely] == 0 and as_dst[lonely] == 0 and (np.bincount(src_c, minlength=n) + np.bincount(dst_c, minlength=n))[lonely] > 0
    want = min(30, hub_degree(n) - 2)                  # (a 37-node hub has 18 arcs each way, of which the lonely node may take one or two)
    assert as_dst[HUB] >= want and as_src[HUB] >= want
    assert as_src[NO_IN] == 1 and as_dst[NO_IN] == 0 and as_dst[NO_OUT] == 1 and as_src[NO_OUT] == 0
    assert 0.45 <= mask.mean() <= 0.75, mask.mean()
