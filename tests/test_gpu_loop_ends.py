"""The two ends of a Loop where the rest of the suite reaches them in one configuration only.

1. OUTPUT STAGE.  apply_filters + net_output (reference GNN/GNN.py:275-279) exists four times: k_out1 (csrc/gnn_loop.hip: one-layer head,
   T <= 8, at most 64 KiB of LDS), small_output_stage (csrc/gnn_small_common.h: the same head folded into the persistent launch, in the
   families k_small_loop / k_small16 / wide k_small16 and their "mixed" variants), k_feats + launch_mlp (everything else) and the edge-based
   k_feats_edge.  Every other test builds the head as [2] with softmax; here T = 1, 3, 5, 8, 9 and a two-layer head, every head
   activation, with and without BatchNormalization, odd state widths, a saturating softmax, and masks that end on a row-block or tile edge.
2. GRAPH READOUT (GNN.py:331-332): k_readout and the copy folded into the persistent launch (small_graph_readout: eight entries at a time
   behind a clamp, G * T lanes in passes of 64), with graphs of 0, 1, 7, 8, 9, 16, 17 nodes, weights that are not 1 / size and T = 1, 3, 8.
3. STOP CONTROL: the per-body path reads one gate on the host every GNN_BODY_CHUNK = 16 bodies and k_finalize finds k with one ballot per 64
   gates; the persistent launch double-buffers its gate words by run parity.  One slowly contracting case stops at bodies 15 .. 129, at the
   chunk and ballot boundaries, with a borderline gate in the first and in the second pass of the scan, on loopback groups and on one handle
   run long, short, long.

References: oracle.c_oracle (loop_node, readout: the pinned evaluation order - impl 0, impl 1 and every persistent launch must return its
bits) and oracle.gnn_oracle in float64 (impl 2 on one launch per body: the bounds of test_gpu_parity.py, 1e-5 against float64 and
2e-6 max(1, max|s|) against the exact chain)."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine():
    from GNN import _engine
    return _engine


def _loop_node(g, st, ou, d, max_it, thr, s0, want_out=True):
    """corc.loop_node; the few hundred rows of these cases on one thread (a team of threads costs more than the work; same bits)"""
    return corc.loop_node(g, st, ou, d, max_it, thr, s0, n_threads=1 if g['nodes'].shape[0] < 2000 else 0, want_out=want_out)


def _dims(net):
    return [net['weights'][0].shape[0]] + [net['weights'][2 * i].shape[1] for i in range(len(net['activations']))]


def _device(e, g, st, ou, mask=None):
    """(Graph, net_state, net_output) handles of a case; mask: the rows with an output (default: set_mask & output_mask of g)"""
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    if mask is None: mask = np.logical_and(g['set_mask'], g['output_mask'])
    graph = e.Graph(g['nodes'].shape[0], g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]], g['nodes'], mask)
    return graph, e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], ou['batch_normalization'])


def _exact_twice(loop, want, what):
    """two runs of one handle (staging that survives only a first run): k, state and output are the C oracle's, shape and bits"""
    kc, sc, oc = want
    for rep in range(2):
        k, s, o = loop.run(), loop.state(), loop.output()
        assert k == kc, (what, rep, k, kc)
        assert s.shape == sc.shape and np.array_equal(s, sc), (what, rep, 'state', int(np.sum(s != sc)))
        assert o.shape == oc.shape and np.array_equal(o, oc), (what, rep, 'output', o.shape, oc.shape, int(np.sum(o != oc)) if o.shape == oc.shape else -1)


def _close_twice(loop, want, want64, what):
    """impl 2 on one launch per body: the oracle's k, values within the bounds of test_gpu_parity.py - 1e-5 of the float64 oracle, and
    2e-6 max(1, max|s|) of the exact chain (impl 1 returns the C oracle's bits - asserted beside this - so `want` stands for it) - and the
    same bits on both runs of the handle"""
    kc, sc, oc = want
    _, s64, o64 = want64
    first = None
    for rep in range(2):
        k, s, o = loop.run(), loop.state(), loop.output()
        e_s64, e_o64 = float(np.max(np.abs(s - s64))), (float(np.max(np.abs(o - o64))) if o.size else 0.0)
        e_s1 = float(np.max(np.abs(s - sc)))
        print(f'{what} run {rep}: k {k} (oracle {kc}), |s - s64| {e_s64:.2e}, |o - o64| {e_o64:.2e}, |s - s1| {e_s1:.2e}')
        assert k == kc, (what, rep, k, kc)
        assert o.shape == oc.shape, (what, o.shape, oc.shape)
        assert e_s64 < 1e-5 and e_o64 < 1e-5, (what, rep, e_s64, e_o64)
        assert e_s1 < 2e-6 * max(1.0, float(np.max(np.abs(sc)))), (what, rep, e_s1)
        if first is None: first = (s, o)
        else: assert np.array_equal(s, first[0]) and np.array_equal(o, first[1]), (what, 'second run differs from the first')


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. output heads on every output-stage implementation
# ----------------------------------------------------------------------------------------------------------------------------------------
GATE = (30, 0.01)      # max_iteration, threshold of parts 1 and 2

# id: seed, n, d, NL, hidden layers of net_state, its activations (one name, or the whole list), form, impls
#   form 'bodies': one launch per body with the persistent launch forbidden; 'bodies_only': there is no persistent form for the net;
#   16 / 32 / '16w': the persistent launch on 16-node tiles, 32-node tiles, or 16-node tiles with hidden layers up to 64 wide
PATHS = {
    'bodies_out1': (9101, 333, 8, 3, (16,), 'selu', 'bodies', (0, 1, 2)),
    'bodies_wide_net': (9102, 333, 64, 3, (128, 128), 'selu', 'bodies_only', (1, 2)),
    'small16': (9101, 333, 8, 3, (16,), 'selu', 16, (1, 2)),
    'small32': (9103, 4129, 8, 3, (16,), 'selu', 32, (1, 2)),          # 130 tiles of 32 nodes, the last with one row
    'small16w': (9104, 333, 8, 3, (64, 64), 'selu', '16w', (1, 2)),
    'small16_mixed': (9105, 333, 8, 3, (16,), ('tanh', 'linear'), 16, (1, 2)),
}
# the n = 333 extras: the scalar row path of k_out1 and odd Ds in the folded head (d = 5, 7); the state IS the node labels, NLc = 0 (d = 0)
EXTRA_PATHS = {}
for _d, _nl in ((5, 3), (7, 3), (0, 6)):
    EXTRA_PATHS[f'bodies_out1_d{_d}'] = (9110 + _d, 333, _d, _nl, (16,), 'selu', 'bodies', (0, 1, 2))
    EXTRA_PATHS[f'small16_d{_d}'] = (9110 + _d, 333, _d, _nl, (16,), 'selu', 16, (1, 2))
    EXTRA_PATHS[f'small16w_d{_d}'] = (9120 + _d, 333, _d, _nl, (64, 64), 'selu', '16w', (1, 2))
ALL_PATHS = dict(PATHS, **EXTRA_PATHS)

# id: layer widths, activation of the hidden layers, of the last layer, BatchNormalization, factor on the weights
HEADS = {
    't1_sigmoid': ([1], None, 'sigmoid', False, 1.0),
    't1_softmax_bn': ([1], None, 'softmax', True, 1.0),
    't3_softmax_bn': ([3], None, 'softmax', True, 1.0),
    't5_tanh': ([5], None, 'tanh', False, 1.0),
    't8_softmax_bn': ([8], None, 'softmax', True, 1.0),
    't8_linear': ([8], None, 'linear', False, 1.0),
    't9_softmax_bn': ([9], None, 'softmax', True, 1.0),               # T = 9: k_feats + launch_mlp, also behind a persistent launch
    't7_3_tanh_softmax_bn': ([7, 3], 'tanh', 'softmax', True, 1.0),   # two layers: k_feats + launch_mlp
    't3_softmax_x200': ([3], None, 'softmax', False, 200.0),          # saturating rows: exp underflows to 0, one output is exactly 1
}
GRID = [h for h in HEADS if h != 't3_softmax_x200']
EXTRA_HEADS = ['t3_softmax_bn', 't5_tanh', 't8_softmax_bn']


@functools.lru_cache(maxsize=None)
def _net_case(seed, n, d, nl, hidden, acts):
    """A seeded random graph (two arc-label columns, 'average' aggregation), an 80 % set_mask and a 70 % output_mask, net_state with random
    BatchNormalization statistics, and the initial state.  Built once per key and never changed."""
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 3 * n, 2)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    ds, nlc = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, 2 + 2 * (ds + nlc), list(hidden) + [ds], acts if isinstance(acts, str) else 'selu', gain=0.6, bn_random=True)
    if not isinstance(acts, str): st['activations'] = list(acts)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
    g['set_mask'] = rng.random(n) < 0.8
    g['output_mask'] = rng.random(n) < 0.7
    return g, st, s0


@functools.lru_cache(maxsize=None)
def _head(seed, wf, head):
    layers, act, out_act, bn, factor = HEADS[head]
    rng = np.random.default_rng([seed, sorted(HEADS).index(head)])
    ou = make_mlp(rng, wf, layers, act if act else out_act, batch_normalization=bn, out_activation=out_act, bn_random=True)
    if factor != 1.0:
        for i in range(0, 2 * len(layers), 2): ou['weights'][i] = (ou['weights'][i] * np.float32(factor)).astype(np.float32)
    return ou


def _masked(g, mask):
    """the case with another output mask (the states do not depend on it)"""
    return dict(g, set_mask=np.asarray(mask, bool), output_mask=np.ones(len(mask), bool))


@functools.lru_cache(maxsize=None)
def _want(key, head, mask_id=None):
    g, st, s0 = _net_case(*key)
    if mask_id is not None: g = _masked(g, _mask(key, mask_id))
    ou = _head(key[0], _dims(st)[-1] + (g['nodes'].shape[1] if key[2] else 0), head)
    return _loop_node(g, st, ou, key[2], GATE[0], GATE[1], s0)


@functools.lru_cache(maxsize=None)
def _want64(key, head):
    g, st, s0 = _net_case(*key)
    ou = _head(key[0], _dims(st)[-1] + (g['nodes'].shape[1] if key[2] else 0), head)
    return orc.loop_node(g, st, ou, key[2], GATE[0], GATE[1], s0, np.float64)


def _new_loop(e, handles, d, s0, form, impl, max_it=GATE[0], thr=GATE[1]):
    """a Loop on the form asked for; WHICH form it takes is asserted from the setters' answers, not assumed"""
    graph, mst, mou = handles
    loop = e.Loop(graph, mst, mou, d, max_it, thr)
    assert loop.set_impl(impl) == impl, (form, impl)
    if form == 'bodies': assert loop.set_persistent(False) is False
    elif form == 'bodies_only': assert loop.set_persistent(True) is False, 'this net has no persistent form'
    else: assert loop.set_persistent(True) is True, (form, impl)
    if d: loop.set_state0(s0)
    return loop


def _assert_form(e, st, n, nlc, form):
    """the persistent form small_form gives the net on n rows is the one the case is named after"""
    f = e.small_form(_dims(st), st['activations'], n, nlc)
    if form == 'bodies_only':
        assert not f['persistent'], f
        return
    want = {'bodies': (16, False), 16: (16, False), 32: (32, False), '16w': (16, True)}[form]
    assert f['persistent'] and (f['tile'], f['wide']) == want, (form, f)


def _out1_lds_bytes(wf, t):
    """dynamic LDS of k_out1 (csrc/gnn_loop.hip, loop_finish): W and b, 64 feature rows of odd stride, 64 rows of T sums"""
    return 4 * ((wf + 1) * t + 64 * (wf | 1) + 64 * t)


def _check_heads(path, head, mask_id=None, impls=None):
    e = _engine()
    seed, n, d, nl, hidden, acts, form, path_impls = ALL_PATHS[path]
    key = (seed, n, d, nl, hidden, acts)
    g, st, s0 = _net_case(*key)
    nlc = nl if d else 0
    _assert_form(e, st, n, nlc, form)
    if not isinstance(acts, str):
        assert e.fused_net_form(_dims(st), st['activations'], nlc)['mixed']
    ou = _head(seed, _dims(st)[-1] + nlc, head)
    want = _want(key, head, mask_id)
    mask = None if mask_id is None else _mask(key, mask_id)
    if mask is not None: assert want[2].shape == (int(mask.sum()), _dims(ou)[-1])
    handles = _device(e, g, st, ou, mask)
    persistent = form in (16, 32, '16w')
    for impl in (impls or path_impls):
        loop = _new_loop(e, handles, d, s0, form, impl)
        what = f'{path} / {head} / impl {impl}' + (f' / mask {mask_id}' if mask_id else '')
        if impl == 2 and not persistent:
            _close_twice(loop, want, _want64(key, head), what)
        else:
            _exact_twice(loop, want, what)
        if persistent: assert loop.set_persistent(True) is True, (what, 'the launch gave up')
        loop.close()
    handles[0].close()


@pytest.mark.parametrize('head', GRID)
@pytest.mark.parametrize('path', sorted(PATHS))
def test_output_heads(path, head):
    """Every head of the grid on every implementation of the output stage.  A one-layer head of T <= 8 is k_out1 behind one launch per body
    and small_output_stage inside a persistent launch; T = 9 and the two-layer head are k_feats + launch_mlp on both."""
    _check_heads(path, head)


@pytest.mark.parametrize('head', EXTRA_HEADS)
@pytest.mark.parametrize('path', sorted(EXTRA_PATHS))
def test_output_heads_odd_state_widths(path, head):
    """State widths 5 and 7 (the scalar row path of k_out1: Ds % 4 != 0; odd Ds in the folded head) and state = node labels (d = 0 with
    NL = 6: no label columns in the features, NLc = 0)."""
    _check_heads(path, head)


@pytest.mark.parametrize('path', ['bodies_out1', 'small16', 'small16w', 'small16_mixed'])
def test_output_head_saturating_softmax(path):
    """Head weights times 200: rows of the softmax saturate (gnn_expf underflows to 0, one output is exactly 1).  The C oracle restates the
    same expf, so the exact paths still return its bits: impl 0 and 1 on one launch per body, impl 1 and 2 on a persistent launch (impl 2 on
    one launch per body is compared by value, and a value bound says nothing about logits this large)."""
    key, form = ALL_PATHS[path][:6], ALL_PATHS[path][6]
    o = _want(key, 't3_softmax_x200')[2]
    assert np.any(o == 1.0) and np.any(o == 0.0) and not np.isnan(o).any()
    _check_heads(path, 't3_softmax_x200', impls=(0, 1) if form == 'bodies' else (1, 2))


def test_output_head_too_large_for_out1():
    """T = 8 on 230 feature columns (d = 0, NL = 230): k_out1 would need more than 64 KiB of LDS, so the per-op path (impl 0) takes k_feats +
    launch_mlp for a head that otherwise qualifies.  100 nodes."""
    e = _engine()
    assert _out1_lds_bytes(230, 8) > 64 * 1024 >= _out1_lds_bytes(218, 8)
    rng = np.random.default_rng(9130)
    n, nl = 100, 230
    g = orc.make_graph_dict(random_arcs(rng, n, 3 * n, 2), (2 * rng.random((n, nl)) - 1).astype(np.float32), 'average')
    st = make_mlp(rng, 2 + 2 * nl, [16, nl], 'tanh', gain=0.6, bn_random=True)
    ou = make_mlp(rng, nl, [8], 'softmax', bn_random=True)
    g['set_mask'], g['output_mask'] = rng.random(n) < 0.8, rng.random(n) < 0.7
    want = _loop_node(g, st, ou, 0, 10, 0.01, None)
    handles = _device(e, g, st, ou)
    loop = e.Loop(handles[0], handles[1], handles[2], 0, 10, 0.01)
    assert loop.set_impl(0) == 0
    _exact_twice(loop, want, 'NL = 230, T = 8, impl 0')
    loop.close()
    handles[0].close()


MASKS = ['none', 'one', 'rows_64', 'rows_65', 'tile_without_rows', 'last_row_of_tile']


@functools.lru_cache(maxsize=None)
def _mask(key, mask_id):
    """Output masks at the edges: no row, one row, 64 and 65 rows (the row block of k_out1), a 16-node tile without a masked row, and tiles
    (a full one and the partial last one) whose only masked row is their last."""
    n = key[1]
    rng = np.random.default_rng([key[0], MASKS.index(mask_id)])
    m = np.zeros(n, bool)
    if mask_id == 'one': m[200] = True
    elif mask_id in ('rows_64', 'rows_65'): m[rng.choice(n, 64 if mask_id == 'rows_64' else 65, replace=False)] = True
    elif mask_id == 'tile_without_rows':
        m = rng.random(n) < 0.6
        m[32:48] = False
    elif mask_id == 'last_row_of_tile':
        m = rng.random(n) < 0.6
        m[48:64] = False; m[63] = True
        m[n - n % 16:] = False; m[n - 1] = True
    return m


@pytest.mark.parametrize('mask_id', MASKS)
@pytest.mark.parametrize('path', ['bodies_out1', 'small16'])
def test_output_mask_edges(path, mask_id):
    """T = 3 behind k_out1 (blocks of 64 masked rows, three threads per row) and in the folded head (out_pos through the mask, a tile at a time)"""
    assert ALL_PATHS[path][1] % 16                          # (the last tile is partial)
    m = _mask(ALL_PATHS[path][:6], mask_id)
    if mask_id in ('none', 'one', 'rows_64', 'rows_65'): assert int(m.sum()) == {'none': 0, 'one': 1, 'rows_64': 64, 'rows_65': 65}[mask_id]
    _check_heads(path, 't3_softmax_bn', mask_id, impls=(0, 1) if path == 'bodies_out1' else (1, 2))
    if mask_id == 'none': assert _want(ALL_PATHS[path][:6], 't3_softmax_bn', mask_id)[2].shape == (0, 3)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. graph readout, folded into the persistent launch and not
# ----------------------------------------------------------------------------------------------------------------------------------------
def _node_graph(rng, n, sizes_fixed, n_graphs):
    """dense NodeGraph [n, G] of consecutive node ranges with random weights in (0.5, 1.5), and its CSR over graphs: the sizes asked for,
    in random order among graphs that share the remaining nodes"""
    rest = n - sum(sizes_fixed)
    n_rest = n_graphs - len(sizes_fixed)
    cuts = np.sort(rng.choice(np.arange(1, rest), n_rest - 1, replace=False))
    sizes = list(sizes_fixed) + list(np.diff(np.concatenate([[0], cuts, [rest]])))
    sizes = [int(sizes[i]) for i in rng.permutation(n_graphs)]
    assert sum(sizes) == n and len(sizes) == n_graphs
    ng = np.zeros((n, n_graphs), np.float32)
    ip = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for gi in range(n_graphs): ng[ip[gi]:ip[gi + 1], gi] = rng.uniform(0.5, 1.5, sizes[gi]).astype(np.float32)
    return ng, sizes


def _ng_csr(ng):
    ip, node, w = [0], [], []
    for gi in range(ng.shape[1]):
        rows = np.nonzero(ng[:, gi])[0]
        node += list(rows); w += list(ng[rows, gi]); ip.append(len(node))
    return np.asarray(ip, np.int32), np.asarray(node, np.int32), np.asarray(w, np.float32)


@pytest.mark.parametrize('head', ['t1_sigmoid', 't3_softmax_bn', 't8_softmax_bn'])
@pytest.mark.parametrize('path', ['bodies_out1', 'small16'])
def test_graph_readout_folded_and_not(path, head):
    """G = 40 graphs, among them graphs of 0, 1, 7, 8, 9, 16 and 17 nodes (the ends of the eight-at-a-time loop of the folded readout), random
    weights; T = 1, 3, 8: G T = 40, 120, 320 lanes, one, two and five passes of 64.  First readout of a handle: k_readout.  From the second
    run on, a persistent launch computes it itself (the NodeGraph is cached with the loop).  Other weights on the same structure, and
    another G, must be noticed.  Every result is corc.readout of the dense NodeGraph and the node outputs, bit for bit."""
    e = _engine()
    seed, n, d, nl, hidden, acts, form, _ = ALL_PATHS[path]
    key = (seed, n, d, nl, hidden, acts)
    g, st, s0 = _net_case(*key)
    all_true = np.ones(n, bool)
    ou = _head(seed, d + nl, head)
    T = _dims(ou)[-1]
    want = _loop_node(_masked(g, all_true), st, ou, d, GATE[0], GATE[1], s0)
    rng = np.random.default_rng([seed, 40])
    ng, sizes = _node_graph(rng, n, [0, 1, 7, 8, 9, 16, 17], 40)
    assert {0, 1, 7, 8, 9, 16, 17} <= set(sizes)
    ng_w2 = (ng * rng.uniform(0.5, 1.5, ng.shape)).astype(np.float32)                  # the same structure, other weights
    ng13, sizes13 = _node_graph(rng, n, [0, 25], 13)                                   # another G
    csr, csr_w2, csr13 = _ng_csr(ng), _ng_csr(ng_w2), _ng_csr(ng13)
    assert np.array_equal(csr[0], csr_w2[0]) and np.array_equal(csr[1], csr_w2[1]) and not np.array_equal(csr[2], csr_w2[2])
    ref, ref_w2, ref13 = corc.readout(ng, want[2]), corc.readout(ng_w2, want[2]), corc.readout(ng13, want[2])
    assert ref.shape == (40, T) and not np.array_equal(ref, ref_w2)
    handles = _device(e, g, st, ou, all_true)
    for impl in (1, 2) if form == 16 else (0, 1):
        loop = _new_loop(e, handles, d, s0, form, impl)
        what = f'{path} / {head} / impl {impl}'

        def run_and_read(c):
            k = loop.run()
            assert k == want[0] and np.array_equal(loop.output(), want[2]), what
            return loop.readout(*c)

        r1 = run_and_read(csr)                              # nothing cached yet: k_readout
        r2 = run_and_read(csr)                              # cached: inside the persistent launch, from pinned memory
        assert r1.shape == ref.shape and np.array_equal(r1, ref), (what, 'first readout', int(np.sum(r1 != ref)))
        assert np.array_equal(r2, ref), (what, 'second readout', int(np.sum(r2 != ref)))
        assert np.array_equal(r2, r1), what
        r3 = loop.readout(*csr_w2)                          # other weights: recomputed, not the cached result
        assert np.array_equal(r3, ref_w2), (what, 'other weights', int(np.sum(r3 != ref_w2)))
        r4 = run_and_read(csr_w2)                           # ... and folded in with them
        assert np.array_equal(r4, ref_w2), (what, 'other weights, second readout')
        r5 = loop.readout(*csr13)                           # another G
        assert r5.shape == (13, T) and np.array_equal(r5, ref13), (what, 'other G')
        r6 = run_and_read(csr13)
        assert np.array_equal(r6, ref13), (what, 'other G, second readout')
        r7 = loop.readout(*csr)                             # and back
        assert np.array_equal(r7, ref), (what, 'first NodeGraph again')
        if form == 16: assert loop.set_persistent(True) is True
        loop.close()
    handles[0].close()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. stop control at the chunk and ballot boundaries
# ----------------------------------------------------------------------------------------------------------------------------------------
TARGETS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 128, 129)
MAX_IT = 140


def _ratios(s_new, s_old):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gate_study
    finally:
        sys.path.pop(0)
    return gate_study.ratios(s_new, s_old)


class StopCase:
    """333 nodes, state width 8, net_state 24 -> 16 -> 8 with tanh at gain 1.2: the state map contracts by about 9 % per body.  r[b] is the
    largest distance / norm ratio that the gate behind body b sees on the exact chain (r[0]: the first condition), from the C oracle's
    states; with a threshold between r[b] and min(r[:b]) the Loop stops at k = b.  n / hidden / gain: the same recipe for the other
    persistent forms (on 4,129 nodes and with a 64-wide hidden layer it is gain 1.1 that contracts by 10 - 13 % per body)."""

    def __init__(self, n=333, hidden=16, depth=MAX_IT, gain=1.2):
        rng = np.random.default_rng(4)
        arcs = random_arcs(rng, n, 3 * n, 2)
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        self.n, self.d = n, 8
        self.g = orc.make_graph_dict(arcs, nodes, 'average')
        self.st = make_mlp(rng, 2 + 2 * (8 + 3), [hidden, 8], 'tanh', gain=gain, bn_random=False)
        self.ou = make_mlp(rng, 8 + 3, [2], 'softmax')
        self.s0 = (0.1 * rng.standard_normal((n, 8))).astype(np.float32)
        # the chain body by body: one body from the state before it is the same arithmetic as b bodies from s0 (checked at the far end)
        self.states = [np.ones_like(self.s0), self.s0]
        for b in range(1, depth + 1):
            self.states.append(_loop_node(self.g, self.st, self.ou, 8, 1, 0.0, self.states[-1], want_out=False)[1])
        assert np.array_equal(self.states[-1], _loop_node(self.g, self.st, self.ou, 8, depth, 0.0, self.s0, want_out=False)[1])
        self.r = [float(np.max(_ratios(self.states[b + 1], self.states[b]))) for b in range(depth + 1)]
        self._want = {}

    def threshold(self, b):
        """stop at b: the geometric mean of r[b] and the smallest ratio before it, which r[b] undercuts by at least 4 %"""
        lo = min(self.r[:b])
        assert self.r[b] <= 0.96 * lo, (b, self.r[b], lo)
        return float(np.float32(np.sqrt(self.r[b] * lo)))

    def want(self, thr, max_it=MAX_IT, start=0):
        """(k, state, output) of the C oracle from the chain's state after `start` bodies"""
        key = (thr, max_it, start)
        if key not in self._want: self._want[key] = _loop_node(self.g, self.st, self.ou, 8, max_it, thr, self.states[start + 1])
        return self._want[key]

    def want64(self, bodies):
        """float64 oracle after exactly `bodies` bodies (threshold 0: its values at the C oracle's k, whatever its own gate would say)"""
        key = ('f64', bodies)
        if key not in self._want: self._want[key] = orc.loop_node(self.g, self.st, self.ou, 8, bodies, 0.0, self.s0, np.float64)
        return self._want[key]

    def stop_at(self, b, max_it=MAX_IT):
        """(threshold, oracle result) of "stop at b"; the oracle DOES stop there - asserted before anything goes to the GPU"""
        thr = self.threshold(b)
        want = self.want(thr, max_it)
        assert want[0] == b, (b, thr, want[0], self.r[b - 1:b + 2])
        return thr, want

    def handles(self, e):
        return _device(e, self.g, self.st, self.ou)


@functools.lru_cache(maxsize=None)
def _stop_case(n=333, hidden=16, depth=MAX_IT, gain=1.2):
    return StopCase(n, hidden, depth, gain)


def test_stop_case_is_what_it_is_built_for():
    """(no device work) every target body is a stop of the C oracle at its threshold, the ratios fall as recorded, and the persistent form is
    the one on 16-node tiles"""
    c = _stop_case()
    assert 0.2 < c.r[15] < 0.3 and 1e-3 < c.r[65] < 2e-3 and 1e-6 < c.r[130] < 1e-5, (c.r[15], c.r[65], c.r[130])
    for b in TARGETS:
        thr, want = c.stop_at(b)
        print(f'target {b}: r[b] {c.r[b]:.6e}, min before {min(c.r[:b]):.6e}, threshold {thr:.6e}, oracle k {want[0]:.0f}')
    f = _engine().small_form(_dims(c.st), c.st['activations'], c.n, 3)
    assert f['persistent'] and f['tile'] == 16 and not f['wide']


@pytest.mark.parametrize('b', TARGETS)
@pytest.mark.parametrize('impl', [0, 1])
def test_stop_per_body_exact(impl, b):
    """one launch per body: stops on both sides of the host's gate reads (16, 32, 64, 128) and of the 64-gate ballot of k_finalize"""
    e, c = _engine(), _stop_case()
    thr, want = c.stop_at(b)
    handles = c.handles(e)
    loop = _new_loop(e, handles, c.d, c.s0, 'bodies', impl, MAX_IT, thr)
    _exact_twice(loop, want, f'impl {impl}, stop at {b}')
    loop.close()
    handles[0].close()


@pytest.mark.parametrize('max_it,b', [(16, None), (17, None), (32, None), (64, None), (65, None), (129, None), (17, 16), (65, 64)])
@pytest.mark.parametrize('impl', [0, 1])
def test_stop_per_body_at_max_iteration(impl, max_it, b):
    """threshold 0: k = max_iteration, at a chunk multiple (no gate is read for the last chunk), one past it, and past the first ballot;
    and a stop at the body in front of max_iteration (b = 16 of 17, b = 64 of 65)"""
    e, c = _engine(), _stop_case()
    if b is None:
        thr, want = 0.0, c.want(0.0, max_it)
        assert want[0] == max_it
    else:
        thr, want = c.stop_at(b, max_it)
    handles = c.handles(e)
    loop = _new_loop(e, handles, c.d, c.s0, 'bodies', impl, max_it, thr)
    _exact_twice(loop, want, f'impl {impl}, max_iteration {max_it}, stop at {b}')
    loop.close()
    handles[0].close()


@pytest.mark.parametrize('b', TARGETS)
def test_stop_per_body_default_path(b):
    """impl 2, one launch per body: the oracle's k and values within the bounds of part 1.  Up to body 66 the thresholds sit 4 % from every
    ratio, far outside the gate's band (1e-3 relative + 1e-5): no gate is borderline and the Loop is not repeated.  At bodies 128 and 129
    the ratios are below 1e-5, where the absolute part of the band makes every node borderline: a repeat on impl 1 is the designed outcome
    there, so only k and the values are asserted."""
    e, c = _engine(), _stop_case()
    thr, want = c.stop_at(b)
    handles = c.handles(e)
    loop = _new_loop(e, handles, c.d, c.s0, 'bodies', 2, MAX_IT, thr)
    _close_twice(loop, want, c.want64(b), f'impl 2, stop at {b}')
    repeated, total = loop.gate_info()
    print(f'stop at {b}: repeated {repeated}, {total} repeats on this handle')
    if b <= 66: assert not repeated and total == 0, (b, repeated, total)
    loop.close()
    handles[0].close()


@pytest.mark.parametrize('BORDER', [40, 70])
def test_borderline_gate_in_every_part_of_the_scan(BORDER):
    """The threshold ON the largest ratio of one body's gate (computed in the kernel's order: ascending feature, unfused): that gate has no
    robust mover and a borderline node.  k_finalize scans the certified-gate words with 64 lanes, 64 gates per pass: gate 70 is lane 5 of the
    second pass, gate 40 a lane of the upper half of the first.  The impl-2 run must notice, repeat on impl 1 and return the oracle's k and
    bits; the handle keeps working; with max_iteration = that body its gate is never consulted, so nothing is repeated."""
    e, c = _engine(), _stop_case()
    s_old, s_new = c.states[BORDER], c.states[BORDER + 1]
    dist = np.zeros(c.n, np.float32); nrm = np.zeros(c.n, np.float32)
    for f in range(c.d):
        df = s_new[:, f] - s_old[:, f]
        dist = dist + df * df
        nrm = nrm + s_old[:, f] * s_old[:, f]
    ratio = np.sqrt(dist) / np.sqrt(nrm)
    thr = float(np.max(ratio))
    assert abs(thr - c.r[BORDER]) < 1e-5 * c.r[BORDER]
    # no robust mover at this gate (nothing above the threshold, let alone the band 1e-5 + 1e-3 thr), robust movers at every gate before it
    assert np.all(ratio <= thr) and all(c.r[b] > 1.04 * thr + 1e-5 for b in range(BORDER))
    want = c.want(thr)
    assert want[0] in (BORDER, BORDER + 1), want[0]          # on the threshold: the oracle's own rounding decides; either way this gate is consulted
    handles = c.handles(e)
    loop = _new_loop(e, handles, c.d, c.s0, 'bodies', 2, MAX_IT, thr)
    k = loop.run()
    repeated, total = loop.gate_info()
    print(f'threshold r[{BORDER}] = {thr:.9e}: oracle k {want[0]:.0f}, k {k:.0f}, repeated {repeated}, total {total}')
    assert repeated and total == 1, (repeated, total)
    assert k == want[0] and np.array_equal(loop.state(), want[1]) and np.array_equal(loop.output(), want[2])
    k = loop.run()                                           # the next run on the same handle
    assert k == want[0] and np.array_equal(loop.state(), want[1]) and np.array_equal(loop.output(), want[2])
    assert loop.gate_info() == (True, 2)
    loop.close()
    want70 = c.want(thr, BORDER)
    assert want70[0] == BORDER
    loop = _new_loop(e, handles, c.d, c.s0, 'bodies', 2, BORDER, thr)
    _close_twice(loop, want70, c.want64(BORDER), f'max_iteration {BORDER}, threshold r[{BORDER}]')
    assert loop.gate_info() == (False, 0)
    loop.close()
    handles[0].close()


@pytest.mark.parametrize('max_it,b', [(MAX_IT, 16), (MAX_IT, 17), (MAX_IT, 64), (MAX_IT, 65), (MAX_IT, 129), (65, None), (129, None)])
def test_stop_persistent_small16(max_it, b):
    """the persistent launch on 16-node tiles: one gate word per body, stops up to body 129 and max_iteration 65 and 129 at threshold 0"""
    e, c = _engine(), _stop_case()
    thr, want = c.stop_at(b) if b is not None else (0.0, c.want(0.0, max_it))
    if b is None: assert want[0] == max_it
    handles = c.handles(e)
    for impl in (1, 2):
        loop = _new_loop(e, handles, c.d, c.s0, 16, impl, max_it, thr)
        _exact_twice(loop, want, f'persistent, impl {impl}, max_iteration {max_it}, stop at {b}')
        assert loop.set_persistent(True) is True
        loop.close()
    handles[0].close()


# (the same recipe on the other two persistent forms; the stop bodies were picked on the CPU as the first body past 64 that undercuts
# every ratio before it by 4 % - stop_at asserts both again)
@pytest.mark.parametrize('form,n,hidden,gain,b', [(32, 4129, 16, 1.1, 66), ('16w', 333, 64, 1.1, 66)], ids=['small32', 'small16w'])
def test_stop_persistent_other_forms(form, n, hidden, gain, b):
    e, c = _engine(), _stop_case(n, hidden, 80, gain)
    _assert_form(e, c.st, n, 3, form)
    thr, want = c.stop_at(b, 80)
    handles = c.handles(e)
    for impl in (1, 2):
        loop = _new_loop(e, handles, c.d, c.s0, form, impl, 80, thr)
        _exact_twice(loop, want, f'persistent {form}, impl {impl}, stop at {b}')
        assert loop.set_persistent(True) is True
        loop.close()
    handles[0].close()


@pytest.mark.parametrize('b', [16, 17, 33])
@pytest.mark.parametrize('world,halo', [(2, False), (3, True)], ids=['world2_whole_shards', 'world3_boundary_blocks'])
def test_stop_loopback_groups(world, halo, b):
    """loopback groups read every rank's copy of the gate at the chunk boundary and must agree: stops at 16, 17 and 33 on impl 1, owned
    rows bit-equal to the unsharded oracle"""
    from test_gpu_sharded import _collect, _sharded_loops
    e, c = _engine(), _stop_case()
    thr, want = c.stop_at(b)
    comms, graphs, loops, ranges = _sharded_loops(e, c.g, c.st, c.ou, c.d, MAX_IT, thr, c.s0, world, 1, halo=halo)
    for rep in range(2):
        k = e.Loop.run_group(loops)
        state, out = _collect(loops, ranges, None)
        assert k == want[0], (world, b, rep, k)
        assert np.array_equal(state, want[1]) and out.shape == want[2].shape and np.array_equal(out, want[2]), (world, b, rep)
    for lp in loops: lp.close()
    for gr in graphs: gr.close()
    for cm in comms: cm.close()


def test_one_handle_long_short_long():
    """ONE Loop (max_iteration 140, the threshold of "stop at 129") run from two states of the chain: from s0 it stops at 129, from the
    state after 113 bodies at 16.  Persistent: long, short, long (the run-parity halves of the gate
    words: each run zeroes the other half for the next); then one launch per body: the same three; then persistent again (the host must
    clear both halves after the per-body runs used the block).  All seven are the oracle's bits."""
    e, c = _engine(), _stop_case()
    thr = c.threshold(129)
    starts = {'long': (0, 129), 'short': (113, 16)}
    wants = {}
    for name, (start, k_want) in starts.items():
        wants[name] = c.want(thr, MAX_IT, start)
        assert wants[name][0] == k_want, (name, wants[name][0])
    handles = c.handles(e)
    loop = e.Loop(handles[0], handles[1], handles[2], c.d, MAX_IT, thr)
    assert loop.set_impl(1) == 1

    def three(stage):
        for name in ('long', 'short', 'long'):
            loop.set_state0(c.states[starts[name][0] + 1])
            k, (kc, sc, oc) = loop.run(), wants[name]
            assert k == kc, (stage, name, k, kc)
            assert np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), (stage, name)

    assert loop.set_persistent(True) is True
    three('persistent')
    assert loop.set_persistent(True) is True
    assert loop.set_persistent(False) is False
    three('one launch per body')
    assert loop.set_persistent(True) is True
    loop.set_state0(c.states[1])
    k, (kc, sc, oc) = loop.run(), wants['long']
    assert k == kc and np.array_equal(loop.state(), sc) and np.array_equal(loop.output(), oc), 'persistent again'
    assert loop.set_persistent(True) is True
    loop.close()
    handles[0].close()


def test_run_many_loops_of_different_depth():
    """three persistent loops on shared Graph and Mlp handles that stop at 129, 17 and 65, in one gnn_loop_run_many call, twice: what each
    returns alone"""
    e, c = _engine(), _stop_case()
    handles = c.handles(e)
    loops, wants = [], []
    for b in (129, 17, 65):
        thr, want = c.stop_at(b)
        loops.append(_new_loop(e, handles, c.d, c.s0, 16, 1, MAX_IT, thr))
        wants.append(want)
    for rep in range(2):
        ks = e.Loop.run_many(loops)
        for lp, k, (kc, sc, oc) in zip(loops, ks, wants):
            assert k == kc, (rep, k, kc)
            assert np.array_equal(lp.state(), sc) and np.array_equal(lp.output(), oc), (rep, kc)
    assert all(lp.set_persistent(True) for lp in loops)      # no launch gave up
    for lp, want in zip(loops, wants):
        _exact_twice(lp, want, f'alone, stop at {want[0]:.0f}')
    for lp in loops: lp.close()
    handles[0].close()
