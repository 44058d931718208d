"""Every kernel form of the training step's matrix-core half (gnn_train_wide.hip: k_fwd3_split, k_bwd3_split, k_gemm_split, k_wgrad_bf,
k_wgrad_f32) against the float64 oracle, on the nets of tests/train_form_cases.py: each case first asserts through gnn_loop_train_forms that the
intended kernels ran (tests/test_train_forms_host.py derives the same table on the CPU), then compares one training-mode body - forward state,
outputs, d loss / d node labels and every gradient array - element by element, and repeats the step for identical bits.

Sizes: 4,113 rows (128 full 32-row tiles + 17 rows, just past the 4,096-row threshold), 4,095 | 4,096, and one sweep of the persistent kernels
+ 8 x 32 x 3 + 17 rows (66,321), where 25 waves take a second tile, the last of them a partial one.

Tolerance: no fixed number.  The oracle is evaluated a second time in float32; the bound of an array is MARGIN x max |oracle_f32 - oracle_f64|
over that array, applied to every element.  MARGIN = 8: a split product adds at most one rounding-sized term per product (3 x 2^-24), the chains
over K <= 144 and over the row chunks are sequential where NumPy sums in blocks, exp is 1.6e-7 relative.
Measured on an MI355X (profiles/r11_train_forms.txt, 489 arrays): the largest ratio of device error to reference noise is 2.76
(sweep_dropout dense grads_state[2]); the margin was set before that measurement and has not moved.

Row isolation: with d_out_nodes = 0 and d_state_extra non-zero on a few sentinel rows only (row 0, the tile edge 31 | 32, the 17 rows of the
partial tile, the rows of the second sweep), every gradient comes from those rows alone - a wrong, lost or doubled row shows at order 1, not 1 / n -
and d_nodes must be exactly zero on every row that is neither a sentinel nor the source of an arc into one.

Kinked activations (relu, selu): rows with a pre-activation within 1e-5 of 0 in the float64 forward get no incoming gradient, so they contribute
exactly nothing to either side; at most 5 % of the rows, and at most a tenth of any sentinel set, may be silenced that way.  Forward states are
compared on all rows.

GNN_TRAIN_FORMS_RATIOS=<file>: every (case, array) error, reference noise and their ratio is appended there (profiles/r11_train_forms.txt)."""
import os

import numpy as np
import pytest

import train_form_cases as T
from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

MARGIN = 8.0
KINK = 1e-5
KINKED = ('relu', 'selu')
SENTINEL_CASES = ['chain_linear', 'chain_sigmoid', 'chain_elu_narrow', 'chain_relu_k144', 'chain_selu']
SWEEP_CASES = ['sweep_chain', 'sweep_dropout', 'sweep_five_tiles']
SMALL_SETS = ['row0', 'tile_edge', 'last17']
RUNS = []                   # (case, incoming gradient), case by case: the oracle's forward of a case is built once and shared by its runs
for _c in T.C1 + T.C4:
    RUNS += [(_c.name, 'dense')] + ([(_c.name, s) for s in SMALL_SETS] if _c.name in SENTINEL_CASES else [])
for _name in SWEEP_CASES:
    RUNS += [(_name, s) for s in ['dense'] + SMALL_SETS + ['second_sweep']]

OBSERVED = {}               # case name -> kernel instantiations gnn_loop_train_forms reported
_BUILT = {}                 # case name -> inputs and the oracle's forward (the sweep cases: one at a time, they are large)


def _engine():
    from GNN import _engine
    return _engine


def get_case(name):
    small = {c.name: c for c in T.C1 + T.C4}
    if name in small: return small[name]
    sweep = _engine().train_forms((135, 64), ['tanh'], None, T.MIN_ROWS)['sweep_rows']
    return {c.name: c for c in T.c2(sweep)}[name]


def built(name):
    """Graph, nets, initial state, Dropout mask and the oracle's training-mode forward in float64 and float32: built once per case, shared by
    its runs, never modified."""
    if name not in _BUILT:
        if name in SWEEP_CASES:
            for other in SWEEP_CASES: _BUILT.pop(other, None)
        c = get_case(name)
        rng = np.random.default_rng(1000 * c.seed + sum(map(ord, c.name)))
        n, ds = c.n, c.dims[-1]
        arcs = random_arcs(rng, n, n, c.al)                               # about two arcs per node
        nodes = (2 * rng.random((n, c.nl)) - 1).astype(np.float32)
        g = orc.make_graph_dict(arcs, nodes, 'average')
        g['set_mask'] = np.ones(n, bool)
        st = make_mlp(rng, c.dims[0], list(c.dims[1:]), c.act, gain=0.7, bn_random=True, batch_normalization=c.bn)
        ou = make_mlp(rng, ds + c.nl, [2], 'softmax', batch_normalization=False)
        st['dropout'], ou['dropout'] = ({1: c.drop1} if c.drop1 else {}), {}
        masks = [{1: rng.random((n, c.dims[1])) > c.drop1}] if c.drop1 else [{}]
        s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
        ctx = {dt: tro.train_forward(g, st, ou, ds, 1, 0.0, s0, masks, {}, dtype=dt) for dt in (np.float64, np.float32)}
        assert ctx[np.float64]['k'] == ctx[np.float32]['k'] == 1
        silent = np.zeros(n, bool)
        if c.act in KINKED:
            for z in ctx[np.float64]['caches'][0]['z']: silent |= (np.abs(z) < KINK).any(axis=1)
        _BUILT[name] = dict(case=c, g=g, st=st, ou=ou, masks=masks, s0=s0, ctx=ctx, silent=silent)
    return _BUILT[name]


def sentinel_rows(b, sset):
    c = b['case']
    sweep = _engine().train_forms((135, 64), ['tanh'], None, T.MIN_ROWS)['sweep_rows']
    rows = {'row0': np.arange(1), 'tile_edge': np.arange(31, 33), 'last17': np.arange(c.n - 17, c.n), 'second_sweep': np.arange(min(sweep, c.n), c.n)}[sset]
    assert rows.size
    return rows


def incoming(b, sset):
    """(d_out_nodes, d_state_extra, sentinel rows or None) of a run; rows next to a kink get no gradient."""
    c = b['case']
    n, ds = c.n, c.dims[-1]
    rng = np.random.default_rng(sum(map(ord, sset)))
    if sset == 'dense':
        d_out, dse, rows = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, ds)).astype(np.float32), None
        assert b['silent'].mean() <= 0.05
    else:
        rows = sentinel_rows(b, sset)
        d_out, dse = np.zeros((n, 2), np.float32), np.zeros((n, ds), np.float32)
        dse[rows] = rng.standard_normal((rows.size, ds)).astype(np.float32)
        assert (~b['silent'][rows]).sum() >= 0.9 * rows.size, 'too many sentinel rows next to a kink: pick another seed'
    d_out[b['silent']] = 0.0
    dse[b['silent']] = 0.0
    return d_out, dse, rows


def run_device(b, d_out, dse):
    """train_forward + train_backward on the device, twice on one loop: (forms of both nets, [results of run 1, of run 2])."""
    from test_gpu_train import _by_source_csr
    e = _engine()
    c, g, st, ou = b['case'], b['g'], b['st'], b['ou']
    n, ds = c.n, c.dims[-1]
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], g['nodes'], g['set_mask'])
    mst, mou = e.Mlp(st['weights'], st['activations'], c.bn), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, ds, 1, 0.0)
    loop.set_state0(b['s0'])
    ms = b['masks'][0][1].astype(np.uint8).ravel() if c.drop1 else None
    runs = []
    for _ in range(2):
        k, out = loop.train_forward(mst, mou, _by_source_csr(g, n), dropout_state=T.rates(c), dropout_output=[0, 0], masks_state=ms,
                                    bn_state=np.concatenate(st['weights'][-4:-2]) if c.bn else None)
        forms = loop.train_forms(0), loop.train_forms(1)
        state = loop.state()
        res = loop.train_backward(d_out, dse, want_d_nodes=True)
        runs.append(dict(k=k, out=out, state=state, d_nodes=res['d_nodes'], grads_state=res['grads_state'], grads_output=res['grads_output']))
    loop.close(); graph.close()
    return forms, runs


def arrays(r):
    """name -> array of one result (device run or oracle), in a fixed order"""
    out = {'state': r['state'], 'out_nodes': r['out'], 'd_nodes': r['d_nodes']}
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def oracle(b, d_out, dse, dt):
    ctx = b['ctx'][dt]
    gs, go, dn = tro.train_backward(ctx, d_out.astype(dt), dse.astype(dt))
    return dict(state=ctx['state'], out=ctx['out_nodes'], d_nodes=dn, grads_state=gs, grads_output=go)


def record(lines):
    path = os.environ.get('GNN_TRAIN_FORMS_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))


@pytest.mark.parametrize('name,sset', RUNS)
def test_form_against_oracle(name, sset):
    b = built(name)
    c = b['case']
    d_out, dse, rows = incoming(b, sset)
    (f_state, f_out), runs = run_device(b, d_out, dse)
    # 1. the intended kernels ran
    assert T.letters(f_state) == (c.fwd, c.bwd, c.wg) and f_state['build_input'] == (c.n < T.MIN_ROWS), (T.letters(f_state), f_state)
    assert T.letters(f_out) == ('P', 'P', 'P')
    OBSERVED[name] = T.kernels(c.dims, c.act, f_state)
    # 2. every array, element by element, within MARGIN x the float32 noise of the reference itself
    got, want, noisy = arrays(runs[0]), arrays(oracle(b, d_out, dse, np.float64)), arrays(oracle(b, d_out, dse, np.float32))
    assert runs[0]['k'] == 1.0 and list(got) == list(want)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(want[key], np.float64)
        assert a.shape == w.shape, key
        noise = float(np.max(np.abs(np.asarray(noisy[key], np.float64) - w)))
        err = float(np.max(np.abs(a.astype(np.float64) - w)))
        ratio = err / noise if noise > 0 else (0.0 if err == 0 else float('inf'))
        lines.append(f'{name:22s} {sset:13s} {key:16s} err {err:9.3e}  noise {noise:9.3e}  ratio {ratio:6.2f}  max|ref| {float(np.max(np.abs(w))):9.3e}')
        if not np.all(np.abs(a.astype(np.float64) - w) <= MARGIN * noise): bad.append(lines[-1])
    record(lines)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)
    # 3. row isolation: the gradients are not vacuous, and nothing reaches a row that is neither a sentinel nor the source of an arc into one
    if rows is not None:
        live = rows[~b['silent'][rows]]
        assert np.abs(want['grads_state[0]']).max() > 0 and (np.abs(want['d_nodes'][live]).max(axis=1) > 0).all()
        indptr, src = b['g']['adjT'][0], b['g']['adjT'][1]
        reach = np.zeros(c.n, bool)
        reach[rows] = True
        for r in rows: reach[src[indptr[r]:indptr[r + 1]]] = True
        assert not got['d_nodes'][~reach].any() and not want['d_nodes'][~reach].any()
    # 4. a repeated step returns identical bits
    again = arrays(runs[1])
    for key, a in got.items():
        assert np.array_equal(a.view(np.uint32), again[key].view(np.uint32)), key


def test_kink_silencing_leaves_the_cases_intact():
    """The conditions under which the kinked cases silence rows (module docstring), stated once more on their own."""
    for name in ('chain_relu_k144', 'chain_selu'):
        b = built(name)
        assert 0 < b['silent'].sum() <= 0.05 * b['case'].n
        for sset in SMALL_SETS:
            rows = sentinel_rows(b, sset)
            assert (~b['silent'][rows]).sum() >= 0.9 * rows.size, (name, sset)
    assert not built('chain_elu_narrow')['silent'].any()           # elu' is continuous: nothing to silence


def test_the_table_launches_every_reachable_instantiation():
    """The union of what gnn_loop_train_forms reported over the table = train_form_cases.REACHABLE, the list tests/test_train_forms_host.py
    derives by enumeration.  (A case whose run was deselected is observed here with a forward pass alone.)"""
    e = _engine()
    for name in [c.name for c in T.C1 + T.C4] + SWEEP_CASES:
        if name in OBSERVED: continue
        c = get_case(name)
        rng = np.random.default_rng(5)
        n, ds = c.n, c.dims[-1]
        arcs = random_arcs(rng, n, n, c.al)
        nodes = (2 * rng.random((n, c.nl)) - 1).astype(np.float32)
        g = orc.make_graph_dict(arcs, nodes, 'average')
        st = make_mlp(rng, c.dims[0], list(c.dims[1:]), c.act, gain=0.7, bn_random=True, batch_normalization=c.bn)
        ou = make_mlp(rng, ds + c.nl, [2], 'softmax', batch_normalization=False)
        graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, np.ones(n, bool))
        mst, mou = e.Mlp(st['weights'], st['activations'], c.bn), e.Mlp(ou['weights'], ou['activations'], False)
        loop = e.Loop(graph, mst, mou, ds, 1, 0.0)
        loop.set_state0((0.1 * rng.standard_normal((n, ds))).astype(np.float32))
        loop.train_forward(mst, mou, None, dropout_state=T.rates(c), dropout_output=[0, 0], seed=3)
        OBSERVED[name] = T.kernels(c.dims, c.act, loop.train_forms(0))
        loop.close(); graph.close()
    seen = set().union(*OBSERVED.values())
    assert seen == T.REACHABLE, (sorted(seen - T.REACHABLE), sorted(T.REACHABLE - seen))
