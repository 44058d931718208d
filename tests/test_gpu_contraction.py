"""The contraction estimate (include/gnn_hip.h: gnn_loop_contraction_estimate; Loop.contraction_estimate) on the device.

1. Exact structure: a directed path, a linear layer without own-state weights - (J^T)^5 = 0 structurally, no tolerance.
2. Closed form: a 16-cycle with 'sum' aggregation, W_own = 0.2 I, W_agg = 0.3 I, v0 = ones (an eigenvector): every growth entry is 0.8 to 1e-5
   relative (64 terms of 2^-24 and a handful of roundings per element: below 4e-6).
3. The gather's forms at their edges against the mirror (tests/contraction_mirror.py) with an injected v0 and 6 iterations, growth and the last
   vector per element under the criterion of tests/test_gpu_adjoint.py (restated: MARGIN x the float32 noise of the mirror itself + FLOOR x the
   array's largest entry, constants unchanged).  The mirror starts from the DEVICE's p: no gate decision enters.  GNN_CONTRACTION_RATIOS=<file>
   appends the measured ratios (profiles/contraction_estimate.txt).  The aligned flavour of the row form reads the rows the three-layer chain
   leaves, and that chain exists at Ds 64 alone (its last layer is a wide product): Ds 4 and 8 run the two-column-block flavour.
4. Behaviour: same bits twice, the seed form, the loop stays usable, the refusals."""
import os

import numpy as np
import pytest

import adjoint_bn_cases as C
import contraction_mirror as cm
import test_gpu_adjoint as ga
from oracle import gnn_oracle as orc
from util import make_mlp

pytestmark = pytest.mark.gpu

MARGIN = ga.MARGIN
FLOOR = ga.FLOOR


class Device:
    """The loop of a problem on the device (bit-exact float32 forward, as the adjoint tests); mode None: the gradient mode is never set."""

    def __init__(self, pb, max_iter=30, thr=1e-2, mode=None, frozen=None):
        from GNN import _engine as e
        g, n = pb['g'], pb['n']
        mask = g['set_mask'] & g['output_mask']
        self.graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], g['nodes'], mask)
        self.mst = e.Mlp(pb['st']['weights'], pb['st']['activations'], pb['st']['batch_normalization'])
        self.mou = e.Mlp(pb['ou']['weights'], pb['ou']['activations'], pb['ou']['batch_normalization'])
        self.loop = e.Loop(self.graph, self.mst, self.mou, pb['D'], max_iter, thr)
        if pb['D']: self.loop.set_state0(pb['s0'])
        self.loop.set_impl(1)
        if mode is not None: self.loop.set_gradient_mode(mode, batch_normalization=frozen)
        self.pb = pb

    def estimate(self, **kw):
        return self.loop.contraction_estimate(self.mst, **kw)

    def step(self):
        pb = self.pb
        return self.loop.train_step(self.mst, self.mou, None, pb['targets'], pb['weights'], 0)

    def close(self):
        self.loop.close(); self.graph.close()


def linear_problem(arcs, n, ds, w_own, w_agg, aggregation, nl=2, al=1, seed=0):
    """One linear Dense layer with the given own-state and aggregated-state blocks [ds, ds]; the label rows are random (they do not enter J)."""
    rng = np.random.default_rng(seed)
    arcs = np.concatenate([np.asarray(arcs, np.float32), (2 * rng.random((len(arcs), al)) - 1).astype(np.float32)], axis=1)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, aggregation)
    w = (0.3 * rng.standard_normal((al + 2 * (ds + nl), ds))).astype(np.float32)
    w[:ds] = w_own
    w[ds + nl:2 * ds + nl] = w_agg
    st = dict(weights=[w, (0.1 * rng.standard_normal(ds)).astype(np.float32)], activations=['linear'], batch_normalization=False)
    ou = make_mlp(rng, ds + nl, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    return dict(g=g, st=st, ou=ou, ds=ds, D=ds, s0=(0.1 * rng.standard_normal((n, ds))).astype(np.float32), n=n,
                targets=np.eye(2)[rng.integers(0, 2, m)].astype(np.float32), weights=np.ones(m, np.float32))


# ---- 1. exact structure ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ds', [3, 4])
def test_nilpotent_path_stops_exactly(ds):
    rng = np.random.default_rng(1)
    pb = linear_problem([(i, i + 1) for i in range(4)], 5, ds, 0.0, (0.5 * rng.standard_normal((ds, ds))).astype(np.float32), 'average')
    dev = Device(pb, max_iter=8, thr=1e-3)
    v0 = rng.standard_normal((5, ds)).astype(np.float32)
    res = dev.estimate(iterations=8, v0=v0)
    assert res['done'] == 5 and res['growth'].shape == (5,) and res['growth'][4] == 0.0 and np.all(res['growth'][:4] > 0), res
    assert res['rho'] == 0.0 and res['contractive'] is True and res['last'] == 0.0
    assert not dev.loop.contraction_vector().any()
    # the raw C result: the entries behind `done` are 0.0
    import ctypes as ct
    from GNN import _engine as e
    growth, done, k = np.full(8, -1.0, np.float32), ct.c_int(-1), ct.c_float(-1.0)
    e._check(e.lib().gnn_loop_contraction_estimate(dev.loop._h, None, None, None, e._fp(np.zeros(2, np.float32)), None, ct.c_int(8), e._fp(v0), ct.c_uint64(0),
                                                   e._fp(growth), ct.byref(done), ct.byref(k)))
    assert done.value == 5 and np.array_equal(growth[:5], res['growth']) and np.all(growth[4:] == 0.0) and k.value == res['k']
    dev.close()


# ---- 2. closed form -------------------------------------------------------------------------------------------------------------------------------
def test_cycle_eigenvector_closed_form():
    n, ds = 16, 4
    arcs = [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]
    pb = linear_problem(arcs, n, ds, 0.2 * np.eye(ds, dtype=np.float32), 0.3 * np.eye(ds, dtype=np.float32), 'sum')
    dev = Device(pb, max_iter=5, thr=1e-3)
    res = dev.estimate(iterations=12, v0=np.ones((n, ds), np.float32))
    print(res['growth'])
    assert res['done'] == 12
    assert np.max(np.abs(res['growth'].astype(np.float64) - 0.8)) <= 1e-5 * 0.8, res['growth']
    assert abs(res['rho'] - 0.8) <= 1e-5 * 0.8 and res['contractive'] is True
    dev.close()


# ---- 3. the forms at their edges ---------------------------------------------------------------------------------------------------------------------
def record(lines):
    path = os.environ.get('GNN_CONTRACTION_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))


def check_against_mirror(tag, dev, iterations=6, seed=5):
    pb = dev.pb
    v0 = np.random.default_rng(seed).standard_normal((pb['n'], pb['ds'])).astype(np.float32)
    res = dev.estimate(iterations=iterations, v0=v0)
    got = {'growth': res['growth'], 'vector': dev.loop.contraction_vector()}
    p = dev.loop.state()                                   # the estimate leaves the inference Loop's state: the p it recorded the body at
    want, noisy = {}, {}
    for dtype, out in ((np.float64, want), (np.float32, noisy)):
        ctx = cm.context(pb['g'], pb['st'], pb['ou'], pb['D'], p, dtype)
        out['growth'], done, out['vector'] = cm.power(ctx, v0, iterations)
        assert done == iterations
    assert res['done'] == iterations and res['k'] >= 1 and np.all(want['growth'] > 0)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(want[key], np.float64)
        assert a.shape == w.shape, key
        noise = float(np.max(np.abs(np.asarray(noisy[key], np.float64) - w)))
        top = float(np.max(np.abs(w)))
        err = float(np.max(np.abs(a.astype(np.float64) - w)))
        lines.append(f'{tag:44s} {key:8s} err {err:9.3e}  noise {noise:9.3e}  ratio {err / noise if noise > 0 else float("nan"):6.2f}  floor {FLOOR * top:9.3e}  max|ref| {top:9.3e}'
                     f'{"  NEEDS THE FLOOR" if err > MARGIN * noise else ""}')
        if not np.all(np.abs(a.astype(np.float64) - w) <= MARGIN * noise + FLOOR * top): bad.append(lines[-1])
    record(lines)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)
    assert abs(res['rho'] - cm.rho(want['growth'], iterations)) <= 1e-5 * cm.rho(want['growth'], iterations)
    return res


# rows 1, 15 | 16 | 17 (the 16 rows of a block), 37 and 83; Ds 3 and 5 (any width) and 4, 8, 64 (16-byte pieces, from the two column blocks of d concat); 1 to 3
# layers, tanh and selu; the symmetric lists with the isolated node 1 and the 70-arc hub of tests/test_gpu_adjoint.py ('sym') and the directed, unsorted
# lists of tests/train_graph_cases.py ('dir': from 37 nodes on); one net that ends in BatchNormalization (variance and gamma far from 1)
SMALL = [('sym', dict(n=1, ds=3)), ('bn', dict(n=15, ds=4, hidden=(), act='selu', bn=False)), ('bn', dict(n=16, ds=8, hidden=(7,), bn=False)),
         ('bn', dict(n=17, ds=64, hidden=(20,), bn=False)), ('bn', dict(n=37, ds=5, hidden=(9, 6), act='selu', bn=False)),
         ('bn', dict(n=37, ds=8, hidden=(7,), bn=True)), ('bn', dict(n=37, ds=3, hidden=(7,), act='selu', bn=True)),
         ('sym', dict(n=83, ds=4, hub=70, isolated=True)), ('sym', dict(n=83, ds=5, hub=70, hidden=())), ('bn', dict(n=83, ds=3, hidden=(7,), act='selu', bn=False)),
         ('bn', dict(n=83, ds=64, hidden=(12, 9), bn=False))]


@pytest.mark.parametrize('kind,case', SMALL, ids=lambda v: v if isinstance(v, str) else '-'.join(f'{k}{x}' for k, x in v.items()).replace(' ', ''))
def test_small_cases_against_the_mirror(kind, case):
    pb = ga.problem(11, **case) if kind == 'sym' else C.problem(101, **case)
    if case['n'] >= 37 and kind == 'bn':                                  # directed: some arc has no reverse
        arcs = {(int(a), int(b)) for a, b in np.asarray(pb['g']['arcs'])[:, :2]}
        assert any((b, a) not in arcs for a, b in arcs)
    dev = Device(pb)
    check_against_mirror(f'small {kind} ' + ' '.join(f'{k}={v}' for k, v in case.items()), dev)
    dev.close()


# 4,113 rows: 258 blocks of partials (k_power_finalize: two per thread); the three-layer chain with its aligned rows (it exists at Ds 64 alone: its last
# layer is a wide product), without and behind a frozen BatchNormalization; the wide products per layer with the two-column-block gather on many rows, at
# Ds 64 and at Ds 40 (six idle lanes per row, a per-op last layer)
LARGE = [((135, 128, 128, 64), False, ['chain3'] * 3, 'rows_aligned'), ((135, 144, 64), False, ['wide'] * 2, 'rows'),
         ((135, 128, 128, 64), True, ['chain3'] * 3, 'rows_aligned'), ((87, 128, 128, 40), True, ['wide', 'wide', 'per_op'], 'rows')]


@pytest.mark.parametrize('dims,bn,backward,gather', LARGE, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_large_row_forms_against_the_mirror(dims, bn, backward, gather):
    from GNN import _engine as e
    n, ds = 4113, dims[-1]
    f = e.adjoint_form(dims, ['tanh'] * (len(dims) - 1), n, batch_normalization=bn, frozen_bn='frozen' if bn else None)
    assert f['backward'] == backward and f['gather'] == gather                     # what net_backward takes without weight gradients on these rows
    pb = C.problem(131, n=n, ds=ds, nl=3, al=1, hidden=dims[1:-1], gain=0.3, bn=bn)
    assert C.dims_of(pb) == list(dims)
    dev = Device(pb)
    check_against_mirror(f'large {"x".join(map(str, dims))} bn={bn}', dev)
    dev.close()


# ---- 4. behaviour ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_the_seed_form():
    pb = C.problem(141, n=300, ds=8, hidden=(12,), bn=True)
    dev = Device(pb)
    v0 = np.random.default_rng(2).standard_normal((300, 8)).astype(np.float32)
    a, wa = dev.estimate(iterations=9, v0=v0), dev.loop.contraction_vector()
    b, wb = dev.estimate(iterations=9, v0=v0), dev.loop.contraction_vector()
    assert a['done'] == 9 and np.array_equal(a['growth'], b['growth']) and np.array_equal(wa, wb) and a['k'] == b['k'] and a['rho'] == b['rho']
    s0, w0 = dev.estimate(iterations=9, seed=0), dev.loop.contraction_vector()
    s0b, w0b = dev.estimate(iterations=9, seed=0), dev.loop.contraction_vector()
    s1, w1 = dev.estimate(iterations=9, seed=1), dev.loop.contraction_vector()
    assert np.array_equal(s0['growth'], s0b['growth']) and np.array_equal(w0, w0b)
    assert not np.array_equal(s0['growth'], s1['growth']) and not np.array_equal(w0, w1) and not np.array_equal(s0['growth'], a['growth'])
    # the first iteration starts from the drawn vector: a different seed moves entry 0 already
    assert s0['growth'][0] != s1['growth'][0]
    one = dev.estimate(iterations=1, v0=v0)
    assert one['done'] == 1 and one['growth'][0] == a['growth'][0]
    dev.close()


def test_default_iterations_and_a_net_that_is_no_contraction():
    """32 iterations by default; the gain-3 net of the truncated adjoint tests is no contraction (the adjoint runs to its cap there): rho > 1."""
    pb = ga.problem(41, n=60, ds=4, gain=3.0)
    dev = Device(pb, max_iter=3, thr=1e-3)
    res = dev.estimate()
    assert res['done'] == 32 and res['growth'].shape == (32,) and res['k'] == 3.0
    ctx = cm.context(pb['g'], pb['st'], pb['ou'], pb['D'], dev.loop.state())
    radius = float(np.max(np.abs(np.linalg.eigvals(cm.dense_jt(ctx)))))
    print(res['rho'], radius)
    assert radius > 1 and res['rho'] > 1 and res['contractive'] is False
    dev.close()


@pytest.mark.parametrize('mode,frozen', [(None, None), (1, 'frozen'), (2, 'frozen'), (0, None)])
def test_estimate_leaves_the_loop_usable(mode, frozen):
    pb = C.problem(151, n=120, ds=8, hidden=(10,), bn=True if frozen else False)
    plain, mixed = Device(pb, mode=mode, frozen=frozen), Device(pb, mode=mode, frozen=frozen)
    k0, state0, out0 = plain.loop.run(), plain.loop.state(), plain.loop.output()
    k1 = mixed.loop.run()
    res = mixed.estimate(iterations=4, seed=3)
    assert res['k'] == k0 == k1 and np.array_equal(mixed.loop.state(), state0)
    assert mixed.loop.run() == k0 and np.array_equal(mixed.loop.state(), state0) and np.array_equal(mixed.loop.output(), out0)
    if mode is not None:
        assert mixed.loop._gradient_mode == mode
        want = plain.step()
        mixed.estimate(iterations=4, seed=3)
        got = mixed.step()
        assert got['loss'] == want['loss'] and got['k'] == want['k']
        for key in ('grads_state', 'grads_output'):
            for x, y in zip(got[key], want[key]): assert np.array_equal(x, y), key
        if mode: assert got['adjoint_iterations'] == want['adjoint_iterations'] and mixed.loop.adjoint_info() == plain.loop.adjoint_info()
        assert np.array_equal(mixed.loop.state(), plain.loop.state()) and np.array_equal(mixed.loop.output(), plain.loop.output())
    plain.close(); mixed.close()


def test_estimate_ends_a_pending_training_forward():
    from GNN import _engine as e
    pb = C.problem(153, n=50, ds=4, bn=False)
    dev = Device(pb)
    dev.loop.train_forward(dev.mst, dev.mou, None)
    dev.estimate(iterations=2)
    with pytest.raises(e.EngineError): dev.loop.train_backward(np.zeros((dev.loop.n_masked, 2), np.float32))
    dev.loop.train_forward(dev.mst, dev.mou, None)                 # a training forward ends the life of the estimate's vector
    with pytest.raises(e.EngineError): dev.loop.contraction_vector()
    dev.close()


def test_refusals():
    from GNN import _engine as e
    import test_gpu_sharded as sh
    pb = C.problem(155, n=40, ds=4, bn=False)
    dev = Device(pb)
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match='iterations'): dev.estimate(iterations=bad)
    with pytest.raises(ValueError): dev.estimate(v0=np.zeros((39, 4), np.float32))
    for pos in range(3):
        rates = [0.0, 0.0, 0.0]; rates[pos] = 0.2
        with pytest.raises(NotImplementedError, match='Dropout'): dev.estimate(dropout_state=rates)
    with pytest.raises(NotImplementedError, match='Dropout'): dev.estimate(dropout_state=[0.0, -0.1, 0.0])
    assert dev.estimate(iterations=2)['done'] == 2                 # a refused call leaves the loop as it was
    dev.close()
    labels = ga.problem(11, n=30, ds=2, nl=2, D=0)                 # state_vect_dim 0: the loop iterates on the node labels
    dev0 = Device(labels)
    with pytest.raises(NotImplementedError, match='state_vect_dim'): dev0.estimate()
    dev0.close()
    comms, graphs, loops, _ = sh._sharded_loops(e, pb['g'], pb['st'], pb['ou'], pb['D'], 5, 1e-2, pb['s0'], 2, 0, strict=False)
    mst = e.Mlp(pb['st']['weights'], pb['st']['activations'], False)
    for lp in loops:
        with pytest.raises(NotImplementedError, match='single-GPU'): lp.contraction_estimate(mst)
    for x in loops + graphs + comms: x.close()


def test_a_graph_without_rows_cannot_reach_the_estimate():
    """gnn_loop_contraction_estimate returns done = 0 and a zero growth for a loop without rows - but one GPU holds no such loop: a graph needs a node, and
    the rank of a group that owns no rows is refused as world > 1 (test_refusals).  What the surface can show: the graph itself is refused."""
    from GNN import _engine as e
    z = np.zeros(0, np.float32)
    with pytest.raises(ValueError):
        e.Graph(0, np.zeros(1, np.int32), np.zeros(0, np.int32), z, z, np.zeros((0, 1), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, bool))


def test_model_method_on_every_model_type():
    """GNNnodeBased.contraction_estimate and what inherits it, on a GraphObject; the model's gradient mode and weights stay."""
    import test_gpu_adjoint_bn as tb
    for kind in ('n', 'g', 'a'):
        t = tb._typed(kind)
        gnn, g = t['gnn'], t['batch']
        before = [np.array(w) for w in gnn.net_state.get_weights()]
        res = gnn.contraction_estimate(g, iterations=5, seed=1)
        again = gnn.contraction_estimate(g, iterations=5, seed=1)
        assert res['done'] == 5 and np.array_equal(res['growth'], again['growth']) and res['rho'] > 0 and isinstance(res['contractive'], bool)
        assert gnn.gradient_mode == 'fixed_point'
        for a, b in zip(before, gnn.net_state.get_weights()): assert np.array_equal(a, np.asarray(b))
        k, state, _ = gnn.Loop(g)
        assert k == res['k'] and state.shape == t['s0'].shape
        with pytest.raises(ValueError, match='iterations'): gnn.contraction_estimate(g, iterations=1025)
