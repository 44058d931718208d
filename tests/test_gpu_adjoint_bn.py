"""The fixed-point gradient for a net_state that ends in BatchNormalization on its moving statistics (gnn_loop_set_gradient_mode_ex with
GNN_ADJOINT_FROZEN_BN; set_gradient_mode(..., batch_normalization='frozen')) on the device, against its float64 mirror (tests/adjoint_bn_mirror.py).

Criterion, as in tests/test_gpu_adjoint.py: the mirror is evaluated a second time in float32; an array passes when every element lies within
MARGIN = 8 x max |mirror_f32 - mirror_f64| over that array, plus FLOOR = 2^-22 x max |mirror_f64| for arrays whose float32 evaluation happens to
be exact.  The arrays: state, outputs, z_final (gnn_loop_adjoint_z) and every gradient array, gamma and beta of net_state included; the loss
to 2e-5.  The mirror runs exactly the device's k bodies and the device's count of adjoint iterations, so no gate decision enters a comparison;
the counts themselves are compared in section 4.  GNN_ADJOINT_BN_RATIOS=<file> appends the measured ratios (profiles/fixed_point_frozen_bn.txt):
318 arrays; the largest ratio among the 310 that pass on 8 x noise alone is 5.99; 8 arrays (4 distinct ones of one to four elements - the b, beta and
gamma gradients of the one-column nets and the gamma gradient of the converging run - whose float32 reference happens to be nearly exact) need the
floor, at ratios 8.31, 8.43, 9.15 and 28.24.

Inputs (tests/adjoint_bn_cases.py): moving mean non-zero, moving variance in [0.25, 4], gamma 0.5 .. 1.5 in size with mixed signs, beta non-zero,
so that a missing or doubled column scale shows at order 1; directed, unsorted arc lists from 37 nodes on.  The loops run on impl 1 (bit-exact
float32 forward), as in tests/test_gpu_adjoint.py."""
import os

import numpy as np
import pytest

import adjoint_bn_cases as C
import adjoint_bn_mirror as bm
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -22
ADAM = (1, [0.01, 0.9, 0.999, 1e-7])


class Device:
    """The loop of a problem on the device, in a fixed-point mode with the frozen flag unless told otherwise."""

    def __init__(self, pb, max_iter, thr, state0=None, impl=1, mode=1, adjoint_max_iter=None, adjoint_threshold=None, frozen='frozen'):
        from GNN import _engine as e
        g, n = pb['g'], pb['n']
        mask = g['set_mask'] & g['output_mask']
        self.graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], g['nodes'], mask)
        self.mst = e.Mlp(pb['st']['weights'], pb['st']['activations'], pb['st']['batch_normalization'])
        self.mou = e.Mlp(pb['ou']['weights'], pb['ou']['activations'], pb['ou']['batch_normalization'])
        self.loop = e.Loop(self.graph, self.mst, self.mou, pb['D'], max_iter, thr)
        s0 = pb['s0'] if state0 is None else state0
        if pb['D']: self.loop.set_state0(s0)
        if impl is not None: self.loop.set_impl(impl)
        self.loop.set_gradient_mode(mode, adjoint_max_iter, adjoint_threshold, batch_normalization=frozen)
        self.pb = pb

    def step(self, **kw):
        pb = self.pb
        res = self.loop.train_step(self.mst, self.mou, None, pb['targets'], pb['weights'], 0, **kw)
        res['state'], res['out'] = self.loop.state(), self.loop.output()
        res['info'] = self.loop.adjoint_info()
        if self.loop._gradient_mode: res['z'] = self.loop.adjoint_z()
        return res

    def close(self):
        self.loop.close(); self.graph.close()


def arrays(r):
    out = {'state': r['state'], 'out': r['out'], 'z': r['z']}
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def mirrors(pb, max_iter, thr, k, iterations, own=True, **kw):
    """The mirror with the device's counts forced, in float64 and float32; and (own) with the device's k but its OWN adjoint gate, in float64."""
    args = (pb['g'], pb['st'], pb['ou'], pb['D'], max_iter, thr, pb['s0'], {}, pb['targets'], pb['weights'])
    want = bm.step(*args, k_forced=k, iterations_forced=iterations, **kw)
    noisy = bm.step(*args, k_forced=k, iterations_forced=iterations, dtype=np.float32, **kw)
    return want, noisy, (bm.step(*args, k_forced=k, **kw) if own else None)


def check_tight(tag, res, want, noisy):
    got, w64, w32 = arrays(res), arrays(want), arrays(noisy)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(w64[key], np.float64)
        assert a.shape == w.shape, key
        noise = float(np.max(np.abs(np.asarray(w32[key], np.float64) - w))) if w.size else 0.0
        top = float(np.max(np.abs(w))) if w.size else 0.0
        err = float(np.max(np.abs(a.astype(np.float64) - w))) if w.size else 0.0
        lines.append(f'{tag:40s} {key:16s} err {err:9.3e}  noise {noise:9.3e}  ratio {err / noise if noise > 0 else float("nan"):6.2f}  floor {FLOOR * top:9.3e}  max|ref| {top:9.3e}')
        if w.size and not np.all(np.abs(a.astype(np.float64) - w) <= MARGIN * noise + FLOOR * top): bad.append(lines[-1])
    path = os.environ.get('GNN_ADJOINT_BN_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))
    print('\n'.join(lines))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    assert not bad, '\n' + '\n'.join(bad)


def scale_shows(pb, want):
    """The case can tell a missing column scale: gamma and beta gradients of order > 1e-3 and a scale away from 1."""
    L = len(pb['st']['activations'])
    gamma, _, _, var = pb['st']['weights'][2 * L:2 * L + 4]
    s = gamma / np.sqrt(var + orc.BN_EPS)
    return np.abs(np.abs(s) - 1).max() > 0.2 and np.abs(want['grads_state'][2 * L]).max() > 1e-3 and np.abs(want['grads_state'][2 * L + 1]).max() > 1e-3


# ---- 1 / 2. the one-launch iteration and the per-kernel chain -------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', C.NARROW, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_small_nets_in_both_forms(case, mode):
    """Mode 1: k_adjoint_narrow with the column scale (the 64-wide state has a 133-wide concat: the chain, k_layer_bwd behind the frozen pass);
    mode 2: the per-kernel chain on every case.  Rows 15 | 16 | 17 and 37 with an isolated node, a hub and rows outside the mask."""
    from GNN import _engine as e
    pb = C.narrow_problem(case)
    dims, acts = C.dims_of(pb), pb['st']['activations']
    form = e.adjoint_form(dims, acts, pb['n'], batch_normalization=True, frozen_bn='frozen')
    narrow = case['ds'] != 64
    assert form['eligible'] and (form['gather'] == 'narrow') == narrow
    dev = Device(pb, 50, 1e-2, mode=mode)
    res, again = dev.step(), dev.step()
    chain = 'rows' if case['ds'] % 4 == 0 and case['ds'] <= 64 else 'generic'
    assert res['info']['gather'] == ('narrow' if mode == 1 and narrow else chain)
    want, noisy, own = mirrors(pb, 50, 1e-2, int(res['k']), res['adjoint_iterations'])
    assert res['k'] >= 2 and res['adjoint_converged'] and res['adjoint_iterations'] >= 3 and abs(res['adjoint_iterations'] - own['adjoint_iterations']) <= 1
    assert scale_shows(pb, want) and (np.abs(want['g']).max(axis=1) == 0).any()
    check_tight(f'small n{case["n"]} ds{case["ds"]} L{len(acts)} {acts[0]} mode {mode}', res, want, noisy)
    for key, a in arrays(res).items(): assert np.array_equal(a, arrays(again)[key]), key
    assert again['loss'] == res['loss'] and again['info'] == res['info']
    assert res['bn_batch_state'].shape[0] == 0               # no batch statistics of net_state
    dev.close()


# ---- 3. many rows -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims,n,backward,gather', C.LARGE, ids=lambda v: str(v).replace(' ', '') if isinstance(v, (tuple, int)) else None)
def test_large_row_forms(dims, n, backward, gather):
    """4,095 | 4,096 and 4,113 rows: the frozen pass in front of k_layer_bwd, of k_bwd3_split (the three-layer chain with its aligned rows) and of
    the wide per-layer products; the gamma and beta gradients are sums of several chunk partials."""
    from GNN import _engine as e
    pb = C.large_problem(dims, n)
    assert e.adjoint_form(dims, ['tanh'] * (len(dims) - 1), n, batch_normalization=True, frozen_bn='frozen') == \
        dict(eligible=True, reason=None, gather=gather, backward=backward, narrow_refusal='width')
    dev = Device(pb, 30, 1e-2)
    res = dev.step()
    assert res['info']['gather'] == gather and dev.loop.train_forms(0)['backward'] == backward
    want, noisy, _ = mirrors(pb, 30, 1e-2, int(res['k']), res['adjoint_iterations'], own=False)
    assert res['k'] >= 2 and res['adjoint_converged'] and res['adjoint_iterations'] >= 3 and scale_shows(pb, want)
    check_tight(f'large {"x".join(map(str, dims))} n{n}', res, want, noisy)
    dev.close()


# ---- 4. iteration count -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('t_max', [7, 1])
def test_truncated_adjoint(t_max, mode):
    """A map that is no contraction: the adjoint stops at adjoint_max_iter (1; 7: in the chunk behind the first five gates) and returns the truncated sum."""
    pb = C.problem(141, n=60, ds=4, gain=2.0)
    dev = Device(pb, 3, 1e-3, adjoint_max_iter=t_max, mode=mode)
    res = dev.step()
    assert res['k'] == 3.0 and res['adjoint_iterations'] == t_max and res['adjoint_converged'] is False
    want, noisy, own = mirrors(pb, 3, 1e-3, 3, t_max, adjoint_max_iter=t_max)
    assert own['adjoint_iterations'] == t_max and not own['adjoint_converged']
    check_tight(f'truncated at {t_max} mode {mode}', res, want, noisy)
    dev.close()


@pytest.mark.parametrize('mode', [1, 2])
def test_converging_run_counts_as_the_mirror(mode):
    """Threshold 1e-2 (the float32 rounding of z is four orders below the movement the gate looks for): the count and `converged` are the mirror's own,
    past the first chunk of five iterations."""
    pb = C.problem(143, n=60, ds=4, gain=0.8)
    dev = Device(pb, 60, 1e-2, mode=mode)
    res = dev.step()
    want, noisy, own = mirrors(pb, 60, 1e-2, int(res['k']), res['adjoint_iterations'])
    assert own['adjoint_converged'] and res['adjoint_converged'] is True and res['adjoint_iterations'] == own['adjoint_iterations'] > 5
    assert res['info'] == dict(iterations=own['adjoint_iterations'], converged=True, gather='narrow' if mode == 1 else 'rows')
    check_tight(f'converging mode {mode}', res, want, noisy)
    dev.close()


# ---- 5. invariants after a step -----------------------------------------------------------------------------------------------------------------------
def _bn_output_problem(seed=151, **kw):
    pb = C.problem(seed, n=50, ds=4, **kw)
    rng = np.random.default_rng(seed + 1)
    pb['ou'] = make_mlp(rng, pb['ou']['weights'][0].shape[0], [7, 2], 'tanh', out_activation='softmax', bn_random=True)
    return pb


def _armed(pb, max_iter=40, frozen='frozen', mode=1, momentum=0.9):
    dev = Device(pb, max_iter, 1e-2, mode=mode, frozen=frozen)
    dev.loop.arm_optimizer(ADAM[0], ADAM[1], True, momentum, momentum)
    res = dev.step()
    out = res, [np.array(w) for w in dev.mst.get_weights()], [np.array(w) for w in dev.mou.get_weights()]
    dev.close()
    return out


def test_invariants_after_an_armed_step():
    pb = _bn_output_problem()
    L = len(pb['st']['activations'])
    before_s, before_o = [np.asarray(w, np.float32) for w in pb['st']['weights']], [np.asarray(w, np.float32) for w in pb['ou']['weights']]
    res, after_s, after_o = _armed(pb)
    assert res['k'] >= 2 and res['adjoint_iterations'] >= 2
    # net_state: the moving statistics bit-unchanged, every trainable array - gamma and beta included - moved
    assert np.array_equal(after_s[2 * L + 2], before_s[2 * L + 2]) and np.array_equal(after_s[2 * L + 3], before_s[2 * L + 3])
    for i in range(2 * L + 2): assert not np.array_equal(after_s[i], before_s[i]), i
    for i in (2 * L, 2 * L + 1): assert np.abs(after_s[i] - before_s[i]).min() > 1e-3       # (Adam: every entry moves by about the rate)
    # net_output: updated from the batch statistics of its one call, as the mirror has them
    want = bm.step(pb['g'], pb['st'], pb['ou'], pb['D'], 40, 1e-2, pb['s0'], {}, pb['targets'], pb['weights'], k_forced=int(res['k']),
                   iterations_forced=res['adjoint_iterations'])
    cache = want['ctx']['cache_o']
    for i, batch in ((-2, cache['batch_mean']), (-1, cache['batch_var'])):
        assert np.max(np.abs(after_o[i] - (before_o[i] * 0.9 + batch * 0.1))) <= 1e-6 and np.max(np.abs(after_o[i] - before_o[i])) > 1e-3
    # two identical steps: identical bits, results and weights
    res2, again_s, again_o = _armed(pb)
    assert res2['loss'] == res['loss'] and res2['info'] == res['info']
    for key, a in arrays(res).items(): assert np.array_equal(a, arrays(res2)[key]), key
    assert all(np.array_equal(a, b) for a, b in zip(after_s + after_o, again_s + again_o))


def test_net_output_is_updated_as_in_mode_0():
    """max_iteration 0: no body runs in either mode, so net_output sees the same rows - its gradients, its updated weights and its moving statistics
    are those of the unrolled step bit for bit."""
    pb = _bn_output_problem(seed=153)
    res_f, s_f, o_f = _armed(pb, max_iter=0)
    res_u, s_u, o_u = _armed(pb, max_iter=0, frozen=None, mode=0)
    assert res_f['k'] == res_u['k'] == 0.0 and res_f['loss'] == res_u['loss']
    assert all(np.array_equal(a, b) for a, b in zip(res_f['grads_output'], res_u['grads_output']))
    assert all(np.array_equal(a, b) for a, b in zip(o_f, o_u))


def test_the_separate_steps_leave_the_moving_statistics_too():
    """gnn_loop_optimizer_step behind an unarmed step, and gnn_loop_update_moving_statistics behind a training-mode forward."""
    pb = _bn_output_problem(seed=155)
    L = len(pb['st']['activations'])
    moving = [np.asarray(w, np.float32) for w in pb['st']['weights'][2 * L + 2:]]
    dev = Device(pb, 40, 1e-2)
    dev.step()
    dev.loop.optimizer_step(ADAM[0], ADAM[1], 1.0, 0.9, 0.9)
    w = dev.mst.get_weights()
    assert np.array_equal(w[2 * L + 2], moving[0]) and np.array_equal(w[2 * L + 3], moving[1]) and not np.array_equal(w[2 * L], pb['st']['weights'][2 * L])
    out_moving = np.array(dev.mou.get_weights()[-1])
    dev.loop.train_forward(dev.mst, dev.mou, None)
    dev.loop.update_moving_statistics(0.9, 0.9)
    w = dev.mst.get_weights()
    assert np.array_equal(w[2 * L + 2], moving[0]) and np.array_equal(w[2 * L + 3], moving[1])
    assert not np.array_equal(dev.mou.get_weights()[-1], out_moving)
    # the halves: no d_nodes, and the backward pass returns no batch statistics of net_state
    dev.loop.train_forward(dev.mst, dev.mou, None)
    d_out = np.ones((dev.loop.n_masked, 2), np.float32)
    with pytest.raises(NotImplementedError, match='d_nodes'): dev.loop.train_backward(d_out, want_d_nodes=True)
    assert dev.loop.train_backward(d_out)['bn_batch_state'].shape[0] == 0
    dev.close()


# ---- 6. model types -------------------------------------------------------------------------------------------------------------------------------------
def _sequential(net):
    from GNN.MLP import Sequential, Dense, Dropout, BatchNormalization
    layers = []
    for l in range(len(net['activations'])):
        if net.get('dropout', {}).get(l): layers.append(Dropout(net['dropout'][l]))
        layers.append(Dense(net['weights'][2 * l].shape[1], net['activations'][l], input_shape=(net['weights'][2 * l].shape[0],)))
    if net['batch_normalization']: layers.append(BatchNormalization())
    seq = Sequential(layers)
    seq.set_weights([np.asarray(w, np.float32) for w in net['weights']])
    return seq


LR = 0.05


def _typed(kind, seed=161, device_optimizer=True):
    """A model of the given type ('n', 'g', 'a') whose net_state ends in BatchNormalization and whose net_output has Dropout and BatchNormalization."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased, GNNedgeBased
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(seed)
    n, nl, al, ds = (32 * 18 if kind == 'g' else 90), 3, 2, 4
    arcs = random_arcs(rng, n, 2 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if kind == 'g':
        arcs = arcs[(arcs[:, 0] // 18) == (arcs[:, 1] // 18)]
        ng = np.zeros((n, 32), np.float32)
        ng[np.arange(n), np.arange(n) // 18] = 1.0 / 18
    rows = len(arcs) if kind == 'a' else n
    set_mask = np.ones(rows, bool) if kind == 'g' else rng.random(rows) < 0.75
    n_t = 32 if kind == 'g' else rows
    targets_full = np.eye(2)[rng.integers(0, 2, n_t)].astype(np.float32)
    weights_full = (rng.uniform(0.5, 1.5, n_t) / n_t).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    g['set_mask'], g['output_mask'] = set_mask, np.ones(rows, bool)
    m = int(set_mask.sum())
    st = C.frozen_net(rng, al + 2 * (ds + nl), [12, ds], 'tanh', 0.3)
    ou = make_mlp(rng, (2 * (ds + nl) + al) if kind == 'a' else ds + nl, [7, 2], 'tanh', out_activation='softmax', bn_random=True)
    st['dropout'], ou['dropout'] = {}, {1: 0.3}
    mo = {1: rng.random((m, 7)) > 0.3}
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    cls = {'n': GNNnodeBased, 'g': GNNgraphBased, 'a': GNNedgeBased}[kind]
    gnn = cls(net_state=_sequential(st), net_output=_sequential(ou), optimizer=optimizers.SGD(LR), loss_function=losses.categorical_crossentropy,
              loss_arguments=None, state_vect_dim=ds, max_iteration=30, threshold=1e-3, addressed_problem='c')
    gnn.impl = 1
    gnn.device_optimizer = device_optimizer
    gnn.set_gradient_mode('fixed_point', batch_normalization='frozen')
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based=kind,
                     aggregation_mode='average', NodeGraph=ng)
    sel = np.ones(n_t, bool) if kind == 'g' else set_mask
    return dict(gnn=gnn, batch=GraphTensor.fromGraphObject(go), g=g, st=st, ou=ou, ds=ds, mo=mo, s0=s0, targets=targets_full[sel], weights=weights_full[sel])


@pytest.mark.parametrize('kind', ['n', 'g', 'a'])
def test_model_types(kind):
    """Node-, graph- and edge-based steps through training_step with the keyword: the host-optimizer path returns the raw gradients, compared with the
    mirror (1e-3 of each array's largest entry, as tests/test_gpu_adjoint.py); the armed device step lands on the same weights to 1e-6; on both
    paths net_state's moving statistics are bit-unchanged and gamma / beta move."""
    t = _typed(kind, device_optimizer=False)
    mo_flat = t['mo'][1].astype(np.uint8).ravel()
    before = [np.array(w) for w in t['gnn'].net_state.get_weights()]
    res = t['gnn'].training_step(t['batch'], mean=True, state0=t['s0'], masks_output=mo_flat)
    kw = dict(graph_based=kind == 'g', edge_based=kind == 'a')
    want = bm.step(t['g'], t['st'], t['ou'], t['ds'], 30, 1e-3, t['s0'], t['mo'], t['targets'], t['weights'], k_forced=int(res['k']),
                   iterations_forced=res['adjoint_iterations'], **kw)
    assert res['k'] >= 2 and res['adjoint_converged'] and res['adjoint_iterations'] >= 2
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    assert len(res['grads_state']) == len(want['grads_state']) == 6
    for got, w in list(zip(res['grads_state'], want['grads_state'])) + list(zip(res['grads_output'], want['grads_output'])):
        assert got.shape == w.shape and np.max(np.abs(got - w)) <= 1e-3 * max(1e-3, np.max(np.abs(w))), (got.shape, np.max(np.abs(got - w)), np.max(np.abs(w)))
    host = [np.array(w) for w in t['gnn'].net_state.get_weights()]
    assert np.array_equal(host[6], before[6]) and np.array_equal(host[7], before[7])
    for i in range(6):                                       # plain SGD with the UNDIVIDED gradients (mean = True, k >= 2)
        assert np.max(np.abs(host[i].astype(np.float64) - (before[i].astype(np.float64) - LR * res['grads_state'][i]))) <= 1e-6
    assert np.max(np.abs(host[4] - before[4])) > 1e-4 and np.max(np.abs(host[5] - before[5])) > 1e-4
    d = _typed(kind, device_optimizer=True)
    res_d = d['gnn'].training_step(d['batch'], mean=True, state0=d['s0'], masks_output=mo_flat)
    assert res_d['k'] == res['k'] and res_d['adjoint_iterations'] == res['adjoint_iterations']
    for a, b in zip(d['gnn'].net_state.get_weights() + d['gnn'].net_output.get_weights(), t['gnn'].net_state.get_weights() + t['gnn'].net_output.get_weights()):
        assert np.max(np.abs(np.asarray(a) - np.asarray(b))) <= 1e-6
    dev_w = d['gnn'].net_state.get_weights()
    assert np.array_equal(dev_w[6], before[6]) and np.array_equal(dev_w[7], before[7])


def _mutag_like(seed=0, graphs=12):
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(graphs):
        n = int(rng.integers(10, 25))
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        cls = int(nodes[:, 0].mean() + 0.5 * nodes[:, 1].mean() > 0)
        out.append(GraphObject(arcs=random_arcs(rng, n, 2 * n, 1), nodes=nodes, targets=np.eye(2)[[cls]], problem_based='g', aggregation_mode='average',
                               NodeGraph=np.ones((n, 1), np.float32) / n))
    return GraphObject.merge(out, problem_based='g', aggregation_mode='average')


def _default_model(cls=None, layer=0):
    """net_state as MLP() builds it by default: ending in a BatchNormalization."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNgraphBased
    from GNN.MLP import MLP, set_seed
    set_seed(7)
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (4 + 3 + extra), [10, 4], 'tanh', 'glorot_normal', 'zeros')
    ou = MLP(4 + 3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    assert st.batch_normalization
    return (cls or GNNgraphBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                  loss_arguments=None, state_vect_dim=4, max_iteration=15, threshold=0.01, addressed_problem='c')


def test_train_reduces_the_loss_of_a_default_net():
    batch = _mutag_like()
    gnn = _default_model()
    with pytest.raises(NotImplementedError): gnn.set_gradient_mode('fixed_point')
    gnn.set_gradient_mode('fixed_point', batch_normalization='frozen')
    moving = [np.array(w) for w in gnn.net_state.get_weights()[-2:]]
    before = gnn.test(batch)['Loss']
    gnn.train(batch, 12, update_freq=4, verbose=0)
    assert gnn.test(batch)['Loss'] < 0.9 * before
    assert all(np.array_equal(a, b) for a, b in zip(gnn.net_state.get_weights()[-2:], moving))
    assert not np.array_equal(gnn.net_state.get_weights()[-4], np.ones(4, np.float32))      # gamma has trained


def test_lgnn_serial_trains_and_parallel_still_raises():
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(3)
    graphs = []
    for _ in range(3):
        nodes = (2 * rng.random((60, 3)) - 1).astype(np.float32)
        graphs.append(GraphObject(arcs=random_arcs(rng, 60, 150, 1), nodes=nodes, targets=np.eye(2)[(nodes[:, 0] > 0).astype(int)]))
    lgnn = LGNN([_default_model(GNNnodeBased), _default_model(GNNnodeBased, layer=1)], get_state=False, get_output=True,
                optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    lgnn.set_gradient_mode('fixed_point', batch_normalization='frozen')
    moving = [np.array(w) for gnn in lgnn.gnns for w in gnn.net_state.get_weights()[-2:]]
    before = lgnn.test(graphs)['Loss']
    lgnn.train(graphs, 8, update_freq=4, training_mode='serial', verbose=0)
    assert lgnn.test(graphs)['Loss'] < before
    assert all(np.array_equal(a, b) for a, b in zip([w for gnn in lgnn.gnns for w in gnn.net_state.get_weights()[-2:]], moving))
    with pytest.raises(NotImplementedError, match='fixed_point'): lgnn.copy().train(graphs, 1, training_mode='parallel', verbose=0)


# ---- 7. flag off, refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
def test_flag_changes_nothing_without_batch_normalization(mode):
    """A net_state without BatchNormalization: the step of a loop set through gnn_loop_set_gradient_mode_ex with the flag returns the bits of one
    set through gnn_loop_set_gradient_mode."""
    pb = C.problem(171, n=37, ds=5, bn=False, gain=0.5)
    results = []
    for frozen in ('frozen', None):
        dev = Device(pb, 50, 1e-2, mode=mode, frozen=frozen)
        results.append(dev.step())
        dev.close()
    a, b = results
    assert a['loss'] == b['loss'] and a['k'] == b['k'] >= 2 and a['info'] == b['info'] and a['adjoint_iterations'] >= 2
    for key, x in arrays(a).items(): assert np.array_equal(x, arrays(b)[key]), key


def test_refusals_with_and_without_the_flag():
    pb = C.problem(173, n=20, ds=4)
    with pytest.raises(NotImplementedError, match='BatchNormalization'): Device(pb, 5, 1e-2, frozen=None)
    dev = Device(pb, 5, 1e-2)
    with pytest.raises(NotImplementedError, match='Dropout'):
        dev.loop.train_step(dev.mst, dev.mou, None, pb['targets'], pb['weights'], 0, dropout_state=[0.0, 0.2, 0.0])
    with pytest.raises(ValueError): dev.loop.set_gradient_mode(1, batch_normalization='batch')
    with pytest.raises(NotImplementedError, match='BatchNormalization'): dev.loop.set_gradient_mode(1)      # the plain entry point still refuses
    assert dev.step()['adjoint_iterations'] >= 1                                                            # ... and left the loop as it was
    assert dev.loop.set_gradient_mode('unrolled') == 0 and 'adjoint_iterations' not in dev.loop.train_step(dev.mst, dev.mou, None, pb['targets'], pb['weights'], 0)
    dev.close()
