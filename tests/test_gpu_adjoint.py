"""Gradient mode 1 ("fixed point": gnn_loop_set_gradient_mode, include/gnn_hip.h) on the device against its float64 mirror (tests/adjoint_mirror.py).

Criterion of the tight comparisons (the method and MARGIN = 8 of tests/test_gpu_train_forms.py): the mirror is evaluated a second time in float32;
an array passes when every element lies within MARGIN x max |mirror_f32 - mirror_f64| over that array, plus FLOOR x max |mirror_f64| - two units in the
last place of the array's largest entry, for arrays whose own float32 evaluation happens to be exact (noise 0) while the device rounds once.  The
measured ratios are in profiles/fixed_point_gradients.txt (GNN_ADJOINT_RATIOS=<file> appends them): the largest is 5.84, and no measured array needs the floor.

Forms: loops in mode 1 take the one-launch iteration of narrow nets (k_adjoint_narrow) wherever gnn_adjoint_form says so - most small cases below -
and the same cases run once more in mode 2, the per-kernel chain with the separate gather kernels, held to the same criterion.

No gate decision enters a gradient comparison: the mirror runs exactly the device's k bodies and the device's count of adjoint iterations.  The counts
themselves are compared with the mirror's OWN gates: equal at threshold 1e-2; within one iteration at 1e-6, where the float32 rounding of z (6e-8
relative) is a tenth of the movement the gate looks for, so a node close to the threshold may pass one iteration earlier or later - the movement
shrinks geometrically, one iteration moves every node far across.

Arithmetic of the forward: these loops run on impl 1 (bit-exact float32) - the default path's fp16-piece states differ from float32 ones by up to 2e-6
relative (tests/test_gpu_parity.py), which is the forward's own tolerance and not what this file measures; one case runs the default path at 1e-3."""
import os

import numpy as np
import pytest

import adjoint_mirror as am
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -22
KINDS = {'categorical_crossentropy': 0, 'mean_squared_error': 1}


def problem(seed, n, ds, nl=2, al=1, hidden=(7,), act='tanh', gain=0.5, n_und=None, isolated=False, hub=0, mask_p=0.7, D=None):
    """Graph, nets, initial state, targets.  isolated: node 1 loses every arc; hub: node 0 gets that many out-arcs."""
    rng = np.random.default_rng(seed)
    n_und = 2 * n if n_und is None else n_und
    arcs = random_arcs(rng, n, n_und, al) if n > 1 else np.zeros((0, 2 + al), np.float32)
    if hub:
        dst = rng.permutation(np.arange(1, n))[:hub]
        extra = np.concatenate([np.zeros((hub, 1)), dst[:, None], 2 * rng.random((hub, al)) - 1], axis=1).astype(np.float32)
        arcs = np.concatenate([arcs, extra])
        _, first = np.unique(arcs[:, :2], axis=0, return_index=True)
        arcs = arcs[np.sort(first)]
        arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    if isolated: arcs = arcs[(arcs[:, 0] != 1) & (arcs[:, 1] != 1)]
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < mask_p
    g['set_mask'][0] = True                                   # at least one row carries g; with mask_p < 1 others carry none
    D = ds if D is None else D
    nlc = nl if D else 0
    st = make_mlp(rng, al + 2 * (ds + nlc), list(hidden) + [ds], act, gain=gain, batch_normalization=False)
    ou = make_mlp(rng, ds + nlc, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    targets = np.eye(2)[rng.integers(0, 2, m)].astype(np.float32)
    weights = rng.uniform(0.5, 1.5, m).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    return dict(g=g, st=st, ou=ou, ds=ds, D=D, s0=s0 if D else None, targets=targets, weights=weights, n=n)


class Device:
    """The loop of a problem on the device, in fixed-point mode unless told otherwise."""

    def __init__(self, pb, max_iter, thr, state0=None, impl=1, mode=1, adjoint_max_iter=None, adjoint_threshold=None):
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
        self.loop.set_gradient_mode(mode, adjoint_max_iter, adjoint_threshold)
        self.pb = pb

    def step(self, loss='categorical_crossentropy', **kw):
        pb = self.pb
        res = self.loop.train_step(self.mst, self.mou, None, pb['targets'], pb['weights'], KINDS[loss], **kw)
        res['state'], res['out'] = self.loop.state(), self.loop.output()
        res['info'] = self.loop.adjoint_info()
        return res

    def close(self):
        self.loop.close(); self.graph.close()


def arrays(r):
    out = {'state': r['state'], 'out': r['out']}
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def record(lines):
    path = os.environ.get('GNN_ADJOINT_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))


def mirrors(pb, max_iter, thr, state0, k, iterations, adjoint_threshold=None, loss='categorical_crossentropy', **kw):
    """The mirror with the device's counts forced, in float64 and float32; and with the device's k but its OWN adjoint gate, in float64."""
    s0 = pb['s0'] if state0 is None else state0
    args = (pb['g'], pb['st'], pb['ou'], pb['D'], max_iter, thr, s0, {}, pb['targets'], pb['weights'])
    want = am.step(*args, loss=loss, k_forced=k, iterations_forced=iterations, **kw)
    noisy = am.step(*args, loss=loss, k_forced=k, iterations_forced=iterations, dtype=np.float32, **kw)
    own = am.step(*args, loss=loss, k_forced=k, adjoint_threshold=adjoint_threshold, **kw)
    return want, noisy, own


def check_tight(tag, res, want, noisy):
    got, w64, w32 = arrays(res), arrays(want), arrays(noisy)
    lines, bad = [], []
    for key, a in got.items():
        w = np.asarray(w64[key], np.float64)
        assert a.shape == w.shape, key
        noise = float(np.max(np.abs(np.asarray(w32[key], np.float64) - w))) if w.size else 0.0
        top = float(np.max(np.abs(w))) if w.size else 0.0
        err = float(np.max(np.abs(a.astype(np.float64) - w))) if w.size else 0.0
        lines.append(f'{tag:34s} {key:16s} err {err:9.3e}  noise {noise:9.3e}  ratio {err / noise if noise > 0 else float("nan"):6.2f}  floor {FLOOR * top:9.3e}  max|ref| {top:9.3e}')
        if w.size and not np.all(np.abs(a.astype(np.float64) - w) <= MARGIN * noise + FLOOR * top): bad.append(lines[-1])
    record(lines)
    print('\n'.join(lines))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    assert not bad, '\n' + '\n'.join(bad)


# ---- 1. tight fixed point -------------------------------------------------------------------------------------------------------------------------
TIGHT = [dict(n=1, ds=3), dict(n=15, ds=4), dict(n=16, ds=8), dict(n=17, ds=64, hidden=(20,)), dict(n=37, ds=3, isolated=True),
         dict(n=37, ds=8, hidden=(9, 6)), dict(n=83, ds=4, hub=70, isolated=True), dict(n=83, ds=3, hub=70, hidden=())]


def expected_gather(pb, mode):
    """What gnn_adjoint_form says an iteration of this problem's net_state launches in mode 1; in mode 2 the gather kernel of its state width."""
    from GNN import _engine as e
    dims = [pb['st']['weights'][0].shape[0]] + [w.shape[0] for w in pb['st']['weights'][1::2]]
    f = e.adjoint_form(dims, pb['st']['activations'], pb['n'])
    chain = 'rows' if pb['ds'] % 4 == 0 and pb['ds'] <= 64 else 'generic'
    return f['gather'] if mode == 1 else (chain if f['gather'] == 'narrow' else f['gather'])


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', TIGHT, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_tight_fixed_point(case, mode):
    """state0 = the float64 fixed point cast to float32, both thresholds 1e-6: outputs, loss, both gradient sets, k and the adjoint count."""
    pb = problem(11, **case)
    g = pb['g']
    p64 = am.forward(g, pb['st'], pb['ou'], pb['D'], 3000, 1e-15, pb['s0'], {})['state']
    p32 = p64.astype(np.float32)
    dev = Device(pb, 50, 1e-6, state0=p32, mode=mode)
    res, again = dev.step(), dev.step()
    want, noisy, own = mirrors(pb, 50, 1e-6, p32, int(res['k']), res['adjoint_iterations'])
    assert res['k'] == 1.0 == am.forward(g, pb['st'], pb['ou'], pb['D'], 50, 1e-6, p32, {})['k']      # body 0 always runs; it does not move p
    assert res['adjoint_converged'] and own['adjoint_converged'] and abs(res['adjoint_iterations'] - own['adjoint_iterations']) <= 1, (res['info'], own['adjoint_iterations'])
    assert res['info'] == dict(iterations=res['adjoint_iterations'], converged=True, gather=expected_gather(pb, mode))
    if mode == 1: assert (res['info']['gather'] == 'narrow') == (case['ds'] != 64)          # (Ds = 64: a 133-wide concat)
    if pb['n'] > 1: assert res['adjoint_iterations'] >= 3 and (np.abs(want['g']).max(axis=1) == 0).any()      # rows with g = 0 exist
    check_tight(f'tight n{case["n"]} ds{case["ds"]} mode {mode}', res, want, noisy)
    for key, a in arrays(res).items(): assert np.array_equal(a, arrays(again)[key]), key
    assert again['loss'] == res['loss'] and again['info'] == res['info']
    dev.close()


# ---- 2. loose threshold -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('n,ds', [(37, 3), (37, 8), (300, 4)])
def test_loose_threshold(n, ds, mode):
    pb = problem(21, n=n, ds=ds, hub=20 if n > 100 else 0)
    dev = Device(pb, 50, 1e-2, mode=mode)
    res = dev.step()
    assert res['info']['gather'] == expected_gather(pb, mode) == ('narrow' if mode == 1 else 'rows' if ds % 4 == 0 else 'generic')
    want, noisy, own = mirrors(pb, 50, 1e-2, None, int(res['k']), res['adjoint_iterations'])
    assert 2 <= res['k'] < 50 and res['adjoint_converged'] and res['adjoint_iterations'] == own['adjoint_iterations'] >= 2
    check_tight(f'loose n{n} ds{ds} mode {mode}', res, want, noisy)
    dev.close()


@pytest.mark.parametrize('act,impl', [('selu', 1), ('relu', 1), ('tanh', None)])
def test_loose_threshold_kinked_and_default_path(act, impl):
    """selu and relu nets, and a tanh net on the loop's default arithmetic: 1e-3 relative to the largest entry of each array (tests/test_gpu_train.py)."""
    pb = problem(23, n=200, ds=8, hidden=(12,), act=act, gain=0.5)
    dev = Device(pb, 50, 1e-2, impl=impl)
    res = dev.step()
    want = am.step(pb['g'], pb['st'], pb['ou'], pb['D'], 50, 1e-2, pb['s0'], {}, pb['targets'], pb['weights'], k_forced=int(res['k']),
                   iterations_forced=res['adjoint_iterations'])
    assert res['k'] >= 2 and res['adjoint_iterations'] >= 2 and res['adjoint_converged']
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    for key, a in arrays(res).items():
        w = np.asarray(arrays(want)[key])
        assert np.max(np.abs(a - w)) <= 1e-3 * max(1e-3, np.max(np.abs(w))), (key, np.max(np.abs(a - w)), np.max(np.abs(w)))
    dev.close()


# ---- 3. every recorded form -----------------------------------------------------------------------------------------------------------------------
def wide_problem(dims, n):
    ds = dims[-1]
    rest = dims[0] - 2 * ds
    al = 1 + (rest + 1) % 2
    nl = (rest - al) // 2
    assert al + 2 * (ds + nl) == dims[0]
    return problem(31, n=n, ds=ds, nl=nl, al=al, hidden=dims[1:-1], gain=0.5, n_und=n)


# the one-launch iteration: rows at its group size (16) - 1 | = | + 1 and past two groups, 1 / 2 / 3 layers, widths 1, 5, 32, 33 and 64, concat 96
NARROW = [((11, 3), 15), ((11, 3), 16), ((11, 3), 17), ((13, 5, 4), 17), ((13, 1, 4), 33), ((13, 32, 4), 16), ((96, 64, 33, 32), 40), ((31, 32, 32, 14), 935)]
FORMS = [(d, n, ['adjoint_narrow'] * (len(d) - 1), 'narrow') for d, n in NARROW] + [((97, 30, 12), 50, ['per_op'] * 2, 'rows'),
         ((135, 128, 128, 64), 4113, ['chain3'] * 3, 'rows_aligned'), ((135, 144, 64), 4113, ['wide'] * 2, 'rows'),
         ((135, 128, 32, 64), 4113, ['wide', 'per_op', 'per_op'], 'rows'), ((135, 128, 128, 64), 4095, ['per_op'] * 3, 'rows')]
WHY_NOT = {(97, 30, 12): 'concat', (135, 128, 128, 64): 'width', (135, 144, 64): 'width', (135, 128, 32, 64): 'width'}


@pytest.mark.parametrize('dims,n,backward,gather', FORMS, ids=lambda v: str(v).replace(' ', '') if isinstance(v, (tuple, int)) else None)
def test_every_backward_and_gather_form(dims, n, backward, gather):
    """The adjoint iteration as one launch (k_adjoint_narrow) and on every form net_backward takes without weight gradients - the row blocks of k_layer_bwd (behind a 97-wide concat),
    the wide product per layer, the three-layer chain with its aligned rows, a mix of two in one net - and the weight-gradient pass behind it."""
    from GNN import _engine as e
    pb = wide_problem(dims, n)
    assert e.adjoint_form(dims, ['tanh'] * (len(dims) - 1), n) == dict(eligible=True, reason=None, gather=gather, backward=backward, narrow_refusal=WHY_NOT.get(dims))
    dev = Device(pb, 30, 1e-2)
    res, again = dev.step(), dev.step()
    assert res['info']['gather'] == gather and (gather == 'narrow' or dev.loop.train_forms(0)['backward'] == backward)
    want, noisy, own = mirrors(pb, 30, 1e-2, None, int(res['k']), res['adjoint_iterations'])
    assert res['k'] >= 2 and res['adjoint_converged'] and res['adjoint_iterations'] == own['adjoint_iterations'] >= 2
    check_tight(f'form {"x".join(map(str, dims))} n{n}', res, want, noisy)
    for key, a in arrays(res).items(): assert np.array_equal(a, arrays(again)[key]), key
    dev.close()
    if gather == 'narrow':          # the per-kernel chain on the same net: same counts, and (both within the criterion of the mirror) the same gradients
        chain = Device(pb, 30, 1e-2, mode=2)
        other = chain.step()
        assert other['info']['gather'] in ('rows', 'generic') and (other['k'], other['adjoint_iterations']) == (res['k'], res['adjoint_iterations'])
        check_tight(f'form {"x".join(map(str, dims))} n{n} chain', other, want, noisy)
        chain.close()


# ---- 4. truncation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('t_max', [7, 6, 5, 1])
def test_truncated_adjoint(t_max, mode):
    """A map that is no contraction: the adjoint stops at adjoint_max_iter (7 and 6: in the chunk behind the first five gates; 5: at its end; 1), in both forms, reports it, and returns
    the truncated sum."""
    pb = problem(41, n=60, ds=4, gain=3.0)
    dev = Device(pb, 3, 1e-3, adjoint_max_iter=t_max, mode=mode)
    res = dev.step()
    assert res['k'] == 3.0 and res['adjoint_iterations'] == t_max and res['adjoint_converged'] is False
    want, noisy, own = mirrors(pb, 3, 1e-3, None, 3, t_max, adjoint_max_iter=t_max)
    assert own['adjoint_iterations'] == t_max and not own['adjoint_converged']
    check_tight(f'truncated at {t_max}', res, want, noisy)
    dev.close()


def test_adjoint_settings_default_to_the_loops():
    """adjoint_max_iter 0 / threshold < 0 = the loop's own; a looser adjoint threshold stops earlier; k == 0 bodies (max_iter 0) still has a gradient."""
    pb = problem(43, n=60, ds=4)
    counts = []
    for kw in (dict(), dict(adjoint_threshold=1e-1), dict(adjoint_max_iter=2)):
        dev = Device(pb, 40, 1e-4, **kw)
        res = dev.step()
        own = am.step(pb['g'], pb['st'], pb['ou'], pb['D'], 40, 1e-4, pb['s0'], {}, pb['targets'], pb['weights'], k_forced=int(res['k']),
                      adjoint_max_iter=kw.get('adjoint_max_iter'), adjoint_threshold=kw.get('adjoint_threshold'))
        assert res['adjoint_iterations'] == own['adjoint_iterations'] and res['adjoint_converged'] == own['adjoint_converged']
        counts.append(res['adjoint_iterations'])
        dev.close()
    assert counts[0] > counts[1] > 1 and counts[2] == 2
    dev = Device(pb, 0, 1e-4, adjoint_max_iter=20)
    res = dev.step()
    want, noisy, _ = mirrors(pb, 0, 1e-4, None, 0, res['adjoint_iterations'], adjoint_max_iter=20)
    assert res['k'] == 0.0 and np.array_equal(res['state'], pb['s0']) and res['adjoint_iterations'] >= 2
    check_tight('no body', res, want, noisy)
    dev.close()


# ---- 5. model types ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dim_zero_and_extra_state_gradient():
    """D == 0 (the state starts as the node labels), and the two halves with d_state_extra: g includes it."""
    from GNN import _engine as e
    pb = problem(51, n=45, ds=3, nl=3, D=0)
    dev = Device(pb, 40, 1e-3)
    res = dev.step(loss='mean_squared_error')
    want, noisy, own = mirrors(pb, 40, 1e-3, None, int(res['k']), res['adjoint_iterations'], loss='mean_squared_error')
    assert res['k'] >= 2 and res['adjoint_iterations'] == own['adjoint_iterations']
    check_tight('D0 mse', res, want, noisy)
    # forward / backward halves with an extra gradient on the final state
    rng = np.random.default_rng(5)
    k, out = dev.loop.train_forward(dev.mst, dev.mou, None)
    assert k == res['k'] and np.array_equal(out, res['out'])
    m = out.shape[0]
    d_out, dse = rng.standard_normal((m, 2)).astype(np.float32), rng.standard_normal((pb['n'], 3)).astype(np.float32)
    with pytest.raises(NotImplementedError, match='d_nodes'): dev.loop.train_backward(d_out, dse, want_d_nodes=True)
    back = dev.loop.train_backward(d_out, dse)
    info = dev.loop.adjoint_info()
    for dt, store in ((np.float64, {}), (np.float32, {})):
        ctx = am.forward(pb['g'], pb['st'], pb['ou'], 0, 40, 1e-3, None, {}, dtype=dt, k_forced=int(k))
        gs, go = am.state_gradient(ctx, d_out.astype(dt), dse.astype(dt))
        z, it, conv, grads = am.adjoint(ctx, gs, 40, 1e-3, iterations_forced=info['iterations'])
        store.update(state=ctx['state'], out=ctx['out_nodes'], grads_state=grads, grads_output=go, loss=0.0)
        if dt is np.float64: w64 = store
        else: w32 = store
    back.update(state=dev.loop.state(), out=out, loss=0.0)
    check_tight('D0 halves + extra', back, w64, w32)
    dev.close()


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


def _typed(kind, seed=61, device_optimizer=True, mode='fixed_point'):
    """A model of the given type ('n', 'g', 'a') whose net_output has Dropout and BatchNormalization, its batch and the mirror's inputs."""
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased, GNNgraphBased, GNNedgeBased
    from GNN.graph_class import GraphObject, GraphTensor
    rng = np.random.default_rng(seed)
    n, nl, al, ds = (32 * 18 if kind == 'g' else 90), 3, 2, 4
    arcs = random_arcs(rng, n, 2 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if kind == 'g':                                            # a MUTAG-sized batch: 32 graphs of 18 nodes, arcs inside the graphs only
        arcs = arcs[(arcs[:, 0] // 18) == (arcs[:, 1] // 18)]
        ng = np.zeros((n, 32), np.float32)
        ng[np.arange(n), np.arange(n) // 18] = 1.0 / 18
    e_ = len(arcs)
    rows = e_ if kind == 'a' else n
    set_mask = np.ones(rows, bool) if kind == 'g' else rng.random(rows) < 0.75
    n_t = 32 if kind == 'g' else rows
    targets_full = np.eye(2)[rng.integers(0, 2, n_t)].astype(np.float32)
    weights_full = (rng.uniform(0.5, 1.5, n_t) / n_t).astype(np.float32)           # (a loss of order 1)
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    g['set_mask'], g['output_mask'] = set_mask, np.ones(rows, bool)
    m = int(set_mask.sum())
    st = make_mlp(rng, al + 2 * (ds + nl), [12, ds], 'tanh', gain=0.5, batch_normalization=False)
    ou = make_mlp(rng, (2 * (ds + nl) + al) if kind == 'a' else ds + nl, [7, 2], 'tanh', out_activation='softmax', bn_random=True)
    st['dropout'], ou['dropout'] = {}, {1: 0.3}
    mo = {1: rng.random((m, 7)) > 0.3}
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    cls = {'n': GNNnodeBased, 'g': GNNgraphBased, 'a': GNNedgeBased}[kind]
    gnn = cls(net_state=_sequential(st), net_output=_sequential(ou), optimizer=optimizers.SGD(LR), loss_function=losses.categorical_crossentropy,
              loss_arguments=None, state_vect_dim=ds, max_iteration=30, threshold=1e-3, addressed_problem='c')
    gnn.impl = 1
    gnn.device_optimizer = device_optimizer
    gnn.set_gradient_mode(mode)
    go = GraphObject(arcs=arcs, nodes=nodes, targets=targets_full, set_mask=set_mask, sample_weights=weights_full, problem_based=kind,
                     aggregation_mode='average', NodeGraph=ng)
    sel = np.ones(n_t, bool) if kind == 'g' else set_mask
    return dict(gnn=gnn, batch=GraphTensor.fromGraphObject(go), g=g, st=st, ou=ou, ds=ds, mo=mo, s0=s0, targets=targets_full[sel], weights=weights_full[sel])


@pytest.mark.parametrize('kind', ['n', 'g', 'a'])
def test_model_types_with_dropout_and_batch_normalization_in_net_output(kind):
    """Node-, graph- (NodeGraph readout over a batch of 32) and edge-based steps through training_step: the host-optimizer path returns the raw
    gradients, compared with the mirror; the armed device step lands on the same weights to 1e-6; two identical steps return identical bits."""
    t = _typed(kind, device_optimizer=False)
    mo_flat = t['mo'][1].astype(np.uint8).ravel()
    w_before = [np.array(w) for w in t['gnn'].net_state.get_weights() + t['gnn'].net_output.get_weights()]
    res = t['gnn'].training_step(t['batch'], mean=True, state0=t['s0'], masks_output=mo_flat)
    kw = dict(graph_based=kind == 'g', edge_based=kind == 'a')
    want = am.step(t['g'], t['st'], t['ou'], t['ds'], 30, 1e-3, t['s0'], t['mo'], t['targets'], t['weights'], k_forced=int(res['k']),
                   iterations_forced=res['adjoint_iterations'], **kw)
    own = am.step(t['g'], t['st'], t['ou'], t['ds'], 30, 1e-3, t['s0'], t['mo'], t['targets'], t['weights'], k_forced=int(res['k']), **kw)
    assert res['k'] >= 2 and res['adjoint_converged'] and res['adjoint_iterations'] == own['adjoint_iterations'] >= 2
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    for got, w in list(zip(res['grads_state'], want['grads_state'])) + list(zip(res['grads_output'], want['grads_output'])):
        assert got.shape == w.shape and np.max(np.abs(got - w)) <= 1e-3 * max(1e-3, np.max(np.abs(w))), (got.shape, np.max(np.abs(got - w)), np.max(np.abs(w)))
    # the host path applied the gradients UNDIVIDED although mean=True and k >= 2: plain SGD, w <- w - lr g with the gradients it returned
    n_s = len(res['grads_state'])
    trainable_before = w_before[:n_s] + w_before[len(t['st']['weights']):len(t['st']['weights']) + len(res['grads_output'])]
    host_w = t['gnn'].net_state.trainable_variables + t['gnn'].net_output.trainable_variables
    moved = 0.0
    for a, b, g_ in zip(host_w, trainable_before, res['grads_state'] + res['grads_output']):
        assert np.max(np.abs(np.asarray(a, np.float64) - (np.asarray(b, np.float64) - LR * np.asarray(g_, np.float64)))) <= 1e-6
        moved = max(moved, float(np.max(np.abs(LR * g_))))
    assert moved > 1e-3                                        # (a division by k would show)
    # armed device step: same weights as the host path
    d = _typed(kind, device_optimizer=True)
    res_d = d['gnn'].training_step(d['batch'], mean=True, state0=d['s0'], masks_output=mo_flat)
    assert res_d['k'] == res['k'] and res_d['adjoint_iterations'] == res['adjoint_iterations']
    for a, b in zip(d['gnn'].net_state.get_weights() + d['gnn'].net_output.get_weights(), t['gnn'].net_state.get_weights() + t['gnn'].net_output.get_weights()):
        assert np.max(np.abs(np.asarray(a) - np.asarray(b))) <= 1e-6
    # two identical steps of two fresh models: identical bits
    r1 = _typed(kind, device_optimizer=False)['gnn'].training_step(t['batch'], mean=True, state0=t['s0'], masks_output=mo_flat)
    assert r1['loss'] == res['loss'] and all(np.array_equal(a, b) for a, b in zip(r1['grads_state'] + r1['grads_output'], res['grads_state'] + res['grads_output']))


# ---- 6. surface -------------------------------------------------------------------------------------------------------------------------------------
def _mutag_like(seed=0, graphs=12):
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(graphs):
        n = int(rng.integers(10, 25))
        arcs = random_arcs(rng, n, 2 * n, 1)
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        cls = int(nodes[:, 0].mean() + 0.5 * nodes[:, 1].mean() > 0)      # learnable from the labels
        out.append(GraphObject(arcs=arcs, nodes=nodes, targets=np.eye(2)[[cls]], problem_based='g', aggregation_mode='average',
                               NodeGraph=np.ones((n, 1), np.float32) / n))
    return GraphObject.merge(out, problem_based='g', aggregation_mode='average')


def _graph_model(mode, cls=None, layer=0, dropout=0.0, bn=False):
    from GNN import losses, optimizers
    from GNN.GNN import GNNgraphBased
    from GNN.MLP import MLP, set_seed
    set_seed(7)
    extra = 2 * (layer > 0)
    st = MLP(1 + 2 * (4 + 3 + extra), [10, 4], 'tanh', 'glorot_normal', 'zeros', dropout_rate=dropout, dropout_pos=0, batch_normalization=bn)
    ou = MLP(4 + 3 + extra, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    gnn = (cls or GNNgraphBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=4, max_iteration=15, threshold=0.01, addressed_problem='c')
    if mode: gnn.set_gradient_mode(mode)
    return gnn


def test_training_reduces_the_loss_in_both_modes():
    batch = _mutag_like()
    for mode in ('unrolled', 'fixed_point'):
        gnn = _graph_model(mode)
        before = gnn.test(batch)['Loss']
        gnn.train(batch, 12, update_freq=4, verbose=0)
        after = gnn.test(batch)['Loss']
        assert after < 0.9 * before, (mode, before, after)
        assert gnn.copy().gradient_mode == mode


def test_refusals_on_the_device():
    """A loop refuses the mode for a net_state with BatchNormalization, a step for one with Dropout; the model classes refuse both at once."""
    from GNN import _engine as e
    pb = problem(71, n=20, ds=4)
    pb['st'] = make_mlp(np.random.default_rng(1), pb['st']['weights'][0].shape[0], [7, 4], 'tanh', gain=0.5, bn_random=True)
    with pytest.raises(NotImplementedError, match='BatchNormalization'): Device(pb, 5, 1e-2)
    pb = problem(71, n=20, ds=4)
    dev = Device(pb, 5, 1e-2)
    with pytest.raises(NotImplementedError, match='Dropout'):
        dev.loop.train_step(dev.mst, dev.mou, None, pb['targets'], pb['weights'], 0, dropout_state=[0.0, 0.2, 0.0])
    with pytest.raises(ValueError): dev.loop.set_gradient_mode('implicit')
    assert dev.loop.set_gradient_mode('unrolled') == 0 and 'adjoint_iterations' not in dev.step()
    dev.close()
    for bad in (_graph_model(None, dropout=0.2), _graph_model(None, bn=True)):
        with pytest.raises(NotImplementedError): bad.set_gradient_mode('fixed_point')


def test_lgnn_serial_trains_and_joint_modes_refuse():
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    from GNN.graph_class import GraphObject
    rng = np.random.default_rng(3)
    graphs = []
    for _ in range(3):
        n = 60
        nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        graphs.append(GraphObject(arcs=random_arcs(rng, n, 150, 1), nodes=nodes, targets=np.eye(2)[(nodes[:, 0] > 0).astype(int)]))
    lgnn = LGNN([_graph_model(None, GNNnodeBased), _graph_model(None, GNNnodeBased, layer=1)], get_state=False, get_output=True,
                optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy, loss_arguments=None, addressed_problem='c')
    lgnn.set_gradient_mode('fixed_point')
    before = lgnn.test(graphs)['Loss']
    lgnn.train(graphs, 8, update_freq=4, training_mode='serial', verbose=0)
    assert lgnn.test(graphs)['Loss'] < before
    other = lgnn.copy()
    with pytest.raises(NotImplementedError, match='fixed_point'): other.train(graphs, 1, training_mode='parallel', verbose=0)


def test_train_evaluate_train_with_a_folded_readout():
    """A small graph-based batch takes the persistent inference launch, which folds the output stage and the graph readout into itself: the step's
    outputs are published as this run's, so train -> evaluate -> train gives what two steps of a fresh model give."""
    batch = _mutag_like(seed=2, graphs=6)
    a, b = _graph_model('fixed_point'), _graph_model('fixed_point')
    from GNN.graph_class import GraphTensor
    gt = GraphTensor.fromGraphObject(batch)
    la = [a.training_step(gt, mean=True)['loss']]
    ev = a.evaluate(gt)[0]['Loss']
    out_eval = a.Loop(gt)[2]
    la.append(a.training_step(gt, mean=True)['loss'])
    lb = [b.training_step(gt, mean=True)['loss'] for _ in range(2)]
    assert la == lb and np.isfinite(ev)
    # and the other way round: the readout after a training step is that step's, not the evaluation's folded one
    k, _, out_train = a.Loop(gt, training=True)
    assert out_train.shape == out_eval.shape and not np.array_equal(out_train, out_eval)      # (two optimizer steps apart)
    assert np.array_equal(a.Loop(gt)[2], a.Loop(gt)[2])


# ---- 7. arena ---------------------------------------------------------------------------------------------------------------------------------------
def test_arena_holds_one_body_whatever_max_iter():
    pb = problem(81, n=500, ds=8, hidden=(16,), gain=3.0)       # no contraction: the forward runs max_iter bodies
    used = {}
    for mode, max_iter in ((1, 3), (1, 200), (0, 200)):
        dev = Device(pb, max_iter, 1e-3, mode=mode, adjoint_max_iter=10)
        res = dev.step()
        assert res['k'] == max_iter
        used[mode, max_iter] = dev.loop.train_arena_bytes()
        dev.close()
    assert used[1, 3] == used[1, 200] > 0
    in_s = pb['st']['weights'][0].shape[0]
    body = 4 * 500 * (in_s + 16 + 8)                            # one body's cache: concat, both Dense outputs
    assert used[0, 200] >= 200 * body and used[1, 200] <= 12 * body, (used, body)
