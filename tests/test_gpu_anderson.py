"""The Anderson-accelerated adjoint solve (include/gnn_hip.h: gnn_loop_set_adjoint_solver) on the device against its mirror (tests/anderson_mirror.py).
Every loop runs through the C ABI on impl 1 (bit-exact float32 forward), as tests/test_gpu_adjoint.py.

(a) Per element, the criterion of tests/test_gpu_adjoint.py::check_tight, restated: the float64 mirror runs the device's k bodies and the device's count of
    iterations (ending as the device ended: on a closed gate, or on the mixed iterate at adjoint_max_iter); the mirror is evaluated a second time in
    float32 as the device is defined (float32 vectors and rings, Gram matrix and solve in float64); an array passes when every element lies within
    MARGIN x max |mirror_f32 - mirror_f64| over that array plus FLOOR x max |mirror_f64|.  MARGIN = 8, FLOOR = 2^-22, unchanged.  State, out, z, every gradient
    array, and the loss at 2e-5.  GNN_ANDERSON_RATIOS=<file> appends the measured ratios (profiles/anderson_adjoint.txt).
(b) z_final of the converged cases of 37 rows or fewer against the dense solve of (I - J^T) z = g: the derived bound of tests/test_anderson_host.py
    (|J^T|_2 |(I - J^T)^-1|_2 thr |z_t|_2) plus the float32 term of (a) over the vector (sqrt(size) x the per-element allowance).
(c) Iteration counts against the mirror's OWN gates: equal at threshold 1e-2, within one at 1e-4 and below; the seeds are ones on which the float32 and the
    float64 mirror agree on the count.
(d) On the rho 0.836 and rho 0.952 problems the device's Anderson count is at most half of the device's Picard count on the same loop.
(e) The same bits on a second call; a loop switched to Anderson and back returns the bits of a loop never switched; a following Loop and a following
    contraction_estimate are unchanged.
(f) adjoint_solver_info() reports solver, window, restarts; adjoint_info() keeps exactly its three keys.

Shapes: 1 row; 15 | 16 | 17 rows; 37 with an isolated node; 83 with the 70-arc hub, and a directed unsorted list; 4,113 rows = 258 blocks of partial dots, a second
run in the block-order sum.  Ds 3 and 5: the generic gather; 4, 8 and 40: the rows of two column blocks; 64 behind the three-layer wide chain: the aligned rows.
Windows 1, 3, 8.  Counts past window + 2 reuse a ring slot; 12 iterations pass two chunks of five and close inside the third."""
import os

import numpy as np
import pytest

import adjoint_bn_cases as C
import adjoint_bn_mirror as abm
import adjoint_labels_mirror as lm
import anderson_mirror as an
import test_anderson_host as ah
import test_gpu_adjoint as ga
import test_gpu_adjoint_bn as gb
import test_gpu_adjoint_labels as gl
import train_graph_cases as G
from oracle import gnn_oracle as orc
from util import make_mlp

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -22


def record(lines):
    path = os.environ.get('GNN_ANDERSON_RATIOS')
    if path:
        with open(path, 'a') as f: f.write(''.join(line + '\n' for line in lines))


def check_tight(tag, got, want, noisy):
    """Dicts name -> array (device, mirror float64, mirror float32).  Every line is printed and recorded before anything is asserted."""
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
        lines.append(f'{tag:40s} {key:18s} err {err:9.3e}  noise {noise:9.3e}  ratio {err / noise if noise > 0 else float("nan"):6.2f}  floor {FLOOR * top:9.3e}  '
                     f'max|ref| {top:9.3e}')
        if not ok: bad.append(lines[-1])
    record(lines)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)


def arrays(r):
    out = {'state': r['state'], 'out': r['out'], 'z': r['z']}
    for i, a in enumerate(r['grads_state']): out[f'grads_state[{i}]'] = a
    for i, a in enumerate(r['grads_output']): out[f'grads_output[{i}]'] = a
    return out


def directed_problem(seed, n, ds, nl=2, al=1, hidden=(7,), gain=0.5):
    """ga.problem on the directed, unsorted arc list of tests/train_graph_cases.py (hub, a node without in-arcs, one without out-arcs, an isolated one)."""
    rng = np.random.default_rng(seed)
    arcs = G.directed_graph(seed, n, degrees=True, al=al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.7
    g['set_mask'][0] = True
    st = make_mlp(rng, al + 2 * (ds + nl), list(hidden) + [ds], 'tanh', gain=gain, batch_normalization=False)
    ou = make_mlp(rng, ds + nl, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    return dict(g=g, st=st, ou=ou, ds=ds, D=ds, s0=(0.1 * rng.standard_normal((n, ds))).astype(np.float32), n=n,
                targets=np.eye(2)[rng.integers(0, 2, m)].astype(np.float32), weights=rng.uniform(0.5, 1.5, m).astype(np.float32))


class Device(gb.Device):
    """The loop of a problem in fixed-point mode with the Anderson solver (window None: the solver is never set)."""

    def __init__(self, pb, max_iter, thr, window=3, **kw):
        super().__init__(pb, max_iter, thr, frozen='frozen' if pb['st']['batch_normalization'] else None, **kw)
        if window is not None: assert self.loop.set_adjoint_solver('anderson', window) == 1

    def step(self, **kw):
        res = super().step(**kw)
        res['solver'] = self.loop.adjoint_solver_info()
        return res


def mirrors(pb, max_iter, thr, res, window, **kw):
    """The mirror with the device's counts forced and the device's ending, in float64 and float32; and with the device's k but its OWN gates, in float64 and float32."""
    args = (pb['g'], pb['st'], pb['ou'], pb['D'], max_iter, thr, pb['s0'], {}, pb['targets'], pb['weights'], window)
    forced = dict(k_forced=int(res['k']), iterations_forced=res['adjoint_iterations'], final_mix=not res['adjoint_converged'], **kw)
    want, noisy = an.step(*args, **forced), an.step(*args, dtype=np.float32, **forced)
    own, own32 = an.step(*args, k_forced=int(res['k']), **kw), an.step(*args, k_forced=int(res['k']), dtype=np.float32, **kw)
    return want, noisy, own, own32


def dense_check(tag, z_dev, want, noisy, thr):
    """(b): the device's z_final against the dense solve at the mirror's context."""
    a = ah.dense_jt(want['ctx'])
    star = np.linalg.solve(np.eye(a.shape[0]) - a, want['g'].ravel()).reshape(want['g'].shape)
    noise, top = float(np.max(np.abs(noisy['z'].astype(np.float64) - want['z']))), float(np.max(np.abs(want['z'])))
    err, bound = np.linalg.norm(z_dev.astype(np.float64) - star), ah.dense_bound(a, thr, z_dev.astype(np.float64)) + np.sqrt(star.size) * (MARGIN * noise + FLOOR * top)
    line = f'{tag:40s} dense solve        err {err:9.3e}  bound {bound:9.3e}'
    record([line]); print(line)
    assert err <= bound


# ---- (a), (b), (c), (e: same bits twice), (f) over the shapes -------------------------------------------------------------------------------------------
# name: (problem, window, loop max_iter, threshold)
CASES = {
    'n1_ds3_w8': (lambda: ga.problem(11, n=1, ds=3), 8, 50, 1e-4),
    'n15_ds4_w1': (lambda: ga.problem(11, n=15, ds=4), 1, 50, 1e-4),
    'n16_ds8_w3': (lambda: ga.problem(11, n=16, ds=8), 3, 50, 1e-6),
    'n17_ds5_w3': (lambda: ga.problem(11, n=17, ds=5), 3, 50, 1e-4),
    'n17_ds40_w8': (lambda: ga.problem(11, n=17, ds=40, hidden=(20,)), 8, 50, 1e-4),
    'n37_ds3_isolated_w3': (lambda: ga.problem(11, n=37, ds=3, isolated=True), 3, 50, 1e-2),
    'n37_ds8_rho0.836_w3': (lambda: ga.problem(3, **ah.TABLE['rho0.836']), 3, 60, 1e-4),        # 12 iterations: two chunks, closing inside the third; slots reused
    'n83_ds4_hub70_w8': (lambda: ga.problem(3, **ah.TABLE['rho0.799']), 8, 60, 1e-4),           # 16 iterations: all eight slots live, then reused
    'n83_ds5_directed_w3': (lambda: directed_problem(13, 83, 5), 3, 50, 1e-4),
    'n4113_ds64_chain3_w3': (lambda: ga.wide_problem((135, 128, 128, 64), 4113), 3, 30, 1e-2),  # the aligned rows; 258 blocks of partials
    'n4113_ds8_w5': (lambda: ga.problem(11, n=4113, ds=8, hub=70), 5, 30, 1e-2),
    'n37_ds8_frozen_bn_w3': (lambda: C.problem(19, n=37, ds=8, nl=5, al=2), 3, 50, 1e-4),
}
GATHER = {'n4113_ds64_chain3_w3': 'rows_aligned', 'n1_ds3_w8': 'generic', 'n17_ds5_w3': 'generic', 'n37_ds3_isolated_w3': 'generic', 'n83_ds5_directed_w3': 'generic'}


@pytest.mark.parametrize('case', list(CASES))
def test_against_the_mirror(case):
    make, window, max_iter, thr = CASES[case]
    pb = make()
    dev = Device(pb, max_iter, thr, window=window)
    res, again = dev.step(), dev.step()
    want, noisy, own, own32 = mirrors(pb, max_iter, thr, res, window)
    line = f'{case:40s} k {res["k"]:.0f}  iterations {res["adjoint_iterations"]}  mirror {own["adjoint_iterations"]} / float32 {own32["adjoint_iterations"]}  restarts {res["solver"]["restarts"]}'
    record([line]); print(line)
    # (f) both reports; the narrow one-launch form is never taken with the solver on
    assert res['info'] == dict(iterations=res['adjoint_iterations'], converged=True, gather=GATHER.get(case, 'rows'))
    assert res['solver'] == dict(solver='anderson', window=window, restarts=own['restarts']) and own['restarts'] == 0
    # (c)
    assert own['adjoint_converged'] and own32['adjoint_iterations'] == own['adjoint_iterations']          # (the seed is one the two mirrors agree on)
    assert abs(res['adjoint_iterations'] - own['adjoint_iterations']) <= (0 if thr >= 1e-2 else 1), (res['adjoint_iterations'], own['adjoint_iterations'])
    if pb['n'] > 1: assert res['k'] >= 2 and res['adjoint_iterations'] >= 3
    # (a)
    check_tight(case, arrays(res), arrays(want), arrays(noisy))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    # (b)
    if pb['n'] <= 37: dense_check(case, res['z'], want, noisy, thr)
    # (e)
    for key, a in arrays(res).items(): assert np.array_equal(a, arrays(again)[key]), key
    assert again['loss'] == res['loss'] and again['info'] == res['info'] and again['solver'] == res['solver']
    dev.close()


def test_chunks_and_ring_reuse_are_exercised():
    """What the table above promises of its counts, on the device: a count past window + 2, and one that passes two chunks of five and closes inside the third."""
    make, window, max_iter, thr = CASES['n37_ds8_rho0.836_w3']
    dev = Device(make(), max_iter, thr, window=window)
    it = dev.step()['adjoint_iterations']
    assert 10 < it < 15 and it > window + 2, it
    # the same count when the first look comes behind the count of the step before, plus one (adjoint_backward's hint)
    assert dev.step()['adjoint_iterations'] == it
    dev.close()


# ---- the count reaching adjoint_max_iter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t_max,window', [(7, 3), (5, 1), (1, 5), (2, 8)])
def test_truncated_solve(t_max, window):
    """rho 0.969: the solve stops at adjoint_max_iter (7: inside the second chunk; 5: at the end of the first; 1: the iteration without history; 2), reports
    it, and returns the mixed iterate with its weight gradients."""
    pb = ga.problem(3, **ah.TABLE['rho0.969'])
    dev = Device(pb, 40, 1e-4, window=window, adjoint_max_iter=t_max)
    res = dev.step()
    assert res['adjoint_iterations'] == t_max and res['adjoint_converged'] is False and res['info']['converged'] is False
    want, noisy, own, _ = mirrors(pb, 40, 1e-4, res, window, adjoint_max_iter=t_max)
    assert own['adjoint_iterations'] == t_max and not own['adjoint_converged']
    check_tight(f'truncated at {t_max} window {window}', arrays(res), arrays(want), arrays(noisy))
    dev.close()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rho0.836', 'rho0.952'])
def test_half_of_picards_iterations(name):
    pb = ga.problem(3, **ah.TABLE[name])
    dev = Device(pb, 400, ah.THR, window=None)
    picard = dev.step()
    assert picard['solver'] == dict(solver='picard', window=5, restarts=0)
    dev.loop.set_adjoint_solver('anderson', 5)
    anderson = dev.step()
    line = f'{name:40s} device iterations: Picard {picard["adjoint_iterations"]}, Anderson window 5 {anderson["adjoint_iterations"]}'
    record([line]); print(line)
    assert picard['adjoint_converged'] and anderson['adjoint_converged'] and picard['k'] == anderson['k']
    assert 2 * anderson['adjoint_iterations'] <= picard['adjoint_iterations']
    # both solve the same system: z agrees to what the two closed gates leave (the derived bound of the dense solve, once per solver)
    want = an.step(pb['g'], pb['st'], pb['ou'], pb['D'], 400, ah.THR, pb['s0'], {}, pb['targets'], pb['weights'], 5, k_forced=int(picard['k']))
    a = ah.dense_jt(want['ctx'])
    assert np.linalg.norm(anderson['z'].astype(np.float64) - picard['z']) <= ah.dense_bound(a, ah.THR, anderson['z']) + ah.dense_bound(a, ah.THR, picard['z'])
    dev.close()


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------------------
def test_switching_back_to_picard_and_what_follows():
    pb = ga.problem(21, n=37, ds=8)
    never = Device(pb, 50, 1e-2, window=None)
    base = never.step()
    k_inf = never.loop.run()
    state_inf, out_inf = never.loop.state(), never.loop.output()
    est = never.loop.contraction_estimate(never.mst, iterations=6, seed=1)
    vec = never.loop.contraction_vector()
    never.close()
    dev = Device(pb, 50, 1e-2, window=3)
    mixed = dev.step()
    assert mixed['solver']['solver'] == 'anderson' and not np.array_equal(mixed['z'], base['z'])
    # a following Loop and a following contraction estimate are what they are without the solver
    assert dev.loop.run() == k_inf and np.array_equal(dev.loop.state(), state_inf) and np.array_equal(dev.loop.output(), out_inf)
    est_b = dev.loop.contraction_estimate(dev.mst, iterations=6, seed=1)
    assert np.array_equal(est_b['growth'], est['growth']) and est_b['k'] == est['k'] and np.array_equal(dev.loop.contraction_vector(), vec)
    assert dev.loop.set_adjoint_solver('picard') == 0
    back = dev.step()
    assert back['solver'] == dict(solver='picard', window=5, restarts=0) and back['info'] == base['info'] and back['loss'] == base['loss']
    assert set(back['info']) == {'iterations', 'converged', 'gather'}
    for key, a in arrays(base).items(): assert np.array_equal(a, arrays(back)[key]), key
    assert dev.loop.train_arena_bytes() > 0
    dev.close()


def test_refusals_of_the_c_call():
    import ctypes as ct
    from GNN import _engine as e
    dev = Device(ga.problem(21, n=20, ds=4), 10, 1e-2, window=None)
    used = ct.c_int(-1)
    for solver, window in ((1, 0), (1, 9), (2, 5), (-1, 5), (0, 0)):
        assert e.lib().gnn_loop_set_adjoint_solver(dev.loop._h, solver, window, ct.byref(used)) == -1          # GNN_ERR_ARG
    assert used.value == -1 and dev.loop.adjoint_solver_info() == dict(solver='picard', window=5, restarts=0)
    with pytest.raises(ValueError): dev.loop.set_adjoint_solver('gmres')
    with pytest.raises(ValueError): dev.loop.set_adjoint_solver('anderson', 9)
    assert e.lib().gnn_loop_set_adjoint_solver(dev.loop._h, 1, 8, None) == 0 and dev.loop.adjoint_solver_info()['window'] == 8
    dev.close()


# ---- label gradients, the model classes, the LGNN device chain -------------------------------------------------------------------------------------------
def anderson_adjoint(window):
    """abm.adjoint's signature over the Anderson mirror: what tests/adjoint_labels_mirror.py calls for z (the label terms behind it are its own)."""
    def solve(ctx, g_state, max_iter, threshold, iterations_forced=None):
        z, it, conv, _, grads = an.anderson(ctx, g_state, max_iter, threshold, window, iterations_forced)
        return z, it, conv, grads
    return solve


@pytest.mark.parametrize('case', ['n37_directed', 'edge37'])
def test_label_gradients(case, monkeypatch):
    """label_gradients=True: d_nodes (edge-based: and d_arc_labels) are the label columns of the weight-gradient pass with the solver's z_final."""
    monkeypatch.setattr(abm, 'adjoint', anderson_adjoint(3))
    pb = gl.CASES[case]()
    d_out, dse = gl.incoming(pb, 5, True)
    dev = gl.Device(pb, gl.MAX_ITER, 1e-4)
    dev.loop.set_adjoint_solver('anderson', 3)
    res, again = dev.halves(d_out, dse), dev.halves(d_out, dse)
    assert res['info']['converged'] and res['info']['iterations'] >= 3 and dev.loop.adjoint_solver_info() == dict(solver='anderson', window=3, restarts=0)
    want, noisy = gl.mirror_halves(pb, gl.MAX_ITER, 1e-4, d_out, dse, int(res['k']), res['info']['iterations'])
    own = lm.halves(pb['g'], pb['st'], pb['ou'], pb['D'], gl.MAX_ITER, 1e-4, pb['s0'], {}, d_out, dse, edge_based=bool(pb.get('edge')), k_forced=int(res['k']))
    assert abs(own['adjoint_iterations'] - res['info']['iterations']) <= 1
    assert np.abs(want['d_nodes']).max() > 1e-3
    check_tight(f'labels {case}', res['arrays'], want, noisy)
    gl.same_bits(res['arrays'], again['arrays'])
    dev.close()


@pytest.mark.parametrize('kind', ['g'])
def test_graph_based_model(kind):
    """training_step of GNNgraphBased (NodeGraph readout over a batch of 32) with adjoint_solver='anderson': the raw gradients against the mirror.  (The edge-based
    case of this file is test_label_gradients[edge37], at the C level.  GNNedgeBased with Dropout and BatchNormalization in net_output is not held to this
    criterion here: its net_output gradients, which no adjoint solve enters, measured 9.5 to 14.2 times the float32 noise of the mirror with this very check;
    tests/test_gpu_adjoint.py holds that model path to 1e-3 of the largest entry.)"""
    t = ga._typed(kind, device_optimizer=False)
    t['gnn'].set_gradient_mode('fixed_point', threshold=1e-4, adjoint_solver='anderson', anderson_window=3)
    mo_flat = t['mo'][1].astype(np.uint8).ravel()
    res = t['gnn'].training_step(t['batch'], mean=True, state0=t['s0'], masks_output=mo_flat)
    kw = dict(graph_based=kind == 'g', edge_based=kind == 'a', adjoint_threshold=1e-4, k_forced=int(res['k']))
    args = (t['g'], t['st'], t['ou'], t['ds'], 30, 1e-3, t['s0'], t['mo'], t['targets'], t['weights'], 3)
    want, noisy = (an.step(*args, iterations_forced=res['adjoint_iterations'], dtype=dt, **kw) for dt in (np.float64, np.float32))
    own = an.step(*args, **kw)
    assert res['k'] >= 2 and res['adjoint_converged'] and abs(res['adjoint_iterations'] - own['adjoint_iterations']) <= 1 and res['adjoint_iterations'] >= 3
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    pick = lambda r: {**{f'grads_state[{i}]': a for i, a in enumerate(r['grads_state'])}, **{f'grads_output[{i}]': a for i, a in enumerate(r['grads_output'])}}
    check_tight(f'model {kind}', pick(res), pick(want), pick(noisy))
    # the Picard model on the same batch: another count, gradients that agree to the threshold and not bit for bit
    p = ga._typed(kind, device_optimizer=False)
    p['gnn'].set_gradient_mode('fixed_point', threshold=1e-4)
    ref = p['gnn'].training_step(p['batch'], mean=True, state0=p['s0'], masks_output=mo_flat)
    assert ref['adjoint_converged'] and ref['adjoint_iterations'] >= res['adjoint_iterations']
    for a, b in zip(res['grads_state'], ref['grads_state']):
        assert not np.array_equal(a, b) and np.max(np.abs(a - b)) <= 1e-2 * max(1e-3, np.max(np.abs(b)))


def test_lgnn_parallel_joint_step_on_the_device_chain(monkeypatch):
    monkeypatch.setattr(abm, 'adjoint', anderson_adjoint(3))
    s = gl.stack('n', True, True, 3, 'parallel')
    s['lgnn'].set_gradient_mode('fixed_point', label_gradients=True, adjoint_solver='anderson', anderson_window=3)
    for gnn in s['lgnn'].gnns: assert (gnn.adjoint_solver, gnn.anderson_window, gnn.adjoint_label_gradients) == ('anderson', 3, True)
    assert s['lgnn'].device_chain is True
    res = gl.joint_step(s)
    assert min(res['k']) >= 2 and all(res['adjoint_converged']) and min(res['adjoint_iterations']) >= 2, (res['k'], res['adjoint_iterations'])
    want, noisy = (gl.joint_mirror(s, res, True, True, 'parallel', dt) for dt in (np.float64, np.float32))
    assert abs(res['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss']))
    check_tight('lgnn n parallel s1 o1', gl.joint_arrays(res), gl.joint_arrays(want), gl.joint_arrays(noisy))
    host = gl.stack('n', True, True, 3, 'parallel', device_chain=False)
    host['lgnn'].set_gradient_mode('fixed_point', label_gradients=True, adjoint_solver='anderson', anderson_window=3)
    res_h = gl.joint_step(host)
    gl.same_bits(gl.joint_arrays(res), gl.joint_arrays(res_h))
    assert res_h['adjoint_iterations'] == res['adjoint_iterations']
