"""The two solvers of the adjoint system of the fixed-point gradient (Loop.set_adjoint_solver: 'picard', and 'anderson' at windows 3, 5, 8) on the SAME build
and loop (profiles/anderson_adjoint.txt).  Engine level, host clock around steps that end in a wait for the device.

Per-iteration time: a difference of whole steps, (median of steps capped at --hi iterations - median of steps capped at --lo) / (hi - lo), in mode 2 (the
per-kernel chain both solvers take) at adjoint threshold 0, where the iteration runs to its cap.  Whole steps: the loop's own --max-iter bodies at most, the
adjoint capped at --cap with threshold --adjoint-thr; medians of --reps warm steps, their iteration counts, converged, restarts, and the peak of the step's
scratch.  The solvers take turns inside every round, over --rounds rounds; what is printed per round is what the round-to-round spread is read from.  A tree
without the solver (the parent commit: --package <its gnn_tf_2.x_amd>) runs the Picard half alone: the control that shows the plain iteration unmoved.

    python tools/bench_anderson.py --case c3 --act tanh --gain 0.5                    (rho 0.14)
    python tools/bench_anderson.py --case c3 --act tanh --gain 1.4                    (a higher gain: look at the rho line it prints)
    python tools/bench_anderson.py --case mutag --act selu --gain 1 --bn              (the rho 0.941 model of profiles/contraction_estimate.txt)

case c3: 1 M nodes / 10 M arcs (syntheticGraph, seed 20261003), state_dim 64, net_state 135 -> 128 -> 128 -> 64; case mutag: the first 32 MUTAG graphs as
one batch (935 nodes), state_dim 14, net_state (AL + 2 (NL + 14)) -> 32 -> 32 -> 14."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--case', choices=['c3', 'mutag'], default='mutag')
ap.add_argument('--max-iter', type=int, default=30)
ap.add_argument('--thr', type=float, default=1e-3)
ap.add_argument('--act', default='tanh')
ap.add_argument('--gain', type=float, default=0.5)
ap.add_argument('--bn', action='store_true', help='net_state ends in BatchNormalization (Keras defaults), frozen in the adjoint steps')
ap.add_argument('--lo', type=int, default=4)
ap.add_argument('--hi', type=int, default=12)
ap.add_argument('--cap', type=int, default=30)
ap.add_argument('--adjoint-thr', type=float, default=1e-4)
ap.add_argument('--windows', type=int, nargs='*', default=[3, 5, 8])
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--warmup', type=int, default=1)
ap.add_argument('--tree', default='this')
ap.add_argument('--package', default=os.path.join(ROOT, 'gnn_tf_2.x_amd'), help="the gnn_tf_2.x_amd folder of the tree to measure (default: this tree's)")
ap.add_argument('--cache', default=None, help='folder for the synthetic graph of case c3 (built once, reused by later runs)')
a = ap.parse_args()
for p in (os.path.join(ROOT, 'tests'), a.package):
    sys.path.insert(0, p)
from GNN import _engine as e, GNN_utils as utils
from util import make_mlp

rng = np.random.default_rng(20261003)
if a.case == 'c3':
    d = 64
    path = os.path.join(a.cache, 'c3_graph.npz') if a.cache else None
    if path and os.path.exists(path):
        s = dict(np.load(path))
    else:
        s = utils.syntheticGraph(1_000_000, 10, 3, 1, 2, seed=20261003)
        s = {k: v for k, v in s.items() if isinstance(v, np.ndarray)} | {'n_nodes': np.int64(s['n_nodes'])}
        if path:
            os.makedirs(a.cache, exist_ok=True)
            np.savez(path, **s)
    n = int(s['n_nodes'])
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    dims_in, hidden, ng, n_out_in, n_targets = 1 + 2 * (3 + d), [128, 128, d], None, 3 + d, n
else:
    import load_MUTAG
    from GNN.graph_class import GraphObject, GraphTensor
    batch = GraphTensor.fromGraphObject(GraphObject.merge(load_MUTAG.load(limit=32), problem_based='g', aggregation_mode='average'))
    graph, ng = batch.device_graph(), batch.nodegraph_csr()
    d, gd = 14, graph.dims()
    n = gd['n_rows']
    dims_in, hidden, n_out_in, n_targets = gd['AL'] + 2 * (gd['NL'] + d), [32, 32, d], gd['NL'] + d, batch.targets.shape[0]

s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
targets = np.eye(2, dtype=np.float32)[rng.integers(0, 2, n_targets)]
weights = np.full(n_targets, 1.0 / n_targets, np.float32)
st = make_mlp(np.random.default_rng(7), dims_in, hidden, a.act, gain=a.gain, batch_normalization=a.bn)
ou = make_mlp(np.random.default_rng(8), n_out_in, [2], 'softmax', batch_normalization=False)
mst, mou = e.Mlp(st['weights'], st['activations'], a.bn), e.Mlp(ou['weights'], ou['activations'], False)
loop = e.Loop(graph, mst, mou, d, a.max_iter, a.thr)
loop.set_state0(s0)
has_solver = hasattr(e.Loop, 'set_adjoint_solver')
solvers = [('picard', 5)] + ([('anderson', m) for m in a.windows] if has_solver else [])
print(f'# case {a.case} rows {n} act {a.act} gain {a.gain} bn {a.bn} max_iter {a.max_iter} thr {a.thr} lo {a.lo} hi {a.hi} cap {a.cap} adjoint_thr {a.adjoint_thr} '
      f'reps {a.reps} tree {a.tree} solver {has_solver}', flush=True)
if hasattr(e.Loop, 'contraction_estimate'):
    r = loop.contraction_estimate(mst, iterations=32, seed=1)
    print(f'{a.case:6s} {a.tree:7s} rho {r["rho"]:.5f} contractive {r["contractive"]} k {int(r["k"])}', flush=True)


def step(solver, window, cap, thr):
    loop.set_gradient_mode(2, cap, thr, batch_normalization='frozen' if a.bn else None)
    if has_solver: loop.set_adjoint_solver(solver, window)
    r = loop.train_step(mst, mou, None, targets, weights, 0, ng)
    if has_solver: r['restarts'] = loop.adjoint_solver_info()['restarts']
    return r


def timed(solver, window, cap, thr):
    times, r = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = step(solver, window, cap, thr)
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), r


label = lambda solver, window: 'picard' if solver == 'picard' else f'anderson{window}'
for _ in range(a.warmup):
    for solver, window in solvers:
        for cap, thr in ((a.lo, 0.0), (a.hi, 0.0), (a.cap, a.adjoint_thr)): step(solver, window, cap, thr)
per_iter, whole = {label(*sv): [] for sv in solvers}, {label(*sv): [] for sv in solvers}
for rnd in range(a.rounds):
    for solver, window in solvers:                              # in turns: every solver's lo, hi and whole step inside every round
        name = label(solver, window)
        lo, r_lo = timed(solver, window, a.lo, 0.0)
        hi, r_hi = timed(solver, window, a.hi, 0.0)
        assert r_lo['adjoint_iterations'] == a.lo and r_hi['adjoint_iterations'] == a.hi, (r_lo['adjoint_iterations'], r_hi['adjoint_iterations'])
        full, r = timed(solver, window, a.cap, a.adjoint_thr)
        per_iter[name].append((hi - lo) / (a.hi - a.lo))
        whole[name].append(full)
        print(f'{a.case:6s} {a.tree:7s} round {rnd}  {name:10s} step({a.lo}) {1e3 * lo:9.3f} ms  step({a.hi}) {1e3 * hi:9.3f} ms  per iteration {1e3 * per_iter[name][-1]:8.4f} ms   '
              f'whole step {1e3 * full:9.3f} ms  k {int(r["k"])}  iterations {r["adjoint_iterations"]}  converged {r["adjoint_converged"]}  restarts {r.get("restarts", 0)}  '
              f'scratch {loop.train_arena_bytes() / 2 ** 30:.3f} GiB', flush=True)
for solver, window in solvers:
    name = label(solver, window)
    v, w = 1e3 * np.asarray(per_iter[name]), 1e3 * np.asarray(whole[name])
    print(f'{a.case:6s} {a.tree:7s} {name:10s} per iteration: median {np.median(v):8.4f} ms  min {v.min():8.4f}  max {v.max():8.4f}   whole step: median {np.median(w):9.3f} ms  '
          f'min {w.min():9.3f}  max {w.max():9.3f}  (rounds {a.rounds})', flush=True)
loop.close(); mst.close(); mou.close()
