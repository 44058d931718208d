"""Time per iteration of the contraction estimate (Loop.contraction_estimate) against the time per adjoint iteration of the SAME build and loop, and the
estimate itself on the nets the project measures with (profiles/contraction_estimate.txt).  Engine level, host clock around calls that end in a wait
for the device.  Both per-iteration times are differences: (median of calls with --hi iterations - median of calls with --lo iterations) / (hi - lo) -
for the estimate its `iterations`, for the adjoint the cap of a fixed-point step in mode 2 (the per-kernel chain the estimate takes) at threshold 0,
where the iteration always runs to its cap.  The four kinds of call take turns, --reps warm calls each, over --rounds rounds; what is printed per
round is what the round-to-round spread is read from.  A tree without the estimate (the parent commit: --package <its gnn_tf_2.x_amd>) runs the adjoint
half alone, which shows the adjoint iteration unmoved.

    python tools/bench_contraction.py --case c3 --act tanh --gain 0.5
    python tools/bench_contraction.py --case c3 --act selu --gain 1 --bn            (what bench.py builds: rho above 1)
    python tools/bench_contraction.py --case mutag

case c3: 1 M nodes / 10 M arcs (syntheticGraph, seed 20261003), state_dim 64, net_state 135 -> 128 -> 128 -> 64; case mutag: the first 32 MUTAG graphs as
one batch (935 nodes), state_dim 14, net_state (AL + 2 (NL + 14)) -> 32 -> 32 -> 14."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--case', choices=['c3', 'mutag'], default='mutag')
ap.add_argument('--max-iter', type=int, default=5)
ap.add_argument('--thr', type=float, default=0.0)
ap.add_argument('--act', default='tanh')
ap.add_argument('--gain', type=float, default=0.5)
ap.add_argument('--bn', action='store_true', help='net_state ends in BatchNormalization (Keras defaults), frozen in the adjoint steps')
ap.add_argument('--lo', type=int, default=4)
ap.add_argument('--hi', type=int, default=12)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--rho-iterations', type=int, default=32)
ap.add_argument('--adjoint-only', action='store_true', help='the adjoint half alone, as a tree without the estimate runs it (the like-for-like control of such a tree)')
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
has_estimate = hasattr(e.Loop, 'contraction_estimate') and not a.adjoint_only
print(f'# case {a.case} rows {n} act {a.act} gain {a.gain} bn {a.bn} max_iter {a.max_iter} thr {a.thr} lo {a.lo} hi {a.hi} reps {a.reps} tree {a.tree} estimate {has_estimate}', flush=True)


def adjoint_step(cap):
    loop.set_gradient_mode(2, cap, 0.0, batch_normalization='frozen' if a.bn else None)
    r = loop.train_step(mst, mou, None, targets, weights, 0, ng)
    assert r['adjoint_iterations'] == cap, r['adjoint_iterations']
    return r


def estimate(m):
    return loop.contraction_estimate(mst, iterations=m, seed=1)


kinds = [('adjoint', adjoint_step)] + ([('estimate', estimate)] if has_estimate else [])
for _ in range(a.warmup):
    for _, f in kinds:
        for m in (a.lo, a.hi): f(m)
per_iter = {name: [] for name, _ in kinds}
for rnd in range(a.rounds):
    med = {}
    for name, f in kinds:                                    # in turns: adjoint lo, adjoint hi, estimate lo, estimate hi
        for m in (a.lo, a.hi):
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f(m)
                times.append(time.perf_counter() - t0)
            med[name, m] = float(np.median(times))
    for name, _ in kinds:
        per_iter[name].append((med[name, a.hi] - med[name, a.lo]) / (a.hi - a.lo))
        print(f'{a.case:6s} {a.tree:7s} round {rnd}  {name:9s} call({a.lo}) {1e3 * med[name, a.lo]:9.3f} ms  call({a.hi}) {1e3 * med[name, a.hi]:9.3f} ms  per iteration {1e3 * per_iter[name][-1]:8.4f} ms', flush=True)
for name, _ in kinds:
    v = 1e3 * np.asarray(per_iter[name])
    print(f'{a.case:6s} {a.tree:7s} {name:9s} per iteration: median {np.median(v):8.4f} ms  min {v.min():8.4f}  max {v.max():8.4f}  (rounds {a.rounds})', flush=True)
if has_estimate:
    r = estimate(a.rho_iterations)
    print(f'{a.case:6s} {a.tree:7s} rho {r["rho"]:.5f} contractive {r["contractive"]} k {int(r["k"])} done {r["done"]} last {r["last"]:.5f}  growth[:4] {np.round(r["growth"][:4], 5).tolist()} '
          f'growth[-4:] {np.round(r["growth"][-4:], 5).tolist()}', flush=True)
    loop.set_gradient_mode(2, 30, 1e-4, batch_normalization='frozen' if a.bn else None)
    r2 = loop.train_step(mst, mou, None, targets, weights, 0, ng)
    print(f'{a.case:6s} {a.tree:7s} a fixed-point step of the same loop, cap 30, threshold 1e-4: adjoint_iterations {r2["adjoint_iterations"]} adjoint_converged {r2["adjoint_converged"]}', flush=True)
loop.close(); mst.close(); mou.close()
