"""Step times and scratch of the training step on nets whose net_state ends in BatchNormalization: the unrolled step, the unrolled step with
set_train_recompute, and the fixed-point step on frozen BatchNormalization (profiles/fixed_point_frozen_bn.txt).  Engine level: gnn_loop_train_step with
Adam armed on the device, host clock around a call that ends in a stream synchronisation, median of --steps warm steps.  One process per run; a
tree without the frozen mode (the parent commit) runs the configurations it has.

    python tools/bench_fixed_point_bn.py --case c3 --max-iter 5 --configs unrolled,recompute,frozen
    python tools/bench_fixed_point_bn.py --case mutag --max-iter 50 --configs unrolled,frozen,frozen_chain,plain_fixed_point

case c3: 1 M nodes / 10 M arcs (syntheticGraph, seed 20261003), state_dim 64, net_state 135 -> 128 -> 128 -> 64; case mutag: the first 32 MUTAG
graphs as one batch (935 nodes), net_state 31 -> 32 -> 32 -> 14, state_dim 0.  --act tanh with --gain 0.5 is a contractive net; --act selu with
--gain 1 is what bench.py builds.  plain_* configurations run the same net WITHOUT BatchNormalization (the controls of the existing modes)."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'gnn_tf_2.x_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
from GNN import _engine as e, GNN_utils as utils
from util import make_mlp

ap = argparse.ArgumentParser()
ap.add_argument('--case', choices=['c3', 'mutag'], default='mutag')
ap.add_argument('--max-iter', type=int, default=10)
ap.add_argument('--thr', type=float, default=0.0)
ap.add_argument('--configs', default='unrolled,recompute,frozen')
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--act', default='tanh')
ap.add_argument('--gain', type=float, default=0.5)
ap.add_argument('--tree', default='this')
ap.add_argument('--cache', default=None, help='folder for the synthetic graph of case c3 (built once, reused by later runs)')
a = ap.parse_args()
rng = np.random.default_rng(20261003)

if a.case == 'c3':
    d, D = 64, 64
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
    dims_in, hidden, ng = 1 + 2 * (3 + d), [128, 128, d], None
    n_out_in, n_targets = 3 + d, n
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
else:
    import load_MUTAG
    from GNN.graph_class import GraphObject, GraphTensor
    batch = GraphTensor.fromGraphObject(GraphObject.merge(load_MUTAG.load(limit=32), problem_based='g', aggregation_mode='average'))
    graph, ng = batch.device_graph(), batch.nodegraph_csr()
    d, D = 14, 0
    dims_in, hidden = 31, [32, 32, 14]
    n_out_in, n_targets, s0 = 14, batch.targets.shape[0], None

targets = np.eye(2, dtype=np.float32)[rng.integers(0, 2, n_targets)]
weights = np.full(n_targets, 1.0 / n_targets, np.float32)
print(f'# case {a.case} act {a.act} gain {a.gain} max_iter {a.max_iter} thr {a.thr} steps {a.steps} tree {a.tree}', flush=True)
for config in a.configs.split(','):
    bn = not config.startswith('plain_')
    net_rng = np.random.default_rng(7)                       # the same Dense weights for every configuration
    st = make_mlp(net_rng, dims_in, hidden, a.act, gain=a.gain, batch_normalization=bn, bn_random=True)
    ou = make_mlp(np.random.default_rng(8), n_out_in, [2], 'softmax', batch_normalization=False)
    mst, mou = e.Mlp(st['weights'], st['activations'], bn), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, D, a.max_iter, a.thr)
    if s0 is not None: loop.set_state0(s0)
    kind = config[6:] if not bn else config
    if kind == 'recompute': loop.set_train_recompute(True)
    elif kind in ('frozen', 'frozen_chain'): loop.set_gradient_mode(1 if kind == 'frozen' else 2, batch_normalization='frozen')
    elif kind in ('fixed_point', 'fixed_point_chain'): loop.set_gradient_mode(1 if kind == 'fixed_point' else 2)
    elif kind != 'unrolled': raise SystemExit(f'unknown configuration {config}')

    def step():
        loop.arm_optimizer(1, [1e-4, 0.9, 0.999, 1e-7], True)
        return loop.train_step(mst, mou, None, targets, weights, 0, ng)

    for _ in range(a.warmup): r = step()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        r = step()
        times.append(time.perf_counter() - t0)
    info = loop.adjoint_info() if 'adjoint_iterations' in r else dict(gather='-')
    print(f'{a.case:6s} {a.max_iter:3d} {a.thr:<7g} {a.tree:7s} {config:22s} k {int(r["k"]):3d}  adjoint {str(r.get("adjoint_iterations")):>4s} converged {str(r.get("adjoint_converged")):5s} '
          f'{info["gather"]:12s} median {1e3 * float(np.median(times)):9.3f} ms  min {1e3 * min(times):9.3f}  arena {loop.train_arena_bytes()}  loss {r["loss"]:.5f}', flush=True)
    loop.close(); mst.close(); mou.close()
