"""Step times and scratch of the JOINT training step of a 3-layer LGNN ('parallel' mode): the unrolled step with its host-chained label gradients,
and the fixed-point step with label gradients, chained inside the device or through host arrays (profiles/fixed_point_lgnn.txt).  Engine level, the
calls of LGNN.training_step: per layer gnn_loop_train_forward and gnn_graph_update_labels, the loss on the host (gnn_loss_grad), the backward passes
from the last layer to the first, Adam per layer on the device (gnn_loop_optimizer_step).  Host clock around a whole step, median of --steps warm
steps; arena = the sum of the layers' training scratch.  One process per run; a tree without the label gradients (the parent commit) runs
--configs unrolled.

    python tools/bench_fixed_point_lgnn.py --case c3 --max-iter 5 --configs fixed_device,fixed_host,unrolled
    python tools/bench_fixed_point_lgnn.py --case mutag --max-iter 50 --get-output 1 --configs fixed_device,fixed_host,unrolled

case c3: 1 M nodes / 10 M arcs (syntheticGraph, seed 20261003), node-based, state_dim 64, get_state: layers 1 and 2 see 3 + 64 label columns,
net_state (1 + 2 (64 + NL)) -> 128 -> 128 -> 64; case mutag: the first 32 MUTAG graphs as one batch (935 nodes), graph-based, state_dim 14,
net_state -> 32 -> 32 -> 14.  tanh nets of gain 0.5 (contractive).  Controls: --layers 1 is the single-GNN step through the same calls."""
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
ap.add_argument('--layers', type=int, default=3)
ap.add_argument('--get-state', type=int, default=1)
ap.add_argument('--get-output', type=int, default=0)
ap.add_argument('--configs', default='fixed_device,fixed_host,unrolled')
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--tree', default='this')
ap.add_argument('--cache', default=None, help='folder for the synthetic graph of case c3 (built once, reused by later runs)')
a = ap.parse_args()
rng = np.random.default_rng(20261003)
T = 2

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
    base = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    nl, al, hidden, ng, n_targets = 3, 1, [128, 128, d], None, n
else:
    import load_MUTAG
    from GNN.graph_class import GraphObject, GraphTensor
    batch = GraphTensor.fromGraphObject(GraphObject.merge(load_MUTAG.load(limit=32), problem_based='g', aggregation_mode='average'))
    base, ng = batch.device_graph(), batch.nodegraph_csr()
    dims = base.dims()
    n, nl, al, d = dims['n_rows'], dims['NL'], dims['AL'], 14
    hidden, n_targets = [32, 32, d], batch.targets.shape[0]
    ng_dense = np.asarray(batch.NodeGraph, np.float32)

L, gs, go = a.layers, bool(a.get_state), bool(a.get_output)
extra = gs * d + go * T
graphs = [base] + [base.derive(extra) for _ in range(L - 1)] if extra else [base] * L
targets = np.eye(T, dtype=np.float32)[rng.integers(0, T, n_targets)]
weights = np.full(n_targets, 1.0 / n_targets, np.float32)
ADAM = (1, [1e-4, 0.9, 0.999, 1e-7])
print(f'# case {a.case} layers {L} get_state {int(gs)} get_output {int(go)} max_iter {a.max_iter} thr {a.thr} steps {a.steps} tree {a.tree}', flush=True)
for config in a.configs.split(','):
    fixed = config.startswith('fixed')
    if config not in ('fixed_device', 'fixed_host', 'unrolled'): raise SystemExit(f'unknown configuration {config}')
    net_rng = np.random.default_rng(7)
    nets, loops = [], []
    for i in range(L):
        nl_i = nl + (i > 0) * extra
        st = make_mlp(net_rng, al + 2 * (d + nl_i), hidden, 'tanh', gain=0.5, batch_normalization=False)
        ou = make_mlp(net_rng, d + nl_i, [T], 'softmax', batch_normalization=False)
        mst, mou = e.Mlp(st['weights'], st['activations'], False), e.Mlp(ou['weights'], ou['activations'], False)
        loop = e.Loop(graphs[i], mst, mou, d, a.max_iter, a.thr)
        loop.set_state0((0.1 * np.random.default_rng(100 + i).standard_normal((n, d))).astype(np.float32))
        if fixed: loop.set_gradient_mode(1, label_gradients=True)
        nets.append((mst, mou)); loops.append(loop)

    def step():
        outs, K = [], []
        for i, loop in enumerate(loops):
            k, out = loop.train_forward(nets[i][0], nets[i][1], None)
            K.append(k)
            outs.append(loop.readout(*ng) if ng is not None else out)
            if i < L - 1 and extra: graphs[i + 1].update_labels(base, loop, gs, go)
        pairs = [e.loss_grad(0, targets, o, weights) for o in outs]
        d_outs = [p[1] / L for p in pairs]
        dse = dox = None
        for i in reversed(range(L)):
            d_nodes_out = ng_dense @ d_outs[i] if ng is not None else d_outs[i]
            chain = i > 0 and extra > 0
            if config == 'fixed_device':
                above = i < L - 1 and extra > 0
                loops[i].train_backward_chained(d_nodes_out, loops[i + 1] if above else None, above and gs, above and go, keep_label_gradients=e.KEEP_D_NODES if chain else 0)
                continue
            if dox is not None: d_nodes_out = d_nodes_out + dox
            res = loops[i].train_backward(d_nodes_out, dse, want_d_nodes=chain)
            dse = dox = None
            if chain:
                c = nl
                if gs:
                    dse = res['d_nodes'][:, c:c + d]
                    c += d
                if go: dox = res['d_nodes'][:, c:c + T]
        for loop, k in zip(loops, K):
            loop.optimizer_step(ADAM[0], ADAM[1], 1.0 if (fixed or not k) else 1.0 / k)
        return float(np.mean([p[0] for p in pairs])), K

    for _ in range(a.warmup): loss, K = step()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        loss, K = step()
        times.append(time.perf_counter() - t0)
    its = [lp.adjoint_info()['iterations'] for lp in loops] if fixed else '-'
    print(f'{a.case:6s} L{L} {a.max_iter:3d} {a.thr:<7g} {a.tree:7s} {config:14s} k {[int(k) for k in K]}  adjoint {its}  median {1e3 * float(np.median(times)):9.3f} ms  '
          f'min {1e3 * min(times):9.3f}  arena {sum(lp.train_arena_bytes() for lp in loops)}  loss {loss:.5f}', flush=True)
    for lp in loops: lp.close()
    for mst, mou in nets: mst.close(); mou.close()
