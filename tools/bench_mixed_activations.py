"""net_state with one activation for all layers against the same net whose last layer has its own, alternating in one process.

Part 1 (benchmark shape: syntheticGraph(N, 10.0, 3, 1), 135 -> 128 -> 128 -> 64, 30 bodies at threshold 0): the SELU net and ('selu', 'selu',
'tanh') with the SAME weights, on the default path (impl 2) and on impl 1; per alternation one Loop each, host clock around a Loop that ends in
a device synchronise, ms per iteration = Loop time / bodies.  Reported: the median, minimum and maximum over the alternations, the ratio of
the two nets, and the per-op path (impl 0) of the mixed net.
Part 2 (MUTAG batches of 32, 31 -> 32 -> 32 -> 14, the method of tools/bench_small.py): Loops per second of ('selu', 'selu', 'tanh') and of the
SELU net, as the library chooses (the persistent launch where the net is covered) and on the per-op path.

Every line also names the impl the loop reports, so that a library without fused kernels for the mixed net shows as impl 0.
Run on the GPU box: python tools/bench_mixed_activations.py [--nodes 1000000] [--alternations 7] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'gnn_tf_2.x_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
from GNN import _engine as e, GNN_utils as utils          # noqa: E402
from GNN.graph_class import GraphObject, GraphTensor      # noqa: E402
from util import make_mlp                                 # noqa: E402
import load_MUTAG                                         # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def sync():
    e._check(e.lib().gnn_device_synchronize(0))


def timed_loop(loop):
    sync()
    t = time.perf_counter()
    k = loop.run()
    sync()
    return 1e3 * (time.perf_counter() - t), k


def spread(v):
    return f'median {statistics.median(v):7.4f}  min {min(v):7.4f}  max {max(v):7.4f}'


def full_size(nodes, alternations, bodies=30):
    d, nl, al = 64, 3, 1
    s = utils.syntheticGraph(nodes, 10.0, nl, al, 2, seed=20261003)
    n = s['n_nodes']
    rng = np.random.default_rng(20261003)
    st = make_mlp(rng, al + 2 * (nl + d), [128, 128, d], 'selu', gain=0.6)
    ou = make_mlp(rng, nl + d, [2], 'softmax')
    mixed = dict(st, activations=['selu', 'selu', 'tanh'])
    state0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    mou = e.Mlp(ou['weights'], ou['activations'], True)
    nets = {'uniform selu': e.Mlp(st['weights'], st['activations'], True), "('selu','selu','tanh')": e.Mlp(mixed['weights'], mixed['activations'], True)}
    say(f'# benchmark shape: {n} nodes, {s["n_arcs"]} arcs, 135 -> 128 -> 128 -> 64, {bodies} bodies at threshold 0; ms per iteration over {alternations} alternations')
    for impl in (2, 1, 0):
        loops, used = {}, {}
        for name, mst in nets.items():
            lp = e.Loop(graph, mst, mou, d, bodies, 0.0)
            used[name] = lp.set_impl(impl)
            lp.set_state0(state0)
            loops[name] = lp
        reps = alternations if impl else 2                       # (the per-op path is the slow control: two alternations)
        for lp in loops.values():                                  # warm-up: code objects, weight images, label block, gather program
            lp.run(); lp.run()
        ms = {name: [] for name in loops}
        for _ in range(reps):
            for name, lp in loops.items():
                t, k = timed_loop(lp)
                assert k == bodies, (name, k)
                ms[name].append(t / k)
        for name in loops:
            say(f'impl asked {impl} used {used[name]}  {name:24s} {spread(ms[name])}  ms/iteration')
        a, b = statistics.median(ms['uniform selu']), statistics.median(ms["('selu','selu','tanh')"])
        say(f'impl asked {impl}: mixed / uniform = {b / a:.4f}')
        for lp in loops.values(): lp.close()
    graph.close()


def mutag(reps=20):
    rng = np.random.default_rng(1)
    graphs = load_MUTAG.load(limit=320)
    batches = [GraphObject.merge(graphs[i:i + 32], problem_based='g', aggregation_mode='average') for i in range(0, 320, 32)]
    st = make_mlp(rng, 31, [32, 32, 14], 'selu', gain=0.7)
    ou = make_mlp(rng, 14, [2], 'softmax')
    mixed = dict(st, activations=['selu', 'selu', 'tanh'])
    mou = e.Mlp(ou['weights'], ou['activations'], True)
    tensors = [GraphTensor.fromGraphObject(b) for b in batches]
    say(f'# MUTAG: {len(batches)} batches of 32 graphs, 31 -> 32 -> 32 -> 14, max_iteration 50, threshold 0.01; {reps} passes over the batches, three repeats')
    for name, net in (('uniform selu', st), ("('selu','selu','tanh')", mixed)):
        mst = e.Mlp(net['weights'], net['activations'], True)
        for impl in (2, 0):
            loops = [e.Loop(gt.device_graph(), mst, mou, 0, 50, 0.01) for gt in tensors]
            used = {lp.set_impl(impl) for lp in loops}
            persistent = {lp.set_persistent(True) for lp in loops}
            for lp in loops: lp.run()
            rates, iters = [], 0
            for _ in range(3):
                sync()
                t = time.perf_counter()
                iters = 0
                for _ in range(reps):
                    for lp in loops: iters += lp.run()
                sync()
                rates.append(reps * len(loops) / (time.perf_counter() - t))
            say(f'impl asked {impl} used {sorted(used)} persistent {sorted(persistent)}  {name:24s} Loops/s median {statistics.median(rates):9.1f}  '
                f'min {min(rates):9.1f}  max {max(rates):9.1f}  mean k {iters / (reps * len(loops)):.1f}')
            for lp in loops: lp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--alternations', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    say(f'# library: {e.LIB_PATH}')
    full_size(args.nodes, args.alternations)
    mutag()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
