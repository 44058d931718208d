"""Latency of small-graph Loops with a wide net_state: MUTAG batches of 32 graphs with net_state 31 -> 64 -> 64 -> 14 (max_iteration 50,
threshold 0.01), and the BASELINE net 31 -> 32 -> 32 -> 14 as the control.  For each net: Loops/s with the persistent launch allowed
(the library's choice) and with set_persistent(False) (one launch per body), impl 1, warm runs.  One line per (net, setting); --label
names the build in the line (A/B runs alternate two checkouts).  Run on the GPU box: python tools/bench_small_wide.py [--reps 300]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'gnn_tf_2.x_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
from GNN import _engine as e                              # noqa: E402
from GNN.graph_class import GraphObject, GraphTensor      # noqa: E402
from util import make_mlp                                 # noqa: E402
import load_MUTAG                                         # noqa: E402


def run(label, name, batches, st, ou, reps):
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    for allow in (True, False):
        loops = []
        for b in batches:
            loop = e.Loop(GraphTensor.fromGraphObject(b).device_graph(), mst, mou, 0, 50, 0.01)
            loop.set_impl(1)
            loops.append(loop)
        used = {loop.set_persistent(allow) for loop in loops}
        for _ in range(3):
            ks = [loop.run() for loop in loops]           # warm: code objects, weight images, label aggregates
        t = time.perf_counter()
        for _ in range(reps):
            for loop in loops:
                loop.run()                                # (ends in a stream synchronisation: k comes back through pinned memory)
        dt = time.perf_counter() - t
        n = reps * len(loops)
        print(f'{label} {name:6s} persistent={"yes" if used == {True} else "no " if used == {False} else "mixed"} loops/s={n / dt:9.1f} '
              f'us/loop={1e6 * dt / n:8.2f} us/body={1e6 * dt / (reps * sum(ks)):7.2f} mean_k={sum(ks) / len(ks):.1f}', flush=True)
        for loop in loops: loop.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--label', default='this')
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    graphs = load_MUTAG.load(limit=320)
    batches = [GraphObject.merge(graphs[i:i + 32], problem_based='g', aggregation_mode='average') for i in range(0, 320, 32)]
    ou = make_mlp(rng, 14, [2], 'softmax')
    run(a.label, 'wide64', batches, make_mlp(rng, 31, [64, 64, 14], 'selu', gain=0.7), ou, a.reps)
    run(a.label, 'net32', batches, make_mlp(rng, 31, [32, 32, 14], 'selu', gain=0.7), ou, a.reps)


if __name__ == '__main__':
    main()
