"""Label projection (Loop.set_label_projection) against what a wide-label Loop runs without it, alternating in one process.

Shapes (syntheticGraph(N, 10.0, NL, AL), state width 64, net_state concat -> 128 -> 128 -> 64 SELU, 30 bodies at threshold 0):
  mutag-widths  the benchmark graph with NL = 14, AL = 3 (concat 159: past the fused kernels' LDS tile);
  wide-128      a quarter of it with NL = 128, AL = 1 (concat 385);
  narrow        the unchanged benchmark shape NL = 3, AL = 1 (concat 135, covered as it stands): the yardstick for what the seed costs.
Per alternation one warm Loop of every form, host clock around a Loop that ends in a device synchronise; reported: median / min / max of
ms per body and ms per Loop, and ms of a Loop whose label caches were dropped first (label block + projection rebuilt) minus a warm one.
Forms: 'off' (mode 0: the per-op kernels on the wide shapes, the unseeded fused kernel on the narrow one), 'auto' / 'always' (seeded).
--parent: the library under GNN_HIP_LIBRARY is one without the projection (the parent commit's, tools/ab_build.sh): its wide shapes only,
on what impl 2 falls back to there.
Run on the GPU box: python tools/bench_label_projection.py [--nodes 1000000] [--alternations 5] [--out FILE] [--parent]"""
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
from util import make_mlp                                 # noqa: E402

LINES = []
BODIES, D = 30, 64


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
    return f'median {statistics.median(v):8.4f}  min {min(v):8.4f}  max {max(v):8.4f}'


def shape(name, nodes, nl, al, forms, alternations, parent):
    s = utils.syntheticGraph(nodes, 10.0, nl, al, 2, seed=20261020)
    n = s['n_nodes']
    rng = np.random.default_rng(20261020)
    st = make_mlp(rng, al + 2 * (nl + D), [128, 128, D], 'selu')        # (gain 1, as bench.py: the map is no contraction, every gate of the 30 bodies sees robust movers)
    ou = make_mlp(rng, nl + D, [2], 'softmax')
    state0 = (0.1 * rng.standard_normal((n, D))).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    iw, h1 = 2 * nl + al, 128
    say(f'# {name}: {n} nodes, {s["n_arcs"]} arcs, NL {nl}, AL {al}, net_state {al + 2 * (nl + D)} -> 128 -> 128 -> {D}, {BODIES} bodies at threshold 0, {alternations} alternations')
    loops, used = {}, {}
    for form in forms:
        lp = e.Loop(graph, mst, mou, D, BODIES, 0.0)
        lp.set_state0(state0)
        seeded = False if parent else lp.set_label_projection(form)
        used[form] = (lp.set_impl(2), lp.body_kernel(), seeded)
        loops[form] = lp
    for lp in loops.values():                                      # warm-up: code objects, weight images, label block, projection, gather program
        lp.run(); lp.run()
    ms, cold = {f: [] for f in loops}, {f: [] for f in loops}
    for _ in range(alternations):
        for form, lp in loops.items():
            t, k = timed_loop(lp)
            assert k == BODIES, (form, k)
            ms[form].append(t)
        for form, lp in loops.items():
            lp.drop_cached_aggregates()
            t, k = timed_loop(lp)
            cold[form].append(t)
    for form, lp in loops.items():
        impl, kernel, seeded = used[form]
        say(f'{name:13s} {form:7s} impl used {impl} body kernel {kernel} seeded {int(seeded)}  ms/body {spread([t / BODIES for t in ms[form]])}   ms/Loop {spread(ms[form])}   '
            f'caches dropped - warm {statistics.median(cold[form]) - statistics.median(ms[form]):7.3f} ms   gate_info {lp.gate_info()} range_info {lp.range_info()}')
    if not parent:
        c = loops[forms[0]].counters()
        say(f'{name:13s} algorithmic bytes per body {c["bytes_per_iteration"] / 1e6:.1f} MB; the seed adds 4 H1 = {4 * h1} B per node-update = {4e-6 * h1 * n:.1f} MB '
            f'({100 * 4 * h1 * n / c["bytes_per_iteration"]:.1f} %) and takes the 4 IW = {4 * iw} B per node of label columns ({4e-6 * iw * n:.1f} MB) out of every body')
        if len(forms) > 1:
            a, b = statistics.median(ms[forms[0]]), statistics.median(ms[forms[-1]])
            say(f'{name:13s} {forms[-1]} / {forms[0]} = {b / a:.4f} per Loop')
    for lp in loops.values(): lp.close()
    graph.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--parent', action='store_true', help='a library without the projection: the wide shapes on its fallback')
    args = ap.parse_args()
    if args.parent: e.EXPORTS[:] = [x for x in e.EXPORTS if 'label_projection' not in x]
    say(f'# library: {e.LIB_PATH}')
    shape('mutag-widths', args.nodes, 14, 3, ['off'] if args.parent else ['off', 'auto'], args.alternations, args.parent)
    shape('wide-128', args.nodes // 4, 128, 1, ['off'] if args.parent else ['off', 'auto'], args.alternations, args.parent)
    if not args.parent: shape('narrow', args.nodes, 3, 1, ['off', 'always'], args.alternations, False)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
