"""The wide-state form (Loop.set_wide_state) against what a wide-state Loop runs without it, alternating in one process.

Shapes (syntheticGraph(N, 10.0, 3, 1): the benchmark graph's arcs and labels; net_state concat -> 128 -> 128 -> D SELU, BODIES bodies at
threshold 0, impl 2 asked for):
  n1m-d128    N = 1,000,000, state width 128 (concat 263: four waves per workgroup);
  n250k-d128  N = 250,000, the same net;
  n1m-d96     N = 1,000,000, state width 96 (concat 199: five waves);
  n32k-d128, n4k-d128, n1k-d128   N = 32,768 / 4,096 / 1,024, state width 128: what 'auto' needs to know about small graphs - 1,024
              tiles (one per wave of the launch), 128 and 32 tiles (fewer workgroups than CUs).
Forms, one loop each on the same graph and nets:
  per-op      mode 'off': k_spmm, the materialised concat and k_dense<8> - the code of the commit before the form, unchanged by it;
  generic     the form with load_tile_generic on every tile (Loop.set_wide_loader('generic'));
  wide        the form with load_tile_wide on the full tiles (the default loader).
Per round one warm Loop of every form, in turn, host clock around a Loop that ends in a device synchronise; reported: median / min / max
over the rounds of ms per body, and the largest state difference between the forms.
One shape per call, so that a runner can give each its own time limit and chain them:
  for s in n1m-d128 n250k-d128 n1m-d96; do timeout -k 10 300 python tools/bench_wide_state.py --shape $s --out report_$s.txt || break; done"""
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

SHAPES = {'n1m-d128': (1_000_000, 128), 'n250k-d128': (250_000, 128), 'n1m-d96': (1_000_000, 96),
          'n32k-d128': (32_768, 128), 'n4k-d128': (4_096, 128), 'n1k-d128': (1_024, 128)}
LINES = []
NL, AL = 3, 1


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=sorted(SHAPES), required=True)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--bodies', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    nodes, d = SHAPES[args.shape]
    s = utils.syntheticGraph(nodes, 10.0, NL, AL, 2, seed=20261020)
    n = s['n_nodes']
    rng = np.random.default_rng(20261020)
    st = make_mlp(rng, AL + 2 * (NL + d), [128, 128, d], 'selu')        # (gain 1, as bench.py: no contraction, every gate sees movers)
    ou = make_mlp(rng, NL + d, [2], 'softmax')
    state0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    say(f'# library: {e.LIB_PATH}')
    say(f'# {args.shape}: {n} nodes, {s["n_arcs"]} arcs, net_state {AL + 2 * (NL + d)} -> 128 -> 128 -> {d}, {args.bodies} bodies at threshold 0, {args.rounds} rounds')
    loops, used = {}, {}
    for form in ('per-op', 'generic', 'wide'):
        lp = e.Loop(graph, mst, mou, d, args.bodies, 0.0)
        lp.set_state0(state0)
        taken = lp.set_wide_state('off' if form == 'per-op' else 'always')
        loader = lp.set_wide_loader('generic' if form == 'generic' else 'wide')
        used[form] = (lp.set_impl(2), lp.body_kernel(), taken, loader, lp.body_launch())
        loops[form] = lp
    assert used['per-op'][0] == 0 and used['generic'][2] and not used['generic'][3] and used['wide'][2] and used['wide'][3], used
    for lp in loops.values():                                      # warm-up: code objects, weight images, label block, buffers
        lp.run(); lp.run()
    ms = {f: [] for f in loops}
    for _ in range(args.rounds):
        for form, lp in loops.items():
            t, k = timed_loop(lp)
            assert k == args.bodies, (form, k)
            ms[form].append(t / args.bodies)
    states = {f: lp.state() for f, lp in loops.items()}
    for form, lp in loops.items():
        impl, kernel, taken, loader, (waves, grid) = used[form]
        say(f'{args.shape:11s} {form:8s} impl used {impl} body kernel {kernel} waves {waves} grid {grid} load_tile_wide {int(loader)}   ms/body {spread(ms[form])}   '
            f'gate_info {lp.gate_info()} range_info {lp.range_info()}')
    a, g_, w = (statistics.median(ms[f]) for f in ('per-op', 'generic', 'wide'))
    say(f'{args.shape:11s} per-op / wide = {a / w:.2f}, per-op / generic = {a / g_:.2f}, generic / wide = {g_ / w:.3f} (medians)')
    say(f'{args.shape:11s} max |state(wide) - state(generic)| {np.max(np.abs(states["wide"] - states["generic"])):.2e}, '
        f'max |state(wide) - state(per-op)| {np.max(np.abs(states["wide"] - states["per-op"])):.2e}, max |state| {np.max(np.abs(states["per-op"])):.2e}')
    for lp in loops.values(): lp.close()
    graph.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
