"""Step time and scratch of the recomputing training step (gnn_loop_set_train_recompute) on the C3 shape: 1 M nodes / 10 M arcs, state_dim 64,
the benchmark's own nets (net_state 135 -> 128 -> 128 -> 64 selu + BatchNormalization, net_output 67 -> 2 softmax + BatchNormalization), threshold 0
(every body runs), Adam armed on the device behind every step.  Depths 5 and 30 bodies.

Protocol: one process per measurement, taken in turns - mode off on the parent commit's library (--parent-lib, skipped when not given), mode off on
this tree, mode on, mode on with the caching kernels in the first pass - three rounds.  Per process: `--warmup` steps, then the median of
`--steps` warm gnn_loop_train_step calls (host clock around a call that ends in a stream synchronisation) and gnn_loop_train_arena_bytes; with
the mode on also the median of `--forwards` gnn_loop_train_forward calls divided by the bodies: the first pass per body, cache-less chain
against caching kernels on scratch (the variant switch is --variant on / on_caching).

Every measuring process runs under its own `timeout`; the driver stops at the first non-zero status.
Run on the GPU box:  python tools/train_recompute_study.py [--parent-lib PATH] [--rounds 3] [--out profiles/train_recompute.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ('off', 'on', 'on_caching')


def worker(args):
    for p in (ROOT, os.path.join(ROOT, 'gnn_tf_2.x_amd')):
        sys.path.insert(0, p)
    import numpy as np
    import bench
    from GNN import GNN_utils as utils, _engine as e
    if args.parent: e.EXPORTS[:] = [x for x in e.EXPORTS if 'train_recompute' not in x]
    N, d = args.nodes, 64
    s = utils.syntheticGraph(N, 10, 3, 1, 2, seed=20261003)
    n = s['n_nodes']
    rng = np.random.default_rng(20261003)
    st = bench.make_net(rng, 1 + 2 * (3 + d), [128, 128, d], 'selu')
    ou = bench.make_net(rng, 3 + d, [2], 'softmax')
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    loop = e.Loop(graph, mst, mou, d, args.bodies, 0.0)
    loop.set_state0(s0)
    targets = np.eye(2, dtype=np.float32)[rng.integers(0, 2, n)]
    weights = np.full(n, 1.0 / n, np.float32)
    if args.variant != 'off':
        assert loop.set_train_recompute(True, cacheless=args.variant == 'on')
    lr, b1, b2, t = 1e-4, 0.9, 0.999, 0

    def step():
        nonlocal t
        t += 1
        loop.arm_optimizer(1, [lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t), b1, b2, 1e-7], True)
        t0 = time.perf_counter()
        r = loop.train_step(mst, mou, None, targets, weights, 0, None)
        return time.perf_counter() - t0, r

    for _ in range(args.warmup): _, r = step()
    times = []
    for _ in range(args.steps):
        dt, r = step()
        times.append(dt)
    out = dict(tree='parent' if args.parent else 'this', variant=args.variant, bodies=args.bodies, k=int(r['k']), loss=float(r['loss']),
               step_ms=1e3 * statistics.median(times), step_ms_min=1e3 * min(times), arena_bytes=loop.train_arena_bytes())
    if args.variant != 'off':
        info = loop.train_recompute_info()
        out.update(replayed=info['replayed'], cacheless_chain=info['cacheless_chain'])
    if not args.parent:           # the first pass alone (mode off: the caching forward that keeps every body)
        fw = []
        for _ in range(args.forwards):
            t0 = time.perf_counter()
            loop.train_forward(mst, mou, None)
            fw.append(time.perf_counter() - t0)
        if fw: out.update(first_pass_ms_per_body=1e3 * statistics.median(fw) / max(1, args.bodies))
    print('RESULT ' + json.dumps(out), flush=True)


def driver(args):
    rows = []
    out = open(args.out, 'a') if args.out else None

    def emit(line):
        print(line, flush=True)
        if out: out.write(line + '\n'); out.flush()

    emit(f'# rounds {args.first_round} .. {args.first_round + args.rounds - 1}; nodes {args.nodes}, steps {args.steps}, warmup {args.warmup}, forwards {args.forwards}')
    for rnd in range(args.first_round, args.first_round + args.rounds):
        for bodies in args.depths:
            turns = ([('parent', 'off')] if args.parent_lib else []) + [('this', v) for v in VARIANTS]
            for tree, variant in turns:
                cmd = ['timeout', '-k', '10', str(args.limit_5 if bodies <= 5 else args.limit_30), sys.executable, os.path.abspath(__file__), '--worker',
                       '--variant', variant, '--bodies', str(bodies), '--steps', str(args.steps), '--warmup', str(args.warmup), '--forwards', str(args.forwards),
                       '--nodes', str(args.nodes)]
                env = dict(os.environ)
                if tree == 'parent':
                    cmd.append('--parent')
                    env['GNN_HIP_LIBRARY'] = os.path.abspath(args.parent_lib)
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if p.returncode != 0:
                    emit(f'# STOP: round {rnd} {tree} {variant} bodies {bodies} ended with status {p.returncode}')
                    emit('# ' + p.stdout[-2000:].replace('\n', '\n# '))
                    return p.returncode
                res = [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1]
                res['round'] = rnd
                rows.append(res)
                fp = res.get('first_pass_ms_per_body')
                emit(f"round {rnd}  bodies {bodies:2d}  {tree:6s} {variant:10s} k {res['k']:2d}  step {res['step_ms']:9.3f} ms (min {res['step_ms_min']:9.3f})  "
                     f"arena {res['arena_bytes']:13d} B  first pass / body {'%8.3f ms' % fp if fp is not None else '       -'}  "
                     f"chain {res.get('cacheless_chain', '-')}  replayed {res.get('replayed', '-')}  loss {res['loss']:.6f}")
    return 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--parent', action='store_true', help='worker: the library under GNN_HIP_LIBRARY has no recompute entry points (mode off only)')
    ap.add_argument('--variant', choices=VARIANTS, default='off')
    ap.add_argument('--bodies', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--forwards', type=int, default=30)
    ap.add_argument('--nodes', type=int, default=1_000_000)
    ap.add_argument('--parent-lib', default=None, help="driver: the parent commit's libgnn_hip.so")
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--first-round', type=int, default=1)
    ap.add_argument('--depths', type=int, nargs='+', default=[5, 30])
    ap.add_argument('--limit-5', type=int, default=150, help='seconds one 5-body process may take')
    ap.add_argument('--limit-30', type=int, default=300, help='seconds one 30-body process may take')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.worker: worker(a)
    else: sys.exit(driver(a))
