"""What a full-size Loop spends OUTSIDE its bodies (loop_begin, loop_finish, the launch gaps and the host's gate reads), from the loop's own
events, and the wall time of a Loop, on the library GNN_HIP_LIBRARY names (default: the product).

  deep        1 M nodes, 135 -> 128 -> 128 -> 64 selu, threshold 0, max_iteration 30: the benchmark's Loop (30 bodies)
  converging  the same at gain 0.5 and threshold 0.01, max_iteration 50: stops after about 8 bodies (tools/gate_study.py B)

Per workload: k; from profiled runs the time between the Loop's first and last event, the sum of its bodies, their difference (everything this
script is about) and the mean gap between two bodies; from unprofiled runs the wall time per Loop.  Medians over the runs.

Needs an MI355X.  python tools/loop_ends_timing.py [runs]      (one line per workload on stdout)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_study as gs      # noqa: E402  (setup: the graph and nets of its part B)

e = gs.e


def measure(name, gain, max_it, thr, runs):
    graph, mst, mou, s0 = gs.setup(1_000_000, 100, gain, 'selu')
    lp = e.Loop(graph, mst, mou, 64, max_it, thr)
    lp.set_persistent(False)
    lp.set_state0(s0)
    k = lp.run()
    wall = []
    for _ in range(runs):
        t = time.perf_counter()
        assert lp.run() == k
        wall.append(1e3 * (time.perf_counter() - t))
    lp.set_profiling(True)
    lp.run()
    rows = []
    for _ in range(runs):
        assert lp.run() == k
        t = lp.timing()
        assert t['n_iter_timed'] == k
        rows.append((t['total_ms'], t['avg_iter_ms'] * k, t['total_ms'] - t['avg_iter_ms'] * k, t['avg_between_bodies_ms']))
    lp.close(); graph.close()
    tot, bodies, outside, gap = (float(np.median([r[i] for r in rows])) for i in range(4))
    print(f'{os.path.basename(os.environ.get("GNN_HIP_LIBRARY", "libgnn_hip.so")):28s} {name:10s} k {int(k):2d} | events: Loop {tot:.3f} ms, bodies {bodies:.3f}, '
          f'outside the bodies {outside:.3f} (mean gap between bodies {1e3 * gap:.1f} us) | wall per Loop {float(np.median(wall)):.3f} ms '
          f'(min {min(wall):.3f}, max {max(wall):.3f}, {runs} runs)', flush=True)


if __name__ == '__main__':
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    e.require_device(0)
    measure('deep', 0.6, 30, 0.0, runs)
    measure('converging', 0.5, 50, 0.01, runs)
