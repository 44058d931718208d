"""Inputs of tests/test_gpu_label_projection.py (no test in here): loops with wide node / arc labels, built as test_gpu_parity._case builds its
own - random_arcs, labels U(-1, 1), make_mlp(..., gain=0.5, bn_random=True), an injected state0 - and their oracle results, computed once."""
import functools

import numpy as np

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

# n, state width, node labels, arc labels, hidden widths, activation, bodies at threshold 0, k at threshold 0.01 (fp32 and float64 oracle), per-body kernel
#                                                                                       (1 k_fused_generic, 2 k_fused_full)
CASES = [
    dict(n=333, d=64, nl=40, al=3, hidden=(128, 128), act='tanh', max_it=4, k=4, kernel=2),
    dict(n=320, d=64, nl=40, al=3, hidden=(128,), act='selu', max_it=5, k=6, kernel=2),
    dict(n=31, d=64, nl=21, al=3, hidden=(128, 128), act='relu', max_it=3, k=3, kernel=2),          # a single, partial tile
    dict(n=333, d=20, nl=150, al=2, hidden=(64,), act='tanh', max_it=5, k=4, kernel=1),             # IW = 302
    dict(n=333, d=48, nl=40, al=3, hidden=(), act='tanh', max_it=5, k=6, kernel=1),                 # one layer: the seed feeds the last layer + BatchNormalization
    dict(n=333, d=64, nl=14, al=3, hidden=(128, 128), act='selu', max_it=5, k=6, kernel=2),         # the MUTAG label widths
    dict(n=97, d=32, nl=40, al=1, hidden=(32, 32), act='sigmoid', max_it=2, k=2, kernel=1),         # one feature tile
    # a last activation of its own; no BatchNormalization
    dict(n=333, d=64, nl=40, al=3, hidden=(128, 128), act='selu', out_act='tanh', max_it=4, k=None, kernel=2),
    dict(n=333, d=64, nl=40, al=3, hidden=(128, 128), act='tanh', bn=False, max_it=4, k=None, kernel=2),
]
CONVERGING = range(7)


def build(seed, n, d, nl, al, hidden, act, out_act=None, bn=True, gain=0.5, **_):
    rng = np.random.default_rng(seed)
    arcs = random_arcs(rng, n, 3 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    ds, nls = (d if d else nl), (nl if d else 0)
    st = make_mlp(rng, al + 2 * (ds + nls), list(hidden) + [ds], act, batch_normalization=bn, out_activation=out_act, gain=gain, bn_random=True)
    ou = make_mlp(rng, ds + nls, [2], 'softmax', bn_random=True)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
    return g, st, ou, s0


@functools.lru_cache(maxsize=None)
def case(i):
    """(g, st, ou, s0) of CASES[i], seed 7000 + i.  Shared between the tests: nobody writes to it."""
    return build(7000 + i, **CASES[i])


@functools.lru_cache(maxsize=None)
def oracles(i, max_it, thr):
    """C oracle (the bit-exact fp32 chain) and float64 oracle of CASES[i]: (k, state, output) each."""
    g, st, ou, s0 = case(i)
    d = CASES[i]['d']
    return corc.loop_node(g, st, ou, d, max_it, thr, s0), orc.loop_node(g, st, ou, d, max_it, thr, s0, np.float64)


def mover_margin(i, max_it):
    """Smallest over the gates 1 .. max_it of a threshold-0 Loop of the largest distance / (1e-5 norm) over the nodes, on the fp32 oracle:
    > 1 at every gate means every gate of the run, the last included, sees a robust mover of the certified gate (band 1e-5 norm)."""
    g, st, ou, s0 = case(i)
    _, _, _, trace = orc.loop_node(g, st, ou, CASES[i]['d'], max_it, 0.0, s0, np.float32, return_trace=True)
    states = [np.asarray(s0 if s0 is not None else g['nodes'], np.float64)] + [np.asarray(s, np.float64) for s in trace]
    worst = np.inf
    for old, new in zip(states[:-1], states[1:]):
        dist, nrm = np.sqrt(((new - old) ** 2).sum(1)), np.sqrt((old ** 2).sum(1))
        worst = min(worst, float(np.max(dist / np.maximum(1e-5 * nrm, 1e-300))))
    return worst, len(trace)


def label_block(g, d):
    """[nodes | Adjacency^T . nodes | ArcNode^T . arc labels] in fp32, the chains of the engine's own aggregation (C oracle), or
    [ArcNode^T . arc labels] alone for a loop whose state is the labels (d == 0)."""
    nodes = np.asarray(g['nodes'], np.float32)
    agg_arcs = corc.spmm(g['arcT'], np.asarray(g['arcs'], np.float32)[:, 2:])
    if not d: return agg_arcs
    return np.concatenate([nodes, corc.spmm(g['adjT'], nodes), agg_arcs], axis=1)


def label_rows(st, ds, nlc):
    """The rows of net_state's first kernel that multiply the label block, in its column order, and the layer's bias."""
    w1 = np.asarray(st['weights'][0], np.float32)
    return np.concatenate([w1[ds:ds + nlc], w1[2 * ds + nlc:]]), np.asarray(st['weights'][1], np.float32)
