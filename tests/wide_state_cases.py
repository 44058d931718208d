"""Inputs of tests/test_gpu_wide_state.py and tests/test_wide_state_host.py (no test in here): loops with state widths 76 .. 128, built by
label_projection_cases.build - random_arcs, labels U(-1, 1), make_mlp(..., gain=0.5, bn_random=True), an injected state0 - and their oracle
results, computed once.

What the cases were chosen for is asserted by check_case, on this machine's CPU: the C oracle stays within 7.3e-7 of the float64 oracle (so
the reference alone uses under a tenth of the default path's 1e-5), every gate of a threshold-0 Loop sees a robust mover of the certified
gate (margin > 5 x band), and the graphs of n = 333 have rows of in-degree 0 and above 16 - an empty row, tail batches and a full batch
of the wide-row loader's 16-entry batches are all walked."""
import functools

import numpy as np

import label_projection_cases as lc
from oracle import c_oracle as corc
from oracle import gnn_oracle as orc

# n, state width, node labels, arc labels, hidden widths, activation, bodies at threshold 0, k at threshold 0.01 (fp32 and float64 oracle;
# None: not run), waves per workgroup of the wide-state form, seeded: covered only together with the label projection
CASES = [
    dict(n=333, d=128, nl=3, al=2, hidden=(128, 128), act='tanh', max_it=4, k=4, waves=4),
    dict(n=333, d=128, nl=3, al=2, hidden=(128,), act='selu', max_it=4, k=9, waves=4),
    dict(n=320, d=96, nl=5, al=1, hidden=(64,), act='relu', max_it=4, k=4, waves=5),
    dict(n=333, d=100, nl=3, al=2, hidden=(128, 128), act='tanh', max_it=4, k=4, waves=5),             # a last feature tile of 4 columns
    dict(n=333, d=76, nl=3, al=2, hidden=(), act='tanh', max_it=4, k=8, waves=7),                       # one layer; the first width past the eight-wave tile
    dict(n=333, d=128, nl=40, al=3, hidden=(128, 128), act='tanh', max_it=4, k=4, waves=4, seeded=True),  # no 4-wave tile of its own: with the label projection
    dict(n=31, d=128, nl=3, al=2, hidden=(128, 128), act='tanh', max_it=3, k=None, waves=4),            # a single, partial tile
    dict(n=333, d=128, nl=3, al=2, hidden=(128, 128), act='selu', out_act='tanh', bn=False, max_it=4, k=5, waves=4),
]
UNSEEDED = [i for i, c in enumerate(CASES) if not c.get('seeded')]
SEED0 = 9100


@functools.lru_cache(maxsize=None)
def case(i):
    """(g, st, ou, s0) of CASES[i], seed 9100 + i.  Shared between the tests: nobody writes to it."""
    return lc.build(SEED0 + i, **CASES[i])


@functools.lru_cache(maxsize=None)
def oracles(i, max_it, thr):
    """C oracle (the bit-exact fp32 chain) and float64 oracle of CASES[i]: (k, state, output) each."""
    g, st, ou, s0 = case(i)
    d = CASES[i]['d']
    return corc.loop_node(g, st, ou, d, max_it, thr, s0), orc.loop_node(g, st, ou, d, max_it, thr, s0, np.float64)


def net_description(i):
    """(dims, activations, state width, node-label columns, arc-label columns, rows) of CASES[i]'s net_state, as _engine.wide_state_form takes them."""
    c = CASES[i]
    _, st, _, _ = case(i)
    dims = [int(np.asarray(st['weights'][0]).shape[0])] + list(c['hidden']) + [c['d']]
    return dims, list(st['activations']), c['d'], c['nl'], c['al'], c['n']


def mover_margin(i, max_it):
    """label_projection_cases.mover_margin on these cases: smallest over the gates of a threshold-0 Loop of the largest distance / (1e-5 norm)."""
    g, st, ou, s0 = case(i)
    _, _, _, trace = orc.loop_node(g, st, ou, CASES[i]['d'], max_it, 0.0, s0, np.float32, return_trace=True)
    states = [np.asarray(s0, np.float64)] + [np.asarray(s, np.float64) for s in trace]
    worst = np.inf
    for old, new in zip(states[:-1], states[1:]):
        dist, nrm = np.sqrt(((new - old) ** 2).sum(1)), np.sqrt((old ** 2).sum(1))
        worst = min(worst, float(np.max(dist / np.maximum(1e-5 * nrm, 1e-300))))
    return worst, len(trace)


@functools.lru_cache(maxsize=None)
def check_case(i):
    """The properties the case was chosen for (module docstring); returns (reference error, margin)."""
    c = CASES[i]
    g, _, _, _ = case(i)
    (kc, sc, oc), (k64, s64, o64) = oracles(i, c['max_it'], 0.0)
    ref_err = max(float(np.max(np.abs(sc - s64))), float(np.max(np.abs(oc - o64))))
    assert kc == k64 == c['max_it'] and ref_err <= 7.3e-7, (i, kc, k64, ref_err)
    margin, bodies = mover_margin(i, c['max_it'])
    assert bodies == c['max_it'] and margin > 5.0, (i, bodies, margin)
    if c['k'] is not None:
        (kc, sc, oc), (k64, s64, o64) = oracles(i, 30, 0.01)
        assert kc == k64 == c['k'], (i, kc, k64)
        assert max(float(np.max(np.abs(sc - s64))), float(np.max(np.abs(oc - o64)))) <= 7.3e-7
    if c['n'] == 333:
        deg = np.diff(np.asarray(g['adjT'][0]))
        assert deg.min() == 0 and deg.max() > 16, (i, int(deg.min()), int(deg.max()))
    return ref_err, margin
