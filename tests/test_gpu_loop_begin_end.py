"""What a full-size Loop does around its bodies (csrc/gnn_loop.hip: loop_begin, loop_finish, run_loops_once), at the smallest shapes where
each piece can go wrong.

1. INITIAL STATE READ IN PLACE.  On one GPU with state_vect_dim > 0 and one launch per body, body 0 gathers from the table gnn_loop_set_state0
   filled (padded to the replica's row count) and nothing copies it; "the state after k bodies" is that table for k = 0 and state[k & 1]
   after.  Generic kernel (Ds = 8; 333 and 4,129 rows) and full-tile kernel with the gather program (Ds = 64, 136 -> 128 -> 128 -> 64; 333 and
   32 * 9 + 1 rows: the partial last tile reads the padded tail), stops at k = 0, 1, 2, 3 and max_iteration, two runs per handle, another
   state between two runs, a state drawn on the device; a D = 0 loop and a world-2 loopback group (which keep the copy) beside them.
2. FIRST CONDITION (k_check_first, csrc/gnn_engine.hip): Ds = 5, 7, 8, 64, 68 and 132 (past the streamed form: k_check), 1, 255, 256, 257
   rows, a threshold between the largest and the second largest first ratio - one row decides - and one above both.
3. OUTPUT STAGE (k_out1): 0, 1, 63, 64, 65 masked rows (its block is 64 rows), T = 1, 2, 3, 8, Ds = 5, 8, 64; softmax + BatchNormalization,
   tanh, the saturating head; a head too large for it.
4. LOOK-AHEAD at the host's gate reads: max_iteration 16, 17, 20, 21, 33 and stops at 15, 16, 17, 19, 20, 21, on impl 1 and impl 2; a
   profiled run that stopped at k has timed k bodies.

References as in test_gpu_loop_ends.py: oracle.c_oracle bit for bit for impl 0 and 1; for impl 2 the oracle's k, 1e-5 from the float64 oracle
and 2e-6 max(1, max|s|) from the exact chain."""
import functools

import numpy as np
import pytest

import test_gpu_loop_ends as le
from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu


def _graph(rng, n, nl):
    """n nodes, two arc-label columns, 'average' aggregation; a single node has no arc"""
    arcs = random_arcs(rng, n, 3 * n, 2) if n > 1 else np.zeros((0, 4), np.float32)
    g = orc.make_graph_dict(arcs, (2 * rng.random((n, nl)) - 1).astype(np.float32), 'average')
    g['set_mask'] = np.ones(n, bool)
    g['output_mask'] = np.ones(n, bool)
    return g


class Chain:
    """A case and its exact chain body by body (the recipe of test_gpu_loop_ends.StopCase): r[b] is the largest distance / norm ratio the gate
    in front of body b sees, so a threshold between r[b] and min(r[:b]) stops the Loop at k = b, and one above r[0] at k = 0.  The initial
    state is the net's own state after `warm` bodies from a random start: from a random start itself the first body moves every node by more
    than the first condition's ratio (about 1), and no threshold would stop at k = 1."""

    def __init__(self, seed, n, d, nl, hidden, depth, head=(2,), head_act='softmax', warm=3):
        rng = np.random.default_rng(seed)
        self.n, self.d, self.nl = n, d, nl
        self.g = _graph(rng, n, nl)
        ds, nlc = (d if d else nl), (nl if d else 0)
        self.st = make_mlp(rng, 2 + 2 * (ds + nlc), list(hidden) + [ds], 'tanh', gain=0.6, bn_random=True)
        self.ou = make_mlp(rng, ds + nlc, list(head), head_act, bn_random=True)
        self.s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32) if d else None
        if d and warm: self.s0 = np.ascontiguousarray(self.loop(warm, 0.0, self.s0, want_out=False)[1])
        first = self.s0 if d else self.g['nodes']
        self.states = [np.ones_like(first), first]
        for _ in range(depth if d else 0):                   # (D = 0: the state is the label table, only the first condition can be placed)
            self.states.append(self.loop(1, 0.0, self.states[-1], want_out=False)[1])
        self.r = [np.sort(le._ratios(self.states[b + 1], self.states[b])) for b in range(len(self.states) - 1)]
        self._want = {}

    def loop(self, max_it, thr, s0, want_out=True):
        if not self.d: assert s0 is None or s0 is self.g['nodes'] or np.array_equal(s0, self.g['nodes'])
        return corc.loop_node(self.g, self.st, self.ou, self.d, max_it, thr, s0 if self.d else None, n_threads=1 if self.n < 2000 else 0, want_out=want_out)

    def threshold(self, b):
        """stop at k = b (b = 0: above every first ratio)"""
        top = float(self.r[b][-1])
        if b == 0: return float(np.float32(1.5 * top))
        lo = min(float(self.r[i][-1]) for i in range(b))
        assert top <= 0.96 * lo, (b, top, lo)
        return float(np.float32(np.sqrt(top * lo)))

    def want(self, thr, max_it, s0=None):
        key = (thr, max_it, None if s0 is None else s0.tobytes())
        if key not in self._want: self._want[key] = self.loop(max_it, thr, self.s0 if s0 is None else s0)
        return self._want[key]

    def want64(self, bodies):
        key = ('f64', bodies)
        if key not in self._want: self._want[key] = orc.loop_node(self.g, self.st, self.ou, self.d, bodies, 0.0, self.s0, np.float64)
        return self._want[key]


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. the initial state read in place
# ----------------------------------------------------------------------------------------------------------------------------------------
MAX_IT1 = 5
# id: seed, n, d, NL, hidden layers, impls
ELISION = {
    'generic_333': (9301, 333, 8, 3, (16,), (0, 1, 2)),
    'generic_4129': (9302, 4129, 8, 3, (16,), (0, 1, 2)),
    'full_tile_333': (9303, 333, 64, 3, (128, 128), (1, 2)),
    'full_tile_289': (9304, 32 * 9 + 1, 64, 3, (128, 128), (1, 2)),
}


@functools.lru_cache(maxsize=None)
def _chain(case):
    seed, n, d, nl, hidden, _ = ELISION[case]
    return Chain(seed, n, d, nl, hidden, MAX_IT1)


def _check(loop, impl, c, want, bodies, what):
    if impl == 2: le._close_twice(loop, want, c.want64(bodies), what)
    else: le._exact_twice(loop, want, what)


@pytest.mark.parametrize('stop', [0, 1, 2, 3, None])
@pytest.mark.parametrize('case', sorted(ELISION))
def test_initial_state_in_place(case, stop):
    """stops at k = 0 (state and output are those of the initial state), 1, 2, 3 and max_iteration = 5 (threshold 0): k, lp.state() - the
    initial table, state[1], state[0], state[1] - and the output, twice per handle"""
    e, c = le._engine(), _chain(case)
    thr = 0.0 if stop is None else c.threshold(stop)
    want = c.want(thr, MAX_IT1)
    k_want = MAX_IT1 if stop is None else stop
    assert want[0] == k_want, (case, stop, want[0])
    if stop == 0: assert np.array_equal(want[1], c.s0)
    if case.startswith('full_tile'):
        dims = le._dims(c.st)
        assert dims == [136, 128, 128, 64] and not e.small_form(dims, c.st['activations'], c.n, c.nl)['persistent']
    handles = le._device(e, c.g, c.st, c.ou)
    for impl in ELISION[case][5]:
        loop = le._new_loop(e, handles, c.d, c.s0, 'bodies_only' if case.startswith('full_tile') else 'bodies', impl, MAX_IT1, thr)
        _check(loop, impl, c, want, k_want, f'{case}, stop {stop}, impl {impl}')
        loop.close()
    handles[0].close()


@pytest.mark.parametrize('case', ['generic_333', 'full_tile_289'])
def test_initial_state_replaced_and_drawn(case):
    """one handle: run, set_state0 with another state, run, the first state again, run - each the oracle's bits from its own state (the table
    is rewritten by set_state0 only, never by a run); then a state drawn on the device: two runs return the same bits, and the same seed
    draws them again"""
    e, c = le._engine(), _chain(case)
    thr = c.threshold(2)
    other = np.ascontiguousarray(c.states[3])                # the chain's state after two bodies: from there the Loop stops earlier
    wants = [c.want(thr, MAX_IT1), c.want(thr, MAX_IT1, other)]
    assert wants[0][0] == 2 and wants[1][0] < 2
    handles = le._device(e, c.g, c.st, c.ou)
    loop = le._new_loop(e, handles, c.d, c.s0, 'bodies_only' if case.startswith('full_tile') else 'bodies', 1, MAX_IT1, thr)
    for step, (s0, want) in enumerate([(c.s0, wants[0]), (other, wants[1]), (c.s0, wants[0])]):
        loop.set_state0(s0)
        le._exact_twice(loop, want, f'{case}, state {step}')
    drawn = []
    for seed in (7, 7, 8):
        loop.set_state0(None, seed=seed)
        a = (loop.run(), loop.state(), loop.output())
        b = (loop.run(), loop.state(), loop.output())
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (case, seed, 'second run differs')
        assert np.isfinite(a[1]).all()
        drawn.append(a)
    assert drawn[0][0] == drawn[1][0] and np.array_equal(drawn[0][1], drawn[1][1]) and np.array_equal(drawn[0][2], drawn[1][2])
    assert not np.array_equal(drawn[0][1], drawn[2][1])
    loop.close()
    handles[0].close()


@pytest.mark.parametrize('stop', [0, 1, 2])
def test_kept_copy_beside_in_place(stop):
    """the layouts that keep the copy of the initial state, interleaved with an in-place loop on the same device: D = 0 (the state is the
    label table, which no warm start can replace: k = 0, or max_iteration at threshold 0) and a world-2 loopback group, each against the C
    oracle"""
    from test_gpu_sharded import _collect, _sharded_loops
    e, c = le._engine(), _chain('generic_333')
    c0 = _chain_d0()
    thr, thr0 = c.threshold(stop), (c0.threshold(0) if stop == 0 else 0.0)
    want, want0 = c.want(thr, MAX_IT1), c0.want(thr0, MAX_IT1)
    assert want[0] == stop and want0[0] == (0 if stop == 0 else MAX_IT1)
    handles, handles0 = le._device(e, c.g, c.st, c.ou), le._device(e, c0.g, c0.st, c0.ou)
    comms, graphs, loops, ranges = _sharded_loops(e, c.g, c.st, c.ou, c.d, MAX_IT1, thr, c.s0, 2, 1, halo=False)
    for impl in (0, 1):
        lp = le._new_loop(e, handles, c.d, c.s0, 'bodies', impl, MAX_IT1, thr)
        lp0 = le._new_loop(e, handles0, 0, None, 'bodies', impl, MAX_IT1, thr0)
        for rep in range(2):
            k, k0, kg = lp.run(), lp0.run(), e.Loop.run_group(loops)
            assert (k, k0, kg) == (want[0], want0[0], want[0]), (impl, rep, k, k0, kg)
            assert np.array_equal(lp.state(), want[1]) and np.array_equal(lp.output(), want[2]), (impl, rep, 'in place')
            assert np.array_equal(lp0.state(), want0[1]) and np.array_equal(lp0.output(), want0[2]), (impl, rep, 'D = 0')
            state, out = _collect(loops, ranges, None)
            assert np.array_equal(state, want[1]) and np.array_equal(out, want[2]), (impl, rep, 'world 2')
        lp.close(); lp0.close()
    for x in loops + graphs + comms: x.close()
    handles[0].close(); handles0[0].close()


@functools.lru_cache(maxsize=None)
def _chain_d0():
    return Chain(9305, 333, 0, 6, (16,), MAX_IT1)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. the first condition
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _first_case(d, n):
    return Chain(9400 + d, n, d, 3, (16,), 1)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
@pytest.mark.parametrize('d', [5, 7, 8, 64, 68, 132])
def test_first_condition(d, n):
    """the gate in front of body 0 with ONE row above the threshold (k >= 1), and with none (k = 0), against the C oracle on impl 0 and 1 (the first condition is the same kernel behind both)"""
    e, c = le._engine(), _first_case(d, n)
    r = c.r[0]
    top, second = float(r[-1]), float(r[-2]) if n > 1 else 0.5 * float(r[-1])
    assert second < top
    open_thr, closed_thr = float(np.float32(0.5 * (top + second))), float(np.float32(1.25 * top))
    assert int(np.sum(r > np.float32(open_thr))) == 1 and not np.any(r > np.float32(closed_thr))
    handles = le._device(e, c.g, c.st, c.ou)
    for thr, opens in ((open_thr, True), (closed_thr, False)):
        want = c.want(thr, 2)
        assert (want[0] >= 1) == opens, (d, n, thr, want[0])
        for impl in ((0, 1) if d <= 68 else (0,)):           # (Ds = 132 has no fused body: the per-op path alone)
            loop = le._new_loop(e, handles, c.d, c.s0, 'bodies', impl, 2, thr)
            le._exact_twice(loop, want, f'Ds {d}, {n} rows, threshold {thr}, impl {impl}')
            loop.close()
    handles[0].close()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. the output stage
# ----------------------------------------------------------------------------------------------------------------------------------------
MAX_IT3 = 2
HEADS3 = {'softmax_bn': ('softmax', True, 1.0), 'tanh': ('tanh', False, 1.0), 'softmax_x200': ('softmax', False, 200.0)}


@functools.lru_cache(maxsize=None)
def _out_case(d):
    return Chain(9500 + d, 333, d, 3, (16,), 0)


@functools.lru_cache(maxsize=None)
def _out_head(d, t, head):
    act, bn, factor = HEADS3[head]
    ou = make_mlp(np.random.default_rng([9500 + d, t, sorted(HEADS3).index(head)]), d + 3, [t], act, batch_normalization=bn, bn_random=True)
    ou['weights'][0] = (ou['weights'][0] * np.float32(factor)).astype(np.float32)
    return ou


@functools.lru_cache(maxsize=None)
def _out_mask(rows):
    m = np.zeros(333, bool)
    m[np.random.default_rng(rows).choice(333, rows, replace=False)] = True
    return m


@functools.lru_cache(maxsize=None)
def _out_want(d, t, head, rows):
    c = _out_case(d)
    g = dict(c.g, set_mask=_out_mask(rows), output_mask=np.ones(333, bool))
    return corc.loop_node(g, c.st, _out_head(d, t, head), d, MAX_IT3, 0.0, c.s0, n_threads=1)


OUT_CASES = ([(d, t, 'softmax_bn', 65) for d in (5, 8, 64) for t in (1, 2, 3, 8)] +
             [(d, 3, 'softmax_bn', rows) for d in (8, 64) for rows in (0, 1, 63, 64, 128, 129)] +
             [(d, t, 'tanh', 65) for d, t in ((5, 2), (8, 8), (64, 2))] + [(d, 3, 'softmax_x200', 65) for d in (5, 8, 64)])


@pytest.mark.parametrize('d,t,head,rows', OUT_CASES)
def test_output_stage(d, t, head, rows):
    """k_out1 behind impl 0 and impl 1 (the exact chains: the oracle's bits); masks that end in front of, on and behind the edge of its
    64-row block and of the second block"""
    e, c = le._engine(), _out_case(d)
    want = _out_want(d, t, head, rows)
    assert want[0] == MAX_IT3 and want[2].shape == (rows, t)
    if head == 'softmax_x200': assert np.any(want[2] == 1.0) and np.any(want[2] == 0.0) and not np.isnan(want[2]).any()
    handles = le._device(e, c.g, c.st, _out_head(d, t, head), _out_mask(rows))
    for impl in (0, 1):
        loop = le._new_loop(e, handles, d, c.s0, 'bodies', impl, MAX_IT3, 0.0)
        le._exact_twice(loop, want, f'Ds {d}, T {t}, {head}, {rows} masked rows, impl {impl}')
        loop.close()
    handles[0].close()


def test_output_head_too_large_still_per_op():
    """a one-layer T = 8 head on 230 feature columns is outside the LDS condition of loop_finish: k_feats + launch_mlp, the oracle's bits"""
    le.test_output_head_too_large_for_out1()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. look-ahead at the host's gate reads
# ----------------------------------------------------------------------------------------------------------------------------------------
LOOKAHEAD = ([(m, None) for m in (16, 17, 20, 21, 33)] + [(le.MAX_IT, b) for b in (15, 16, 17, 19, 20, 21)] +
             [(33, b) for b in (15, 16, 17, 19, 20, 21)] + [(20, 19), (21, 19), (21, 20), (17, 16)])


@pytest.mark.parametrize('max_it,b', LOOKAHEAD)
@pytest.mark.parametrize('impl', [1, 2])
def test_stop_around_the_lookahead(impl, max_it, b):
    """the gate of body 16 reaches the host while bodies 16 .. 19 are queued behind it: stops in front of, on and behind the read (15, 16,
    17) and its look-ahead (19, 20, 21), max_iteration at the same places; no repeat is reported; a profiled run has timed k bodies"""
    e, c = le._engine(), le._stop_case()
    if b is None:
        thr, want = 0.0, c.want(0.0, max_it)
        assert want[0] == max_it
    else:
        thr, want = c.stop_at(b, max_it)
    k_want = int(want[0])
    handles = c.handles(e)
    loop = le._new_loop(e, handles, c.d, c.s0, 'bodies', impl, max_it, thr)
    what = f'impl {impl}, max_iteration {max_it}, stop at {b}'
    if impl == 2: le._close_twice(loop, want, c.want64(k_want), what)
    else: le._exact_twice(loop, want, what)
    assert loop.gate_info() == (False, 0) and loop.range_info() == (False, 0), (what, loop.gate_info(), loop.range_info())
    loop.set_profiling(True)
    assert loop.run() == k_want
    t = loop.timing()
    assert t['n_iter_timed'] == k_want, (what, t)
    loop.set_profiling(False)
    loop.close()
    handles[0].close()
