"""The tile schedule's builder (gnn_tile_schedule_build, host code): kind 0 is the identity, kind 1 a permutation that is a pure function of
its arguments, ends on the lightest tiles in non-increasing cost, keeps every window of `waves` body slots near the body's mean cost and
hands the eight waves of a workgroup first tiles of different cost."""
import numpy as np
import pytest

WAVES = 2048          # 8 waves x 256 CUs
CUS = 256


def _engine():
    from GNN import _engine
    return _engine


def tile_costs(indptr):
    """Real entries (arcs) of every 32-row tile, the partial last tile included."""
    indptr = np.asarray(indptr, np.int64)
    edges = np.minimum(np.arange(0, indptr.size - 1 + 32, 32), indptr.size - 1)
    return np.diff(indptr[edges])


_SYNTH = {}


def synthetic_costs():
    """Tile costs of syntheticGraph(300_000): 9,375 tiles, in-degree growing with the node id (built once, never modified)."""
    if 'c' not in _SYNTH:
        from GNN import GNN_utils as utils
        _SYNTH['c'] = tile_costs(utils.syntheticGraph(300_000, 10.0, seed=1)['indptr'])
        _SYNTH['c'].setflags(write=False)
    return _SYNTH['c']


def split(order, cost, waves):
    k = min(2 * waves, cost.size // 2)
    return order[:cost.size - k], order[cost.size - k:]


def check_permutation(order, slots):
    assert order.dtype == np.int32 and order.shape == (slots,)
    assert np.array_equal(np.sort(order), np.arange(slots))


def check_tail(order, cost, waves):
    """Stability and tail: the tail is exactly the end of the order sorted by (cost descending, id ascending), in that order - so it is
    non-increasing in cost and no tail tile is heavier than any body tile; the body holds the rest."""
    cost = np.asarray(cost, np.int64)
    ref = np.lexsort((np.arange(cost.size), -cost))
    body, tail = split(order, cost, waves)
    assert np.array_equal(tail, ref[body.size:])
    assert np.array_equal(np.sort(body), np.sort(ref[:body.size]))
    assert np.all(np.diff(cost[tail]) <= 0)
    if body.size and tail.size: assert cost[tail].max() <= cost[body].min()


def window_deviation(order, cost, waves, leave_out=None):
    """Largest |window mean / body mean - 1| over all windows of `waves` consecutive body slots (None: the body has no such window, or
    its mean is 0).  leave_out: a tile whose cost is left out of the body's mean and whose windows are skipped."""
    body, _ = split(order, cost, waves)
    c = np.asarray(cost, np.float64)[body]
    keep = np.ones(c.size, bool) if leave_out is None else body != leave_out
    if c.size < waves: return None
    mean = c[keep].mean()
    s = np.concatenate([[0.0], np.cumsum(c)])
    sums = s[waves:] - s[:-waves]
    if leave_out is not None:
        pos = int(np.flatnonzero(body == leave_out)[0])
        starts = np.arange(sums.size)
        sums = sums[(starts > pos) | (starts + waves <= pos)]
    if mean == 0: return float(np.abs(sums).max())
    return float(np.abs(sums / waves / mean - 1).max())


@pytest.mark.parametrize('waves', [16, WAVES])
def test_identity_and_permutation(waves):
    e = _engine()
    rng = np.random.default_rng(3)
    for slots in (1, 2, 4 * waves - 1, 4 * waves, 9375):
        cost = rng.integers(0, 2000, slots)
        assert np.array_equal(e.tile_schedule(cost, waves, 0), np.arange(slots))
        order = e.tile_schedule(cost, waves, 1)
        check_permutation(order, slots)
        check_tail(order, cost, waves)


def test_synthetic_graph_tail_and_windows():
    """The benchmark's recipe at 300 k nodes: ascending order ranges over tens of per cent, the balanced body stays within 10 %."""
    e = _engine()
    cost = synthetic_costs()
    assert cost.size == 9375
    order = e.tile_schedule(cost, WAVES, 1)
    check_permutation(order, cost.size)
    check_tail(order, cost, WAVES)
    dev = window_deviation(order, cost, WAVES)
    asc = window_deviation(np.arange(cost.size, dtype=np.int32), cost, WAVES)
    print(f'window means: balanced within {dev:.3%} of the body mean, ascending body within {asc:.3%}')
    assert dev <= 0.10
    for waves in (256, 512):                     # smaller devices: shorter windows (still several deals of the 61 strata), longer body
        o = e.tile_schedule(cost, waves, 1)
        check_tail(o, cost, waves)
        d = window_deviation(o, cost, waves)
        print(f'waves {waves}: within {d:.3%}')
        assert d <= 0.10


def test_two_valued_costs():
    """Tiles of two costs, both in the body (512 tail slots): every window holds both in the body's proportion."""
    e = _engine()
    rng = np.random.default_rng(5)
    cost = np.where(rng.random(9375) < 0.3, 100, 400)
    order = e.tile_schedule(cost, 256, 1)
    check_permutation(order, cost.size)
    check_tail(order, cost, 256)
    body, _ = split(order, cost, 256)
    assert np.unique(cost[body]).size == 2
    dev = window_deviation(order, cost, 256)
    print(f'two-valued: within {dev:.3%}')
    assert dev <= 0.10


def test_equal_costs_are_stable_by_tile_id():
    e = _engine()
    cost = np.full(9375, 320)
    order = e.tile_schedule(cost, WAVES, 1)
    check_permutation(order, cost.size)
    check_tail(order, cost, WAVES)
    body, tail = split(order, cost, WAVES)
    assert np.array_equal(tail, np.arange(body.size, cost.size))      # ties by id ascending: the highest ids are "the lightest"
    assert np.array_equal(np.sort(body), np.arange(body.size))
    assert window_deviation(order, cost, WAVES) == 0.0


def test_one_huge_cost_among_zeros():
    """One hub tile among empty ones.  No order keeps a window WITHOUT the hub within 10 % of a mean that includes it, so the window
    property is asked of what can hold: the hub opens the launch (slot 0 - it is never in the tail), and every window beside it has the
    mean of the body beside it, 0."""
    e = _engine()
    cost = np.zeros(9375, np.int64)
    cost[4711] = 1 << 40
    order = e.tile_schedule(cost, 256, 1)
    check_permutation(order, cost.size)
    check_tail(order, cost, 256)
    assert order[0] == 4711
    assert window_deviation(order, cost, 256, leave_out=4711) == 0.0


def test_first_round_of_a_workgroup_spans_costs():
    """Wave w of workgroup b starts on slot w x grid + b: on the 300 k graph the eight first tiles of every workgroup have at least 3
    distinct costs (under the ascending order they are eight of the graph's lightest 2,048 tiles)."""
    e = _engine()
    cost = synthetic_costs()
    order = e.tile_schedule(cost, WAVES, 1)
    distinct = [np.unique(cost[order[np.arange(8) * CUS + b]]).size for b in range(CUS)]
    print(f'distinct first-round costs per workgroup: min {min(distinct)}')
    assert min(distinct) >= 3


def test_repeatable():
    e = _engine()
    cost = synthetic_costs()
    assert np.array_equal(e.tile_schedule(cost, WAVES, 1), e.tile_schedule(cost.copy(), WAVES, 1))


def test_bad_arguments_are_refused():
    e = _engine()
    with pytest.raises(ValueError): e.tile_schedule(np.ones(4), 0, 1)
    with pytest.raises(ValueError): e.tile_schedule(np.ones(4), 8, 2)
