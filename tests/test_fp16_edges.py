"""Piece format 2 (two fp16 pieces per fp32 operand, impl 2) at its edges: the device cut bit for bit, the range guard at every cut with exact
boundaries, which bodies it reads, the repeat's bookkeeping, and the branches of sharded and multi-loop runs.

The emulated cut (cut_pieces) is tied to the host packer on the CPU; everything else needs a GPU.  The nets are built so that every
expected value is exact: linear layers without BatchNormalization whose weights are identity blocks (powers of two) make each output one
product of pieces, and a zeroed weight column makes a unit's pre-activation equal to its bias."""
import numpy as np
import pytest

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs

UNDER = np.nextafter(np.float32(4094.0), np.float32(0.0))  # the largest fp32 whose 2^4 multiple stays below GNN_F16_LIMIT = 65,504


def _engine():
    from GNN import _engine
    return _engine


# ---- the emulated cut ----------------------------------------------------------------------------------------------------------------

def cut_pieces(x):
    """split_pair_f16 of gnn_fused_kernel.h in numpy: s = 2^4 x (exact), p0 = f16(s), p1 = f16(s - p0) (the difference is exact in fp32);
    numpy's float32 -> float16 conversion rounds to nearest even and keeps fp16 subnormals."""
    s = np.asarray(x, np.float32) * np.float32(16.0)
    p0 = s.astype(np.float16)
    p1 = (s - p0.astype(np.float32)).astype(np.float16)
    return p0, p1


def cut(x, times=1):
    """What an identity weight returns for the operand x after `times` cuts: (p0 + p1) / 2^4.  The fp32 sum is exact (p0 + p1 spans at most
    23 bits), and so is the device's: an identity weight is 2^14 in the layer's scale, its product with a piece is exact, and every MFMA adds
    one such product to an accumulator that started from a zero bias."""
    v = np.asarray(x, np.float32)
    for _ in range(times):
        p0, p1 = cut_pieces(v)
        v = (p0.astype(np.float32) + p1.astype(np.float32)) / np.float32(16.0)
    return v


def probe_values(rng):
    """Operands for the bit-exact probe, both signs and +-0: magnitudes 2^-30 .. just under 4,094, round-to-nearest-even ties in p0 and in
    p1, values whose p0 rounds into the next binade, values whose p1 is an fp16 subnormal.  Built in float64, exact in float32."""
    out = [np.exp2(rng.uniform(-30.0, np.log2(4094.0), 2000))]
    for e in range(-14, 16):                                       # 2^4 x in the fp16 binade [2^e, 2^(e+1))
        k = rng.integers(1024, 2046 if e == 15 else 2048, 8)
        out.append((k + 0.5) * 2.0 ** (e - 10) / 16)                # a tie in p0: halfway between two fp16 neighbours
        k = rng.integers(1024, 2046 if e == 15 else 2048, 8)
        if e == -14:                                               # (half an ulp of p0 is below the smallest fp16 subnormal)
            r = np.zeros(8)
        elif e >= -2:                                                # a tie in a normal p1: r = +-(m + 1/2) 2^(e - 22) < half an ulp of p0
            r = (rng.integers(1024, 2048, 8) + 0.5) * 2.0 ** (e - 22)
        else:                                                      # a tie in a subnormal p1: r = +-(m + 1/2) 2^-24
            r = (rng.integers(0, 2 ** (e + 13), 8) + 0.5) * 2.0 ** -24
        out.append((k * 2.0 ** (e - 10) + rng.choice([-1.0, 1.0], 8) * r) / 16)
        if e < 15:                                                 # p0 rounds up into the next binade (a tie to even, and above it)
            out.append(np.array([2.0 ** (e + 1) - 2.0 ** (e - 11), 2.0 ** (e + 1) - 2.0 ** (e - 12)]) / 16)
    out.append((rng.integers(0, 1024, 16) + 0.5) * 2.0 ** -28)     # ties among the fp16 subnormals of p0
    out.append(np.exp2(rng.uniform(-18.0, -7.0, 500)))             # p1 subnormal (2^4 |x| < 2^-3), p0 normal
    out.append(np.array([4093.0, 4093.99, float(UNDER)]))
    v = np.concatenate(out).astype(np.float32)
    v = np.where(np.abs(v) >= np.float32(4094.0), UNDER, v).astype(np.float32)
    return np.concatenate([v, -v, np.float32([0.0, -0.0])])


def test_emulated_cut_matches_host_packer():
    """The emulation is the production cut: gnn_split_f16 (the weight packer, the same round-to-nearest-even fp16 conversion) at exponent 4
    gives the same pieces bit for bit - at the exponent the packer picks itself for an array whose max lies in [2^10, 2^11), and at an
    explicit 4 over the whole probe set."""
    e = _engine()
    v = probe_values(np.random.default_rng(1))
    small = np.concatenate([v[np.abs(v) < 2000.0], np.float32([2000.0])])
    p0, p1, ex = e.split_f16(small)
    assert ex == 4
    q0, q1 = cut_pieces(small)
    assert np.array_equal(p0.view(np.uint16), q0.view(np.uint16)) and np.array_equal(p1.view(np.uint16), q1.view(np.uint16))
    p0, p1, _ = e.split_f16(v, exponent=4)
    q0, q1 = cut_pieces(v)
    assert np.array_equal(p0.view(np.uint16), q0.view(np.uint16)) and np.array_equal(p1.view(np.uint16), q1.view(np.uint16))
    sub = (q1 != 0) & (np.abs(q1.astype(np.float32)) < 2.0 ** -14)
    assert sub.sum() > 500 and np.all(np.isfinite(q0))             # the set reaches the subnormal p1 and never the fp16 overflow


def test_cut_precision_curve():
    """The precision the 2^4 activation scale gives (gnn_fused_kernel.h): p1 is an fp16 subnormal for every
    |x| < 2^-7 (2^4 |x| < 2^-3 leaves a remainder below 2^-14), where the cut keeps an ABSOLUTE error of at most 2^-29 (half the subnormal
    spacing 2^-24, unscaled); above, the relative error is at most 2^-23.  So: relative max(2^-23, 2^-29 / |x|) - 2^-19 at 1e-3, 2^-23 from
    2^-6 on - and never more than 2^-29 absolute below 2^-6, far inside the 1e-5 contract."""
    rng = np.random.default_rng(2)
    for lo in (1e-5, 1e-4, 1e-3, 2.0 ** -8, 2.0 ** -6, 0.1, 1.0, 1000.0):
        x = (lo * (1 + rng.random(100_000))).astype(np.float32)
        p0, p1 = cut_pieces(x)
        err = np.abs((p0.astype(np.float64) + p1.astype(np.float64)) / 16 - x.astype(np.float64))
        assert np.all(err <= np.maximum(2.0 ** -23 * np.abs(x), 2.0 ** -29))
        if 2 * lo <= 2.0 ** -7:
            assert np.all((p1 == 0) | (np.abs(p1.astype(np.float32)) < 2.0 ** -14))
    x = (1e-3 * (1 + rng.random(100_000))).astype(np.float32)
    _, p1 = cut_pieces(x)
    assert np.mean(np.abs(p1.astype(np.float32)) < 2.0 ** -14) > 0.99


# ---- graphs and nets -----------------------------------------------------------------------------------------------------------------

def _cycle_graph(rng, n, nl=1, al=1, mode='average', hub=None, hub_sources=()):
    """One cycle through nodes 0 .. n - 1 (or 0 .. n - 2 when `hub` = n - 1 is given: the hub has no out-arcs and takes its in-arcs from
    hub_sources).  Every other node has in-degree 1, so its aggregated columns are copies of its source's rows in any aggregation mode."""
    m = n - 1 if hub is not None else n
    perm = rng.permutation(m)
    src, dst = list(perm[np.r_[1:m, 0]]), list(perm)
    for s in hub_sources:
        src.append(s); dst.append(hub)
    lab = (2 * rng.random((len(src), al)) - 1)
    arcs = np.concatenate([np.stack([src, dst], 1).astype(np.float64), lab], 1)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))].astype(np.float32)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    return orc.make_graph_dict(arcs, nodes, mode)


def _csr_parts(g):
    arc_labels = np.asarray(g['arcs'], np.float32)[:, 2:]
    return g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], arc_labels[g['arcT'][1]]


def _device_graph(e, g):
    indptr, adj_src, adj_w, arc_w, arc_lab = _csr_parts(g)
    mask = np.logical_and(g['set_mask'], g['output_mask']).astype(np.uint8)
    return e.Graph(g['nodes'].shape[0], indptr, adj_src, adj_w, arc_w, arc_lab, g['nodes'], mask)


def _net(Ws, bs, act):
    w = []
    for W, b in zip(Ws, bs):
        w += [np.asarray(W, np.float32), np.asarray(b, np.float32)]
    return dict(weights=w, activations=[act] * len(Ws), batch_normalization=False)


def _identity_chain(ds, nl, al, hidden, act='linear', route='own'):
    """[state | nodes | agg state | agg nodes | agg arcs] -> hidden... -> ds.  Layer 0 copies the own state into units 0 .. ds - 1 and the
    aggregated state into units 64 .. 64 + ds - 1 (when hidden); hidden layers are identities; the last layer takes units 0 .. ds - 1
    (route 'own') or 64 .. (route 'agg').  Zero biases."""
    n_in = al + 2 * (ds + nl)
    dims = [n_in] + list(hidden) + [ds]
    Ws = [np.zeros((dims[i], dims[i + 1]), np.float32) for i in range(len(dims) - 1)]
    bs = [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)]
    i = np.arange(ds)
    Ws[0][i, i] = 1.0
    if hidden:
        Ws[0][ds + nl + i, 64 + i] = 1.0
        for W in Ws[1:-1]:
            W[np.arange(W.shape[0]), np.arange(W.shape[0])] = 1.0
        Ws[-1][i if route == 'own' else 64 + i, i] = 1.0
    return Ws, bs


def _loop(e, graph, st, ou, ds, max_it, thr, s0, impl=2, pieces=2, form=0):
    lp = e.Loop(graph, e.Mlp(st['weights'], st['activations'], st['batch_normalization']),
                e.Mlp(ou['weights'], ou['activations'], ou['batch_normalization']), ds, max_it, thr)
    assert lp.set_impl(impl) == impl
    if impl == 2:
        assert lp.set_pieces(pieces) == pieces
        if form:
            assert lp.set_tile_form(form) == form
    lp.set_state0(s0)
    return lp


def _run(e, g, st, ou, ds, max_it, thr, s0, impl=2, pieces=2, form=0):
    graph = _device_graph(e, g)
    lp = _loop(e, graph, st, ou, ds, max_it, thr, s0, impl, pieces, form)
    k = lp.run()
    res = (k, lp.state(), lp.output(), lp.range_info(), lp.gate_info())
    lp.close()
    graph.close()
    return res


def _same(a, b):
    """k, states and outputs bit-equal (NaN where the other has NaN)."""
    return a[0] == b[0] and np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)


def _mismatch(x, got, want):
    bad = got != want
    if not bad.any():
        return ''
    _, p1 = cut_pieces(x[bad])
    sub = int(np.sum((p1 != 0) & (np.abs(p1.astype(np.float32)) < 2.0 ** -14)))
    ex = ', '.join(f'{a!r}: {b!r} != {c!r}' for a, b, c in list(zip(x[bad], got[bad], want[bad]))[:6])
    return f'{int(bad.sum())} of {bad.size} differ ({sub} with a subnormal p1): {ex}'


# ---- 1. the device cut, bit for bit --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ds,n', [(64, 1280), (64, 1293), (40, 1607)])
def test_device_cut_is_the_emulated_cut(ds, n):
    """One body of [state ...] -> ds with an identity block on the own state: every state is (p0 + p1) / 2^4 of its s0, bit for bit -
    round to nearest even in both pieces, fp16 subnormals kept.  Ds = 64: the full-tile kernel (n = 1293: a partial last tile); Ds = 40:
    the generic layout, partial last tile."""
    e = _engine()
    rng = np.random.default_rng(10 + ds + n)
    g = _cycle_graph(rng, n)
    st = _net(*_identity_chain(ds, 1, 1, ()), 'linear')
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    v = probe_values(rng)
    assert v.size <= n * ds
    s0 = np.resize(rng.permutation(v), (n, ds)).astype(np.float32)
    k, s, _, rinfo, _ = _run(e, g, st, ou, ds, 1, 0.0, s0, form=1)
    assert k == 1 and rinfo == (False, 0)
    want = cut(s0)
    assert np.array_equal(s, want), _mismatch(s0, s, want)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['own', 'agg'])
@pytest.mark.parametrize('form', [1, 2])
def test_device_cut_through_hidden_layers(form, route):
    """[state | node | agg state | agg node | agg arc] -> 128 -> 128 -> 64, identity blocks: the own state runs through hidden units 0 - 63,
    the aggregated state (spmm over the graph) through units 64 - 127, so every 32-feature output tile of both hidden layers carries probe
    values; the last layer returns one of the two halves.  Every state is cut o cut o cut of its input, bit for bit, in both tile forms
    (the pair form: either wave's half)."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(20 + form)
    g = _cycle_graph(rng, n)
    st = _net(*_identity_chain(ds, 1, 1, (128, 128), route=route), 'linear')
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    s0 = np.resize(rng.permutation(probe_values(rng)), (n, ds)).astype(np.float32)
    x = s0 if route == 'own' else corc.spmm(g['adjT'], s0)
    k, s, _, rinfo, _ = _run(e, g, st, ou, ds, 1, 0.0, s0, form=form)
    assert k == 1 and rinfo == (False, 0)
    want = cut(x, 3)
    assert np.array_equal(s, want), _mismatch(x, s, want)


# ---- 2. the range guard at every cut -------------------------------------------------------------------------------------------------

def _guard_case(e, g, st, ou, ds, s0, form, max_it=1):
    """(format-2 run, format-3 run) of one Loop.  One body: with the identity nets a second body would cut the same values again, move no
    node robustly, and the certified gate would repeat the run on impl 1."""
    r2 = _run(e, g, st, ou, ds, max_it, 0.0, s0, pieces=2, form=form)
    r3 = _run(e, g, st, ou, ds, max_it, 0.0, s0, pieces=3, form=form)
    assert r3[3] == (False, 0)                                     # format 3 never trips
    return r2, r3


@pytest.mark.gpu
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('where', ['state', 'label', 'agg_state', 'agg_label', 'agg_arc'])
def test_layer0_guard_boundary(where, form):
    """Layer 0 cuts every column of the concat.  One offending row in the whole graph, the last (in a partial tile), which has no out-arcs:
    its own state or node label exactly 4,094 (2^4 x 4,094 = 65,504) trips the guard, the next fp32 below does not.  Aggregated columns,
    'sum' mode: the row is a hub over two sources whose state / label / arc label is 2,047 each - every input in range, the sum 4,094
    trips - or half the value below the limit.  A trip returns exactly format 3's k, states and outputs; no trip returns the emulated cut."""
    e = _engine()
    n, ds = 1293, 64
    hub = n - 1
    for trip in (True, False):
        rng = np.random.default_rng(30)
        g = _cycle_graph(rng, n, mode='sum', hub=hub, hub_sources=(3, 700))
        s0 = np.resize(rng.permutation(probe_values(rng)), (n, ds)).astype(np.float32)
        s0 = np.clip(s0, -1000.0, 1000.0)                          # the aggregated state of the cycle stays in range
        val = np.float32(4094.0) if trip else UNDER
        half = np.float32(2047.0) if trip else np.float32(UNDER / 2)
        if where == 'state':
            s0[hub, 5] = val
        elif where == 'label':
            g['nodes'][hub, 0] = val
        elif where == 'agg_state':
            s0[[3, 700], 9] = half
        elif where == 'agg_label':
            g['nodes'][[3, 700], 0] = half
        else:
            into = np.asarray(g['arcs'])[:, 1] == hub
            g['arcs'][into, 2] = half
        st = _net(*_identity_chain(ds, 1, 1, (128,)), 'linear')
        ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
        r2, r3 = _guard_case(e, g, st, ou, ds, s0, form)
        if trip:
            assert r2[3] == (True, 1) and _same(r2, r3), where
        else:
            assert r2[3] == (False, 0), where
            assert np.array_equal(r2[1], cut(s0, 2)), where


def _hidden_probe_net(ds, layer, unit, v, act):
    """3-layer identity chain; unit `unit` of hidden layer `layer` (1: after layer 0, 2: after layer 1) has a zero input column and bias v,
    and the last layer returns it in column unit % 64."""
    Ws, bs = _identity_chain(ds, 1, 1, (128, 128))
    j0 = unit % 64
    if unit >= 64:
        Ws[2][j0, j0] = 0.0
        Ws[2][unit, j0] = 1.0
    Ws[layer - 1][:, unit] = 0.0
    bs[layer - 1][unit] = v
    return _net(Ws, bs, act), j0


@pytest.mark.gpu
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('unit', [5, 40, 70, 100])
@pytest.mark.parametrize('layer', [1, 2])
def test_hidden_guard_boundary(layer, unit, form):
    """The hidden layers' guard (hidden_range of k_fused / pair_cut): one unit's pre-activation is its bias, exactly 4,094 (trips) or the
    fp32 below (does not), placed in each 32-feature output tile in turn - in the pair form in either wave's half - after hidden layer 1
    and after hidden layer 2.  Both forms agree on the repeat; the repeat is format 3; without one the result is the emulated chain."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(40)
    g = _cycle_graph(rng, n)
    s0 = np.resize(rng.permutation(probe_values(rng)), (n, ds)).astype(np.float32)
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    for v, trip in ((np.float32(4094.0), True), (UNDER, False)):
        st, j0 = _hidden_probe_net(ds, layer, unit, v, 'linear')
        r2, r3 = _guard_case(e, g, st, ou, ds, s0, form, max_it=1)
        if trip:
            assert r2[3] == (True, 1) and _same(r2, r3)
        else:
            want = cut(s0, 3)
            want[:, j0] = cut(np.full(n, v, np.float32), 3 - layer)
            assert r2[3] == (False, 0) and np.array_equal(r2[1], want)


@pytest.mark.gpu
@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('act,v,trip', [('linear', 4094.0, True), ('linear', float(UNDER), False), ('relu', 4094.0, True),
                                        ('relu', float(UNDER), False), ('elu', 4094.0, True), ('elu', float(UNDER), False),
                                        ('selu', 3000.0, True), ('selu', 2600.0, False), ('selu', -1e6, True),
                                        ('tanh', 1e6, True), ('tanh', -1e6, True), ('sigmoid', 1e6, True), ('sigmoid', -1e6, True)])
def test_activation_guard(act, v, trip, form):
    """The bound the hidden guard takes is max |accumulator| 2^4, before the activation.  linear / relu / elu pass a positive pre-activation
    unchanged: 4,094 trips, the fp32 below does not (then the emulated chain holds).  The folded SELU hands log2(e) v to the cut, so its
    limit is 65,504 / (2^4 log2 e) = 2,837.8: 3,000 trips although 2^4 x 3,000 < 65,504; 2,600 does not (nor does the next hidden layer's
    2,600 x 1.0507 = 2,731.8).  tanh / sigmoid / selu at +-1e6:
    the operand is small but the bound is conservative - it trips and returns exactly format 3.  Unit 100: tile 3, the pair's second wave."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(50)
    g = _cycle_graph(rng, n)
    s0 = np.abs(np.resize(rng.permutation(probe_values(rng)), (n, ds))).astype(np.float32)
    s0 = np.minimum(s0, np.float32(1.0))                           # every activation is the identity on [0, 1] except the selu / tanh family
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    st, j0 = _hidden_probe_net(ds, 1, 100, np.float32(v), act)
    r2, r3 = _guard_case(e, g, st, ou, ds, s0, form, max_it=1)
    if trip:
        assert r2[3] == (True, 1) and _same(r2, r3)
        return
    assert r2[3] == (False, 0)
    if act == 'selu':
        # three layers, each: weight image and operand cut relative <= 2^-23 each, the dropped p1 q1 <= 2^-22, an operand's absolute
        # <= 2^-29 below 2^-6 (test_cut_precision_curve); format 3's own error is smaller.  2^-19 relative + 2^-26 absolute covers it.
        assert np.all(np.abs(r2[1] - r3[1]) <= 2.0 ** -19 * np.abs(r3[1]) + 2.0 ** -26)
    else:
        want = cut(s0, 3)
        want[:, j0] = cut(np.full(n, v, np.float32), 2)
        assert np.array_equal(r2[1], want)


# ---- 3. which bodies the guard reads ------------------------------------------------------------------------------------------------

def _doubling(ds=64, self_w=2.0, rest=None):
    Ws, bs = _identity_chain(ds, 1, 1, ())
    Ws[0] *= np.float32(self_w)
    if rest is not None:
        Ws[0][np.arange(1, ds), np.arange(1, ds)] = rest
    return _net(Ws, bs, 'linear')


@pytest.mark.gpu
@pytest.mark.parametrize('max_it,thr,trip,value,k', [(3, 0.0, False, 8000.0, 3), (4, 0.0, True, None, 4), (4, 1.5, False, 2000.0, 1)])
def test_guard_reads_the_bodies_that_ran(max_it, thr, trip, value, k):
    """W = 2 I on the own state, s0 = 1,000: body b cuts 1,000 x 2^b (exact in every format).  Three bodies cut up to 4,000 and return 8,000
    exactly - no repeat; a fourth cuts 8,000 (2^4 x 8,000 > 65,504): the trip is in the LAST body that ran and must be seen.  A threshold
    of 1.5 closes the gate after body 0 (every later body ratio is exactly 1): the body that would trip never runs, no repeat."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(60)
    g = _cycle_graph(rng, n)
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    s0 = np.full((n, ds), 1000.0, np.float32)
    r2 = _run(e, g, _doubling(), ou, ds, max_it, thr, s0)
    assert r2[0] == k
    if trip:
        r3 = _run(e, g, _doubling(), ou, ds, max_it, thr, s0, pieces=3)
        assert r2[3] == (True, 1) and _same(r2, r3)
    else:
        assert r2[3] == (False, 0) and np.all(r2[1] == value)


@pytest.mark.gpu
def test_guard_trips_in_a_later_body():
    """A run that looks contractive - every state column shrinks by half each body - except one value of one row (in the partial last tile)
    that doubles from 1,000: in range for bodies 0 - 2, out of range from body 3 on.  The repeat returns exactly format 3."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(61)
    g = _cycle_graph(rng, n)
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    s0 = (0.5 * rng.standard_normal((n, ds))).astype(np.float32)
    s0[:, 0] = 0.0
    s0[n - 1, 0] = 1000.0
    st = _doubling(rest=0.5)
    r2 = _run(e, g, st, ou, ds, 6, 0.0, s0)
    r3 = _run(e, g, st, ou, ds, 6, 0.0, s0, pieces=3)
    assert r2[3] == (True, 1) and _same(r2, r3) and r3[0] == 6
    r2 = _run(e, g, st, ou, ds, 3, 0.0, s0)                      # three bodies: 4,000 is the largest value cut
    assert r2[3] == (False, 0) and r2[1][n - 1, 0] == 8000.0


# ---- 4. bookkeeping of the repeat ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_repeat_leaves_the_loop_in_format_2():
    """A tripping run, then (set_state0) an in-range run on the same Loop: range_info (True, 1), then (False, 1); the second run is bit-equal
    to a fresh format-2 Loop - and differs from format 3 - so the repeat did not leave the Loop in format 3."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(70)
    g = _cycle_graph(rng, n)
    ou = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    st = _doubling()
    big = np.full((n, ds), 1000.0, np.float32)
    small = np.clip(np.resize(rng.permutation(probe_values(rng)), (n, ds)), -200.0, 200.0).astype(np.float32)
    graph = _device_graph(e, g)
    lp = _loop(e, graph, st, ou, ds, 4, 0.0, big)
    k = lp.run()
    assert lp.range_info() == (True, 1) and k == 4 and np.all(lp.state() == 16000.0)
    lp.set_state0(small)
    k = lp.run()
    second = (k, lp.state(), lp.output())
    assert lp.range_info() == (False, 1)
    lp.close()
    graph.close()
    fresh2 = _run(e, g, st, ou, ds, 4, 0.0, small)
    fresh3 = _run(e, g, st, ou, ds, 4, 0.0, small, pieces=3)
    assert _same(second, fresh2)
    assert not np.array_equal(second[1], fresh3[1])


@pytest.mark.gpu
def test_range_repeat_then_certified_gate_repeat():
    """A node label of 1e5 trips the guard in every body, and the threshold sits on the exact chain's largest distance / norm ratio of body
    4 (as in test_sharded_default_path_certified_gate): the format-3 repeat has a gate with a borderline node and no robust mover, so it is
    itself repeated on impl 1.  k, states and outputs bit-equal to the C oracle; range_info and gate_info both report it."""
    e = _engine()
    n, d = 1500, 64
    rng = np.random.default_rng(77)
    g = orc.make_graph_dict(random_arcs(rng, n, 4 * n, 1), (2 * rng.random((n, 3)) - 1).astype(np.float32), 'average')
    g['nodes'][n // 2, 1] = 1e5
    st = make_mlp(rng, 1 + 2 * (d + 3), [128, 128, d], 'tanh', gain=0.5, bn_random=True)
    ou = make_mlp(rng, d + 3, [2], 'softmax', bn_random=True)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    _, s3, _ = corc.loop_node(g, st, ou, d, 3, 0.0, s0)
    _, s4, _ = corc.loop_node(g, st, ou, d, 4, 0.0, s0)
    dist = np.zeros(n, np.float32); nrm = np.zeros(n, np.float32)
    for c in range(d):
        df = s4[:, c] - s3[:, c]
        dist = dist + df * df
        nrm = nrm + s3[:, c] * s3[:, c]
    thr = float(np.max(np.sqrt(dist) / np.sqrt(nrm)))
    kc, sc, oc = corc.loop_node(g, st, ou, d, 12, thr, s0)
    k, s, o, rinfo, ginfo = _run(e, g, st, ou, d, 12, thr, s0)
    assert rinfo == (True, 1) and ginfo == (True, 1)
    assert k == kc and np.array_equal(s, sc) and np.array_equal(o, oc)


@pytest.mark.gpu
def test_nan_does_not_trip_and_inf_does():
    """a NaN operand does not trip the guard (the running max ignores it) - the NaN rows are the exact path's, the
    rest within the 1e-5 contract; an infinity does, and the repeat is exactly format 3 (NaNs included)."""
    e = _engine()
    n, ds = 1293, 64
    rng = np.random.default_rng(80)
    g = _cycle_graph(rng, n, nl=3)
    st = make_mlp(rng, 1 + 2 * (ds + 3), [128, 128, ds], 'selu', gain=0.6, bn_random=True)
    ou = make_mlp(rng, ds + 3, [2], 'softmax', bn_random=True)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    g['nodes'][n - 1, 1] = np.nan
    r2 = _run(e, g, st, ou, ds, 4, 0.0, s0)
    r1 = _run(e, g, st, ou, ds, 4, 0.0, s0, impl=1)
    assert r2[3] == (False, 0) and r2[0] == r1[0] == 4
    nan = np.isnan(r1[1])
    assert nan.any() and np.array_equal(np.isnan(r2[1]), nan) and np.array_equal(np.isnan(r2[2]), np.isnan(r1[2]))
    assert np.max(np.abs(r2[1][~nan] - r1[1][~nan])) < 1e-5
    g['nodes'][n - 1, 1] = np.inf
    r2 = _run(e, g, st, ou, ds, 4, 0.0, s0)
    r3 = _run(e, g, st, ou, ds, 4, 0.0, s0, pieces=3)
    assert r2[3] == (True, 1) and _same(r2, r3)


# ---- 5. ranks and multi-loop entry points --------------------------------------------------------------------------------------------

def last_rank_trip_case(seed, n, world, d=64):
    """A sharded case whose only out-of-range operand is one node label on the LAST rank: 5,000 (2^4 x 5,000 > 65,504) on a row whose
    out-neighbours average it with at least one other label (so no other row, on any rank, aggregates it past 4,094).  net_state's
    weights on the node-label columns are zero, so the label changes nothing but the guard: every body trips on that rank only."""
    import test_gpu_sharded as S
    e = _engine()
    g, st, ou, s0 = S._case(seed, n, d, hidden=(128, 128))
    nl = g['nodes'].shape[1]
    st['weights'][0][d:d + nl] = 0.0
    st['weights'][0][2 * d + nl:2 * d + 2 * nl] = 0.0
    indptr, adj_src = np.asarray(g['adjT'][0]), np.asarray(g['adjT'][1])
    indeg = np.diff(indptr)
    rb_last, _ = e.shard_range(n, world - 1, world)
    dst_of = np.repeat(np.arange(n), indeg)
    row = next(r for r in range(n - 1, rb_last - 1, -1) if np.all(indeg[dst_of[adj_src == r]] >= 2))
    g['nodes'][row, 0] = 5000.0
    agg = corc.spmm(g['adjT'], g['nodes'])
    off = np.flatnonzero((np.abs(g['nodes']) >= 4094.0).any(1) | (np.abs(agg) >= 4094.0).any(1))
    assert off.size and off.min() >= rb_last
    return g, st, ou, s0


@pytest.mark.gpu
@pytest.mark.parametrize('world,layout', [(2, 'whole'), (3, 'whole'), (2, 'halo'), (3, 'halo'), (2, 'slice'), (4, 'slice')])
def test_sharded_range_repeat_when_only_the_last_rank_trips(world, layout):
    """Loopback groups: the offending rows belong to the last rank alone, the repeat is decided from the exchanged word 3 - every rank reports
    it, and k, states and outputs are bit-equal to the same group in format 3 and to the unsharded format-3 run."""
    import test_gpu_sharded as S
    e = _engine()
    n, d = 1500, 64
    g, st, ou, s0 = last_rank_trip_case(90 + world, n, world)
    indptr, adj_src, adj_w, _, _ = S._csr_parts(g)

    def group(pieces):
        comms, graphs, loops, ranges = S._sharded_loops(e, g, st, ou, d, 6, 0.0, s0, world, 2, halo=layout == 'halo')
        for gr, lp in zip(graphs, loops):
            lp.set_pieces(pieces)
            if layout == 'slice':
                gr.set_full_adjacency(n, indptr, adj_src, adj_w)
                lp.set_slice_exchange(True)
        k = e.Loop.run_group(loops)
        state, out = S._collect(loops, ranges, None)
        info = [lp.range_info() for lp in loops]
        for lp in loops: lp.close()
        for c in comms: c.close()
        return (k, state, out), info

    r2, info2 = group(2)
    r3, info3 = group(3)
    assert info2 == [(True, 1)] * world and info3 == [(False, 0)] * world
    assert _same(r2, r3)
    ru = _run(e, g, st, ou, d, 6, 0.0, s0, pieces=3)
    assert _same(r2, ru[:3])


@pytest.mark.gpu
def test_run_many_repeats_only_the_tripping_loop():
    """Loop.run_many with one tripping fused Loop among persistent small ones: every Loop's k, states and outputs as if run alone, and only
    the tripping Loop counts a repeat."""
    import test_gpu_sharded as S
    e = _engine()
    n, d = 1293, 64
    g, st, ou, s0 = last_rank_trip_case(95, n, 1)
    smalls = [S._case(96 + i, 300 + 37 * i, 8, hidden=(16,)) for i in range(2)]

    def make(case, ds, pieces=2, persistent=False):
        gc, stc, ouc, s0c = case
        graph = _device_graph(e, gc)
        lp = e.Loop(graph, e.Mlp(stc['weights'], stc['activations'], True), e.Mlp(ouc['weights'], ouc['activations'], True), ds, 8, 0.0)
        lp.set_pieces(pieces)
        assert lp.set_persistent(persistent) == persistent
        lp.set_state0(s0c)
        return graph, lp

    made = [make(smalls[0], 8, persistent=True), make((g, st, ou, s0), d), make(smalls[1], 8, persistent=True)]
    ks = e.Loop.run_many([lp for _, lp in made])
    got = [(k, lp.state(), lp.output(), lp.range_info()) for k, (_, lp) in zip(ks, made)]
    alone = []
    for case, ds, pieces, pers in ((smalls[0], 8, 2, True), ((g, st, ou, s0), d, 3, False), (smalls[1], 8, 2, True)):
        graph, lp = make(case, ds, pieces, pers)
        alone.append((lp.run(), lp.state(), lp.output()))
        lp.close(); graph.close()
    for graph, lp in made:
        lp.close(); graph.close()
    assert [x[3] for x in got] == [(False, 0), (True, 1), (False, 0)]
    for a, b in zip(got, alone):
        assert _same(a, b)


@pytest.mark.gpu
def test_lgnn_stack_repeats_the_layer_whose_labels_trip():
    """Loop.lgnn_run: layer 1's last bias puts its state column 0 at 5,000 after its only body (never cut there: no trip), so layer 2, whose
    node labels carry layer 1's state, trips in every body.  Layer 1 is exact in both formats (identity chain, states k / 1024), so the
    stack is bit-equal to the same stack with every Loop in format 3, and only layer 2 counts a repeat."""
    e = _engine()
    n, ds = 1293, 32
    rng = np.random.default_rng(97)
    g = _cycle_graph(rng, n)
    Ws, bs = _identity_chain(ds, 1, 1, (128,))
    Ws[1][:, 0] = 0.0
    bs[1][0] = 5000.0
    st0 = _net(Ws, bs, 'relu')
    ou0 = make_mlp(rng, ds + 1, [2], 'linear', batch_normalization=False)
    nl1 = 1 + ds
    st1 = make_mlp(rng, 1 + 2 * (ds + nl1), [128, ds], 'relu', batch_normalization=False, gain=0.6)
    ou1 = make_mlp(rng, ds + nl1, [2], 'linear', batch_normalization=False)
    s0 = [(rng.integers(-1024, 1025, (n, ds)) / 1024).astype(np.float32), (0.1 * rng.standard_normal((n, ds))).astype(np.float32)]

    def stack(pieces):
        base = _device_graph(e, g)
        derived = base.derive(ds)
        loops = []
        for gr, (st, ou), max_it, s in zip((base, derived), ((st0, ou0), (st1, ou1)), (1, 3), s0):
            loops.append(_loop(e, gr, st, ou, ds, max_it, 0.0, s, pieces=pieces))
        K = e.Loop.lgnn_run(loops, [base, derived], True, False)
        res = [(K[i], lp.state(), lp.output(), lp.range_info()) for i, lp in enumerate(loops)]
        for lp in loops: lp.close()
        derived.close(); base.close()
        return res

    a, b = stack(2), stack(3)
    assert [x[3] for x in a] == [(False, 0), (True, 1)]
    assert np.all(a[0][1][:, 0] == 5000.0)
    for x, y in zip(a, b):
        assert _same(x, y)
