"""Inputs and expectations of tests/test_gpu_fp16_forms.py and tests/test_fp16_form_cases_host.py (no test in here): piece format 2 (two fp16
pieces per fp32 operand, impl 2) in the fused forms that tests/test_fp16_edges.py does not reach - k_fused_generic with hidden layers in its
four tile pairs, the wide-state form, the seeded kernels of the label projection, the kernels for a last layer with its own activation.

Every net is an identity chain: weights 0, 1 or 0.5, at most one weight per output unit, a bias only on a unit without input.  Every product
is then exact in every format, and what a Loop body returns is `cut` (test_fp16_edges) applied once per layer that cuts the value, bit for
bit.  `emulate` is that chain in numpy; it also returns what every range guard of the body reads - layer 0: the scaled operands themselves
(split_pair_f16), hidden layers: the accumulators, i.e. the pre-activations, times log2(e) under the folded SELU (hidden_range) - so that the
host tests can assert that the inputs, not the kernel, decide each verdict: no operand at 4,094 where no repeat is expected, exactly one,
at the intended cut, where one is.

A case is a dict(g, st, ou, s0, ds, seeded, bodies, trip: the cut whose guard must trip or None, want: the expected states or None, x: the
value each state element was cut from (for messages), count: how many operands reach the limit at the cut `trip` - one, or one unit's on
every row where a bias puts it there).  Nobody writes to a case after it is built."""
import numpy as np

from oracle import c_oracle as corc
from oracle import gnn_oracle as orc
from test_fp16_edges import UNDER, _cycle_graph, _net, cut, probe_values
from util import make_mlp

LIMIT = np.float32(4094.0)               # 2^4 x 4,094 = 65,504 = GNN_F16_LIMIT
LOG2E = 1.44269504088896341
N = 413                                  # 12 full tiles and a last tile of 29 rows; N x 16 covers the probe set
ROWS = dict(full=40, partial=N - 1)      # the offending row: in a full tile (tile 1), in the partial last tile
SOURCES = (3, 200)                       # the two in-neighbours of a hub
COL = dict(state=5, label=0, agg_state=9, agg_label=0, agg_arc=0)      # the offending column inside its block
WHERES = ('state', 'label', 'agg_state', 'agg_label', 'agg_arc')


def _row(name, kind, ds, hidden, tiles, kernel=1, waves=8, nl=1, al=1, acts=None, proj='off', wide='off', seeded=False):
    acts = list(acts) if acts else ['linear'] * (len(hidden) + 1)
    return dict(id=name, kind=kind, ds=ds, hidden=tuple(hidden), tiles=tiles, kernel=kernel, waves=waves, nl=nl, al=al, acts=acts, proj=proj,
                wide=wide, seeded=seeded)


# kind: G k_fused_generic, W wide-state form, S seeded (label projection), M a last layer with its own activation.  tiles: (NT, NTL) of the
# instantiation (of the shadow net over [state | aggregated state] when seeded); kernel: 1 k_fused_generic, 2 k_fused_full; waves per workgroup.
FORMS = [
    _row('G11-24-h32', 'G', 24, (32,), (1, 1)),
    _row('G11-24-h32-32', 'G', 24, (32, 32), (1, 1)),
    _row('G22-40-h48', 'G', 40, (48,), (2, 2)),                               # a padded second hidden tile
    _row('G22-40-h64-64', 'G', 40, (64, 64), (2, 2)),
    _row('G42-16-h128', 'G', 16, (128,), (4, 2)),                             # NTL bumped from 1 to 2
    _row('G42-40-h128-128', 'G', 40, (128, 128), (4, 2)),
    _row('G22-40-one-layer', 'G', 40, (), (2, 2)),
    _row('W4-128-h128', 'W', 128, (128,), (4, 4), waves=4, wide='always'),
    _row('W5-96-h128-128', 'W', 96, (128, 128), (4, 4), waves=5, wide='always'),
    _row('W5-100-h128', 'W', 100, (128,), (4, 4), waves=5, wide='always'),     # a last feature tile of 4 columns
    _row('W7-76-one-layer', 'W', 76, (), (4, 4), waves=7, wide='always'),
    _row('S-full-h128-nl1', 'S', 64, (128,), (4, 2), kernel=2, proj='always', seeded=True),
    _row('S-full-h128-128-nl1', 'S', 64, (128, 128), (4, 2), kernel=2, proj='always', seeded=True),
    _row('S-full-h128-nl40', 'S', 64, (128,), (4, 2), kernel=2, nl=40, proj='auto', seeded=True),
    _row('S-full-h128-128-nl40', 'S', 64, (128, 128), (4, 2), kernel=2, nl=40, proj='auto', seeded=True),
    _row('S-generic-40-h128-nl60', 'S', 40, (128,), (4, 2), nl=60, proj='auto', seeded=True),
    _row('S-wide-128-h128-128-nl40', 'S', 128, (128, 128), (4, 4), waves=4, nl=40, proj='auto', wide='always', seeded=True),
    _row('S-generic-40-one-layer-nl1', 'S', 40, (), (2, 2), proj='always', seeded=True),
    _row('M-full-relu-linear', 'M', 64, (128,), (4, 2), kernel=2, acts=('relu', 'linear')),
    _row('M-full-linear-linear-relu', 'M', 64, (128, 128), (4, 2), kernel=2, acts=('linear', 'linear', 'relu')),
    _row('M-generic-relu-linear', 'M', 40, (128,), (4, 2), acts=('relu', 'linear')),
    _row('M-generic-linear-linear-relu', 'M', 40, (128, 128), (4, 2), acts=('linear', 'linear', 'relu')),
]
BY_ID = {r['id']: r for r in FORMS}
ACTIVATION_FORMS = ('G42-40-h128-128', 'W5-96-h128-128')
BOOKKEEPING_FORMS = ('W4-128-h128', 'S-full-h128-nl1')
SHARDED_FORM = 'W4-128-h128'
# test_fp16_edges.test_activation_guard's table; selu at 3,000: k_fused_generic (both forms here are its instantiations) starts the hidden
# accumulators from weights and a bias folded with log2(e) (gnn_fused_pack, fused_stage_vectors) and hidden_range reads those accumulators, so
# the guard sees log2(e) x 3,000 = 4,328 >= 4,094: it trips
ACTIVATIONS = [('linear', 4094.0, True), ('linear', float(UNDER), False), ('relu', 4094.0, True), ('relu', float(UNDER), False),
               ('elu', 4094.0, True), ('elu', float(UNDER), False), ('selu', 3000.0, True), ('selu', 2600.0, False), ('selu', -1e6, True),
               ('tanh', 1e6, True), ('tanh', -1e6, True), ('sigmoid', 1e6, True), ('sigmoid', -1e6, True)]


def concat_width(row):
    return row['al'] + 2 * (row['ds'] + row['nl'])


def dims_of(row, shadow=False):
    return [2 * row['ds'] if shadow else concat_width(row)] + list(row['hidden']) + [row['ds']]


def hidden_units(row):
    """(hidden layer, unit) with one unit in every 32-feature tile of every hidden layer: 5, 40 (the padded tile of a 48-wide layer), 70, 100."""
    return [(layer, u) for layer, width in enumerate(row['hidden'], 1) for u in (5, 40, 70, 100) if u < width]


# ---- nets ------------------------------------------------------------------------------------------------------------------------------------

def identity_chain(ds, nl, al, hidden, route='own'):
    """[state | nodes | agg state | agg nodes | agg arcs] -> hidden... -> ds: layer 0 copies the own state (route 'own') or the aggregated state
    ('agg') into units 0 .. ds - 1, hidden layers are identity blocks, the last layer takes units 0 .. ds - 1.  Zero biases."""
    assert not hidden or min(hidden) >= ds
    dims = [al + 2 * (ds + nl)] + list(hidden) + [ds]
    Ws = [np.zeros((dims[i], dims[i + 1]), np.float32) for i in range(len(dims) - 1)]
    bs = [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)]
    i = np.arange(ds)
    Ws[0][i if route == 'own' else ds + nl + i, i] = 1.0
    for W in Ws[1:]:
        k = np.arange(min(W.shape))
        W[k, k] = 1.0
    return Ws, bs


def probe_unit(row, Ws, bs, layer, unit, v):
    """Unit `unit` of hidden layer `layer` gets a zero input column and the bias v; a following hidden layer takes it with weight 0.5 (its own
    pre-activation stays out of the guard's way), the last layer returns it in state column unit % ds.  Returns that column."""
    ds, L = row['ds'], len(Ws)
    Ws[layer - 1][:, unit] = 0.0
    bs[layer - 1][unit] = v
    if layer < L - 1: Ws[layer][unit, unit] = 0.5
    j0 = unit % ds
    Ws[-1][:, j0] = 0.0
    Ws[-1][unit, j0] = 1.0
    return j0


def _out_net(rng, row):
    return make_mlp(rng, row['ds'] + row['nl'], [2], 'linear', batch_normalization=False)


def _state_net(row, Ws, bs, acts=None):
    st = _net(Ws, bs, 'linear')
    st['activations'] = list(acts or row['acts'])
    return st


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------------

def graph(rng, n, nl, al, mode='average', hub=None, hub_sources=()):
    """test_fp16_edges._cycle_graph with the hub anywhere: one cycle through every node but the hub, which has no out-arcs and takes its in-arcs
    from hub_sources.  Every other node has in-degree 1: its aggregated columns are copies of its source's rows in any aggregation mode."""
    if hub is None or hub == n - 1: return _cycle_graph(rng, n, nl, al, mode, hub, hub_sources)
    perm = rng.permutation(np.delete(np.arange(n), hub))
    src, dst = list(perm[np.r_[1:n - 1, 0]]), list(perm)
    for s in hub_sources:
        src.append(s); dst.append(hub)
    lab = 2 * rng.random((len(src), al)) - 1
    arcs = np.concatenate([np.stack([src, dst], 1).astype(np.float64), lab], 1)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))].astype(np.float32)
    return orc.make_graph_dict(arcs, (2 * rng.random((n, nl)) - 1).astype(np.float32), mode)


def concat(g, s0):
    """[state | nodes | agg state | agg nodes | agg arcs] in fp32, aggregated by the engine's own chains (the C oracle's)."""
    nodes = np.asarray(g['nodes'], np.float32)
    return np.concatenate([np.asarray(s0, np.float32), nodes, corc.spmm(g['adjT'], np.asarray(s0, np.float32)), corc.spmm(g['adjT'], nodes),
                           corc.spmm(g['arcT'], np.asarray(g['arcs'], np.float32)[:, 2:])], axis=1)


def block_start(row, where):
    ds, nl = row['ds'], row['nl']
    return dict(state=0, label=ds, agg_state=ds + nl, agg_label=2 * ds + nl, agg_arc=2 * ds + 2 * nl)[where]


# ---- the chain in numpy ----------------------------------------------------------------------------------------------------------------------

def _act(name, v):
    v = np.asarray(v, np.float64)
    with np.errstate(over='ignore'):
        if name == 'linear': return v
        if name == 'relu': return np.maximum(v, 0.0)
        if name == 'elu': return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
        if name == 'selu': return 1.0507009873554805 * np.where(v > 0, v, 1.6732632423543772 * np.expm1(np.minimum(v, 0.0)))
        if name == 'tanh': return np.tanh(v)
        if name == 'sigmoid': return 1.0 / (1.0 + np.exp(-v))
    raise ValueError(name)


def emulate(case):
    """(states after case['bodies'] bodies, {cut: what its guard reads}) with cuts named 'b<body>.layer0', 'b<body>.hidden<l>'.  Exact (bit for
    bit the device's) wherever every activation met is the identity on the values it sees; the guard magnitudes are exact for linear / relu / elu
    and rounded for the others."""
    st, ds, g = case['st'], case['ds'], case['g']
    Ws, bs, acts = st['weights'][0::2], st['weights'][1::2], st['activations']
    L = len(Ws)
    nl = np.asarray(g['nodes']).shape[1]
    fold = LOG2E if L > 1 and acts[0] == 'selu' else 1.0
    state, ops = np.asarray(case['s0'], np.float32), {}
    for body in range(case['bodies']):
        x = concat(g, state)
        is_label = np.ones(x.shape[1], bool)
        is_label[:ds] = False
        is_label[ds + nl:2 * ds + nl] = False
        uncut = is_label if case['seeded'] else np.zeros(x.shape[1], bool)      # the label projection takes the label columns in fp32
        ops[f'b{body}.layer0'] = np.abs(x[:, ~uncut])
        a = x
        for l in range(L):
            W, b = np.asarray(Ws[l]), np.asarray(bs[l])
            with np.errstate(over='ignore', invalid='ignore'): c = cut(a)      # (past the limit the pieces are infinite: such a run is repeated)
            h = np.empty((a.shape[0], W.shape[1]), np.float32)
            for j in range(W.shape[1]):
                k = np.flatnonzero(W[:, j])
                assert k.size <= 1 and (k.size == 0 or (b[j] == 0 and W[k[0], j] in (0.5, 1.0))), 'one exact product or one bias per unit'
                if k.size == 0: h[:, j] = b[j]
                else: h[:, j] = (a if l == 0 and uncut[k[0]] else c)[:, k[0]] * W[k[0], j]
            if l < L - 1: ops[f'b{body}.hidden{l + 1}'] = np.abs(h.astype(np.float64)) * fold
            a = _act(acts[l], h).astype(np.float32)
        state = a
    return state, ops


def reaching(ops):
    """{cut: (operands at or past the limit, columns that hold one)} over the cuts that have one."""
    big = {name: v >= float(LIMIT) for name, v in ops.items()}
    return {name: (int(b.sum()), int(b.any(0).sum())) for name, b in big.items() if b.any()}


def _finish(row, rng, g, Ws, bs, s0, trip, x=None, bodies=1, seeded=None, acts=None, exact=True, count=1):
    case = dict(row=row, g=g, st=_state_net(row, Ws, bs, acts), ou=_out_net(rng, row), s0=np.ascontiguousarray(s0, np.float32), ds=row['ds'],
                seeded=row['seeded'] if seeded is None else seeded, bodies=bodies, trip=trip, x=x, count=count)
    case['want'] = emulate(case)[0] if trip is None and exact else None
    return case


def _probe_state(rng, row, n=N, limit=None):
    """The probe set of test_fp16_edges dealt over [n, ds]; non-negative where an activation other than linear must stay the identity."""
    v = probe_values(rng)
    assert v.size <= n * row['ds']
    s0 = np.resize(rng.permutation(v), (n, row['ds'])).astype(np.float32)
    if limit is not None: s0 = np.clip(s0, -limit, limit)
    if row['kind'] == 'M': s0 = np.abs(s0)
    return s0


# ---- 1. the chain ----------------------------------------------------------------------------------------------------------------------------

def chain_case(row, route):
    """One body over the probe set, through the own state or the aggregated state ('average' over a cycle: a copy of the source's row).  Every
    probe value lies below 4,094 and an identity chain never grows one: no operand reaches the limit at any cut.  A seeded form carries two
    fp32 label terms on top: node label 0 into state column ds - 1 and aggregated arc label 0 into column ds - 2, in place of the state."""
    ds, nl = row['ds'], row['nl']
    rng = np.random.default_rng(1000 + FORMS.index(row) * 2 + (route == 'agg'))
    g = graph(rng, N, nl, row['al'])
    Ws, bs = identity_chain(ds, nl, row['al'], row['hidden'], route)
    s0 = _probe_state(rng, row)
    x = s0 if route == 'own' else corc.spmm(g['adjT'], s0)
    if row['seeded']:
        x = x.copy()
        for j, k in ((ds - 1, ds), (ds - 2, 2 * ds + 2 * nl)):
            Ws[0][:, j] = 0.0
            Ws[0][k, j] = 1.0
            x[:, j] = concat(g, s0)[:, k]
    return _finish(row, rng, g, Ws, bs, s0, None, x)


# ---- 2. layer 0 ------------------------------------------------------------------------------------------------------------------------------

def layer0_case(row, where, pos, at_limit):
    """One offending operand in the whole graph, on a hub without out-arcs ('sum' mode): its own state or node label is 4,094 (or the fp32
    below), or its two sources carry 2,047 (or half the fp32 below 4,094) in a state column, a node label or the label of their arc into the
    hub.  The weights on the offending column are zero, so the value meets layer 0's cut and nothing behind it.  A seeded form never cuts a
    label column: there only 'state' and 'agg_state' trip."""
    ds, nl = row['ds'], row['nl']
    hub = ROWS[pos]
    rng = np.random.default_rng(2000 + FORMS.index(row))
    g = graph(rng, N, nl, row['al'], 'sum', hub, SOURCES)
    s0 = _probe_state(rng, row, limit=1000.0)                        # the hub's sums stay in range
    val = LIMIT if at_limit else UNDER
    half = np.float32(2047.0) if at_limit else np.float32(UNDER / 2)
    Ws, bs = identity_chain(ds, nl, row['al'], row['hidden'])
    c = COL[where]
    if where == 'state':
        s0[hub, c] = val
        Ws[0][c, c] = 0.0
    elif where == 'label': g['nodes'][hub, c] = val
    elif where == 'agg_state': s0[list(SOURCES), c] = half
    elif where == 'agg_label': g['nodes'][list(SOURCES), c] = half
    else: g['arcs'][np.asarray(g['arcs'])[:, 1] == hub, 2 + c] = half
    trips = at_limit and not (row['seeded'] and where not in ('state', 'agg_state'))
    return _finish(row, rng, g, Ws, bs, s0, 'b0.layer0' if trips else None, s0)


# ---- 3. hidden layers ------------------------------------------------------------------------------------------------------------------------

def hidden_case(row, layer, unit, at_limit):
    rng = np.random.default_rng(3000 + FORMS.index(row))
    g = graph(rng, N, row['nl'], row['al'])
    Ws, bs = identity_chain(row['ds'], row['nl'], row['al'], row['hidden'])
    probe_unit(row, Ws, bs, layer, unit, LIMIT if at_limit else UNDER)
    s0 = _probe_state(rng, row)
    return _finish(row, rng, g, Ws, bs, s0, f'b0.hidden{layer}' if at_limit else None, s0, count=N)


# ---- 4. activations --------------------------------------------------------------------------------------------------------------------------

def activation_case(row, act, v, trips):
    """test_fp16_edges.test_activation_guard on a three-layer form: unit 100 of hidden layer 1 has the pre-activation v; states in [0, 1]."""
    assert len(row['hidden']) == 2
    rng = np.random.default_rng(4000 + FORMS.index(row))
    g = graph(rng, N, row['nl'], row['al'])
    Ws, bs = identity_chain(row['ds'], row['nl'], row['al'], row['hidden'])
    probe_unit(row, Ws, bs, 1, 100, np.float32(v))
    s0 = np.minimum(np.abs(_probe_state(rng, row)), np.float32(1.0))
    return _finish(row, rng, g, Ws, bs, s0, 'b0.hidden1' if trips else None, s0, acts=[act] * 3, exact=act in ('linear', 'relu', 'elu'), count=N)


# ---- 5. seeded forms -------------------------------------------------------------------------------------------------------------------------

def zeroed_label_case(row, value, seeded, arc=True):
    """(a) node label 0 of the hub - and, with `arc`, the labels of the arcs into it - set to `value`; every label row of W1 is zero.  value None:
    the same graph as the generators left it.  Unseeded, the node label alone is the one operand past the limit (the hub has no out-arcs)."""
    rng = np.random.default_rng(5000 + FORMS.index(row))
    hub = ROWS['partial']
    g = graph(rng, N, row['nl'], row['al'], 'sum', hub, SOURCES)
    Ws, bs = identity_chain(row['ds'], row['nl'], row['al'], row['hidden'])
    s0 = _probe_state(rng, row, limit=1000.0)
    if value is not None:
        g['nodes'][hub, 0] = value
        if arc: g['arcs'][np.asarray(g['arcs'])[:, 1] == hub, 2] = value
    return _finish(row, rng, g, Ws, bs, s0, None if seeded or value is None else 'b0.layer0', s0, seeded=seeded)


LABEL_UNIT = 7


def behind_label_unit(col, layers):
    """What the layers behind layer 0 make of the label unit's value (layers >= 2)."""
    return cut(col) if layers == 2 else cut(np.float32(0.5) * cut(col))


def unit_weight_case(row, v, seeded, trips, pos='partial', bodies=1):
    """(b), (c): node label 0 through a weight of 1 into unit 7 of layer 0 (no other input, zero bias); the hub's label is v.  Seeded, the unit's
    accumulator starts from exactly v and is cut by the next layer alone; unseeded, layer 0 cuts the label first.  A second hidden layer takes the
    unit with weight 0.5, as probe_unit."""
    ds, nl = row['ds'], row['nl']
    rng = np.random.default_rng(5500 + FORMS.index(row))
    hub = ROWS[pos]
    g = graph(rng, N, nl, row['al'], 'sum', hub, SOURCES)
    Ws, bs = identity_chain(ds, nl, row['al'], row['hidden'])
    Ws[0][:, LABEL_UNIT] = 0.0
    Ws[0][ds, LABEL_UNIT] = 1.0
    if len(Ws) > 2: Ws[1][LABEL_UNIT, LABEL_UNIT] = 0.5
    s0 = _probe_state(rng, row, limit=1000.0)
    g['nodes'][hub, 0] = v
    x = s0.copy()
    x[:, LABEL_UNIT] = g['nodes'][:, 0]
    return _finish(row, rng, g, Ws, bs, s0, trips, x, bodies=bodies, seeded=seeded)


# ---- 6. bookkeeping --------------------------------------------------------------------------------------------------------------------------

def bookkeeping_case(row):
    """(a tripping case, an in-range state0 for the same Loop)."""
    case = layer0_case(row, 'state', 'partial', True)
    small = np.clip(case['s0'], -200.0, 200.0).astype(np.float32)
    return case, small


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------------

def sharded_case():
    """The wide-state form on a loopback world of 2: the only operand at the limit is node label 0 of the last row, a hub without out-arcs -
    the last rank's."""
    return layer0_case(BY_ID[SHARDED_FORM], 'label', 'partial', True)
