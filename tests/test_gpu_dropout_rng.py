"""The Dropout / AlphaDropout masks that a training step DRAWS (the engine's own generator: every train(), training_step and LGNN joint
step), read back with gnn_loop_train_mask.  The tight comparisons of tests/test_gpu_train.py inject their masks - the `mask_in` branch of
k_train_input / k_dropout_fwd; this file takes the other branch: the mask that was recorded is the mask that was applied (the float64
oracle, fed the read-back masks, gives the step's loss and gradients), a drawn step equals the same step with its masks injected, the
keep rate is 1 - rate, and no two uses of the generator - elements, rows, bodies, positions, nets, seeds, steps, LGNN layers - share bits.

Statistics: a mask bit is kept with probability 1 - r.  Two independent masks of rates r1, r2 agree in a share q = (1 - r1)(1 - r2) + r1 r2
of their elements (q = (1 - r)^2 + r^2 for equal rates), with standard deviation sqrt(q (1 - q) / n) over n elements; blocks of different
widths are compared over their common leading elements (the generator indexes a block flat).  Every check is |observed - expected| <= 5
sigma, seeds fixed: 5.7e-7 per check under independence, a few hundred checks in the file.  A mask shared between two uses agrees in
1 - |r1 - r2| of its elements instead - 100 % for equal rates - tens of sigma away at these sizes.

Not covered: the 64-bit index branch of k_train_input (more than 2^31 elements in one concat) is not reachable at test size."""
import functools

import numpy as np
import pytest

from oracle import gnn_oracle as orc
from oracle import gnn_train_oracle as tro
from test_gpu_train import _by_source_csr
from util import make_mlp, random_arcs

pytestmark = pytest.mark.gpu

MAX_IT = 6
# Dropout rates [n_layers + 1] of net_state (24 -> 16 -> 8) and net_output (11 -> 9 -> 2): config 0 is the one of test_train_step_matches_oracle
# (the mask of net_state rides on k_train_input), config 1 puts them inside net_state and in front of both BatchNormalizations (k_dropout_fwd)
RATES = [([0.2, 0.0, 0.0], [0.1, 0.3, 0.0]), ([0.0, 0.25, 0.15], [0.0, 0.0, 0.2])]
SEED = 5


@functools.lru_cache(maxsize=None)
def _case(cfg, alpha, graph_based):
    """The node-based shape of test_train_step_matches_oracle (n = 500, d = 8, threshold 0: all six bodies run); alpha: AlphaDropout on a
    SELU net (negative rates on the C ABI)."""
    from GNN import _engine as e
    rng = np.random.default_rng(108)
    n, d, nl, al = 500, 8, 3, 2
    arcs = random_arcs(rng, n, 1500, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    ng = None
    if graph_based:
        ng = np.zeros((n, 3), np.float32); ng[:200, 0] = 1 / 200; ng[200:350, 1] = 1 / 150; ng[350:, 2] = 1 / 150
    g = orc.make_graph_dict(arcs, nodes, 'average', NodeGraph=ng)
    if not graph_based:
        g['set_mask'] = rng.random(n) < 0.8
    act = 'selu' if alpha else 'tanh'
    st = make_mlp(rng, al + 2 * (d + nl), [16, d], act, gain=0.8, bn_random=True)
    ou = make_mlp(rng, d + nl, [9, 2], act, out_activation='softmax', bn_random=True)
    rs, ro = RATES[cfg]
    st['dropout'], ou['dropout'] = {i: r for i, r in enumerate(rs) if r}, {i: r for i, r in enumerate(ro) if r}
    if alpha: st['alphadropout'] = ou['alphadropout'] = True
    loss = 'mean_squared_error' if graph_based else ('categorical_crossentropy_from_logits' if alpha else 'categorical_crossentropy')
    mask = g['set_mask'] & g['output_mask']
    n_t = 3 if graph_based else int(mask.sum())
    targets = np.eye(2)[rng.integers(0, 2, n_t)].astype(np.float32)
    weights = rng.uniform(0.5, 1.5, n_t).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    ng_csr = None
    if graph_based:
        cols, rows = np.nonzero(ng.T)
        ip = np.zeros(4, np.int32); np.cumsum(np.bincount(cols, minlength=3), out=ip[1:])
        ng_csr = (ip, rows.astype(np.int32), ng[rows, cols])
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    loop = e.Loop(graph, mst, mou, d, MAX_IT, 0.0)
    loop.set_state0(s0)
    sgn = -1.0 if alpha else 1.0
    kind = {'categorical_crossentropy': 0, 'mean_squared_error': 1, 'categorical_crossentropy_from_logits': 2}[loss]
    return dict(g=g, st=st, ou=ou, s0=s0, targets=targets, weights=weights, loss=loss, kind=kind, ng_csr=ng_csr, graph_based=graph_based, loop=loop,
                mst=mst, mou=mou, src=_by_source_csr(g, n), rs=[sgn * r for r in rs], ro=[sgn * r for r in ro], d=d)


def _read_masks(loop, rs, ro, k):
    """every mask of the last step: ([{position: [N, width] bool} per body], {position: [M, width] bool})"""
    ms = [{p: loop.train_mask(0, body, p) for p, r in enumerate(rs) if r} for body in range(k)]
    return ms, {p: loop.train_mask(1, 0, p) for p, r in enumerate(ro) if r}


def _pack(ms, mo):
    """the layout of masks_state / masks_output (include/gnn_hip.h): per body the positions' blocks one after the other"""
    return (np.concatenate([b[p].astype(np.uint8).ravel() for b in ms for p in sorted(b)]),
            np.concatenate([mo[p].astype(np.uint8).ravel() for p in sorted(mo)]))


def _step(c, seed, inject=None):
    kw = dict(dropout_state=c['rs'], dropout_output=c['ro'], bn_state=np.concatenate(c['st']['weights'][-4:-2]),
              bn_output=np.concatenate(c['ou']['weights'][-4:-2]))
    if inject is not None: kw.update(masks_state=inject[0], masks_output=inject[1])
    res = c['loop'].train_step(c['mst'], c['mou'], c['src'], c['targets'], c['weights'], c['kind'], c['ng_csr'], seed=seed, **kw)
    assert res['k'] == MAX_IT
    ms, mo = _read_masks(c['loop'], c['rs'], c['ro'], MAX_IT)
    return dict(res=res, ms=ms, mo=mo)


@functools.lru_cache(maxsize=None)
def _drawn(cfg, alpha, graph_based, seed):
    """one step with the engine's own masks (shared by the tests below; nobody writes to it)"""
    return _step(_case(cfg, alpha, graph_based), seed)


def _blocks(run, c):
    """[(name, mask, rate)] of every (net, body, position) of a step"""
    out = [(f'state body {b} pos {p}', m, abs(c['rs'][p])) for b, body in enumerate(run['ms']) for p, m in sorted(body.items())]
    return out + [(f'output pos {p}', m, abs(c['ro'][p])) for p, m in sorted(run['mo'].items())]


def _agreement_z(a, ra, b, rb):
    """(share of the common leading elements in which two masks agree - what independence predicts) / its standard deviation"""
    a, b = a.ravel(), b.ravel()
    n = min(a.size, b.size)
    q = (1 - ra) * (1 - rb) + ra * rb
    return (float(np.mean(a[:n] == b[:n])) - q) / np.sqrt(q * (1 - q) / n)


def _same_results(a, b):
    return (a['loss'] == b['loss'] and a['k'] == b['k'] and all(np.array_equal(x, y) for x, y in zip(a['grads_state'] + a['grads_output'], b['grads_state'] + b['grads_output']))
            and np.array_equal(a['bn_batch_state'], b['bn_batch_state']) and np.array_equal(a['bn_batch_output'], b['bn_batch_output']))


def _same_masks(a, b):
    return all(np.array_equal(x[p], y[p]) for x, y in zip(a['ms'], b['ms']) for p in x) and all(np.array_equal(a['mo'][p], b['mo'][p]) for p in a['mo'])


CASES = [(0, False, False), (1, False, False), (0, True, False), (1, True, False), (0, False, True)]


@pytest.mark.parametrize('cfg,alpha,graph_based', CASES)
def test_drawn_masks_are_what_the_step_applied(cfg, alpha, graph_based):
    """a. train_step(seed) without masks; the float64 oracle on the masks read back gives the step's loss, k and gradients at the bars of
    test_train_step_matches_oracle - a keep byte that differed from what the kernel applied, forward or backward, would not."""
    c = _case(cfg, alpha, graph_based)
    run = _drawn(cfg, alpha, graph_based, SEED)
    res = run['res']
    ref = tro.train_step(c['g'], c['st'], c['ou'], c['d'], MAX_IT, 0.0, c['s0'], run['ms'], run['mo'], c['targets'], c['weights'], loss=c['loss'], mean=False,
                         graph_based=graph_based)
    assert res['k'] == ref['k'] == MAX_IT
    print('loss', res['loss'], ref['loss'])
    assert abs(res['loss'] - ref['loss']) <= 2e-5 * max(1.0, abs(ref['loss']))
    for got, want in list(zip(res['grads_state'], ref['grads_state'])) + list(zip(res['grads_output'], ref['grads_output'])):
        print(got.shape, float(np.max(np.abs(got - want))), float(np.max(np.abs(want))))
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-3 * max(1e-3, np.max(np.abs(want))), (got.shape, np.max(np.abs(got - want)), np.max(np.abs(want)))


@pytest.mark.parametrize('cfg,alpha,graph_based', CASES[:4])
def test_drawn_step_equals_the_step_with_its_masks_injected(cfg, alpha, graph_based):
    """b. the same step with the read-back masks injected: identical bits in every result, and the getter returns the injected masks."""
    c = _case(cfg, alpha, graph_based)
    run = _drawn(cfg, alpha, graph_based, SEED)
    again = _step(c, SEED + 17, inject=_pack(run['ms'], run['mo']))          # (the seed is not read when masks are given)
    assert _same_results(run['res'], again['res'])
    assert _same_masks(run, again)


@pytest.mark.parametrize('cfg', [0, 1])
def test_a_seed_defines_the_masks_and_the_next_seed_draws_others(cfg):
    """c. seed s twice: the same masks and results; seed s + 1: masks that agree with those of s at the chance rate only."""
    c = _case(cfg, False, False)
    run = _drawn(cfg, False, False, SEED)
    twice = _step(c, SEED)
    assert _same_masks(run, twice) and _same_results(run['res'], twice['res'])
    other = _drawn(cfg, False, False, SEED + 1)
    bad = []
    for (name, a, r), (_, b, _) in zip(_blocks(run, c), _blocks(other, c)):
        z = _agreement_z(a, r, b, r)
        if abs(z) > 5: bad.append((name, z))
    assert not bad, bad


@pytest.mark.parametrize('cfg', [0, 1])
@pytest.mark.parametrize('seed', [0, 1, 5, 1000003])
def test_keep_rate(cfg, seed):
    """d. every (net, body, position) block keeps 1 - r of its elements, within 5 sigma of a Bernoulli sample of its size."""
    c = _case(cfg, False, False)
    bad = []
    for name, m, r in _blocks(_drawn(cfg, False, False, seed), c):
        z = (float(m.mean()) - (1 - r)) / np.sqrt(r * (1 - r) / m.size)
        if abs(z) > 5: bad.append((name, m.size, float(m.mean()), z))
    assert not bad, bad


@pytest.mark.parametrize('cfg', [0, 1])
def test_blocks_of_one_step_share_no_bits(cfg):
    """e. inside a block: against itself shifted by one element and by one row; between blocks: every pair of (net, body, position) blocks
    of one step - other bodies, other positions, net_state against net_output."""
    c = _case(cfg, False, False)
    blocks = _blocks(_drawn(cfg, False, False, SEED), c)
    bad, worst = [], 0.0
    for name, m, r in blocks:
        f = m.ravel()
        for what, z in (('element', _agreement_z(f[1:], r, f[:-1], r)), ('row', _agreement_z(m[1:], r, m[:-1], r))):
            worst = max(worst, abs(z))
            if abs(z) > 5: bad.append((name, 'shifted by one ' + what, z))
    for i, (na, a, ra) in enumerate(blocks):
        for nb, b, rb in blocks[i + 1:]:
            z = _agreement_z(a, ra, b, rb)
            worst = max(worst, abs(z))
            if abs(z) > 5: bad.append((na, nb, z))
    print('worst deviation', worst, 'sigma')
    assert not bad, bad


@pytest.mark.parametrize('cfg', [0, 1])
def test_nearby_seeds_do_not_replay_masks_in_another_body_or_net(cfg):
    """e. stream keys that are SUMS of the seed and per-use constants meet: with body e keyed seed + 7919 (e + 1) and net_output keyed
    seed + 104729, seed s in body e + 1 drew the masks of seed s + 7919 in body e, bit for bit, and net_output under seed s those of body 0
    under seed s + 104729 - 7919 (its leading elements, thresholded at net_output's rate).  Hashed keys do not."""
    c = _case(cfg, False, False)
    run = _drawn(cfg, False, False, SEED)
    bad = []
    later = _drawn(cfg, False, False, SEED + 7919)
    for e in range(MAX_IT - 1):
        for p, a in run['ms'][e + 1].items():
            r = abs(c['rs'][p])
            z = _agreement_z(a, r, later['ms'][e][p], r)
            if abs(z) > 5: bad.append((f'seed s body {e + 1} / seed s + 7919 body {e}, position {p}', z))
    other = _drawn(cfg, False, False, SEED + 104729 - 7919)
    for p, a in run['mo'].items():
        for ps, b in other['ms'][0].items():
            z = _agreement_z(a, abs(c['ro'][p]), b, abs(c['rs'][ps]))
            if abs(z) > 5: bad.append((f'seed s net_output position {p} / seed s + 96810 body 0 position {ps}', z))
    assert not bad, bad


def _surface_graph(rng, n):
    from GNN.graph_class import GraphObject, GraphTensor
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    cls = (nodes[:, 0] + 0.5 * nodes[:, 1] > 0).astype(int)
    return GraphTensor.fromGraphObject(GraphObject(arcs=random_arcs(rng, n, 3 * n, 1), nodes=nodes, targets=np.eye(2)[cls]))


def _surface_model(layer=0):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    w = 3 + 2 * (layer > 0)
    st = MLP(1 + 2 * w, [8, w], 'tanh', 'glorot_normal', 'zeros', dropout_rate=0.2, dropout_pos=0)
    ou = MLP(w, [6, 2], ['tanh', 'softmax'], 'glorot_normal', 'zeros', dropout_rate=0.3, dropout_pos=1, batch_normalization=False)
    return GNNnodeBased(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.01), loss_function=losses.categorical_crossentropy, loss_arguments=None,
                        state_vect_dim=0, max_iteration=3, threshold=0.0, addressed_problem='c')


def test_python_surface_draws_fresh_masks_per_step_and_per_lgnn_layer():
    """f. GNNnodeBased.training_step twice: the masks of the model's loop differ between the calls at the chance rate.  A two-layer LGNN joint
    step: the layers' net_output masks (equal shapes and rates) and their net_state masks (common leading elements) agree at the chance rate
    only - the layers' seeds advance in step, so without the layer index in the seed every layer drew the same bits."""
    from GNN import losses, optimizers
    from GNN.LGNN import LGNN
    from GNN.MLP import set_seed
    set_seed(3)
    g = _surface_graph(np.random.default_rng(3), 400)
    gnn = _surface_model()
    loop = gnn._device_loop(g.device_graph(gnn.device))
    steps = []
    for _ in range(2):
        res = gnn.training_step(g, True)
        assert res['k'] == 3
        steps.append(_read_masks(loop, [0.2, 0, 0], [0, 0.3, 0], 3))
    bad = []
    for body in range(3):
        z = _agreement_z(steps[0][0][body][0], 0.2, steps[1][0][body][0], 0.2)
        if abs(z) > 5: bad.append(('training_step 1 / 2, net_state body', body, z))
    z = _agreement_z(steps[0][1][1], 0.3, steps[1][1][1], 0.3)
    if abs(z) > 5: bad.append(('training_step 1 / 2, net_output', z))
    # ---- LGNN, joint step: layer 1 sees two more label columns (get_output), its net_output is 5 -> 6 -> 2 beside 3 -> 6 -> 2: the Dropout
    # in front of the second Dense layer has the same shape [n, 6] in both
    lgnn = LGNN([_surface_model(0), _surface_model(1)], False, True, optimizers.Adam(0.01), losses.categorical_crossentropy, None, 'c')
    lgnn.training_mode = 'parallel'
    lgnn.training_step(g, True)
    loops = [lgnn.gnns[0]._device_loop(g.device_graph(lgnn.gnns[0].device)), lgnn.gnns[1]._device_loop(next(iter(g._lgnn_graphs.values())))]
    m0, m1 = (_read_masks(lp, [0.2, 0, 0], [0, 0.3, 0], 3) for lp in loops)
    assert m0[1][1].shape == m1[1][1].shape == (400, 6)
    z = _agreement_z(m0[1][1], 0.3, m1[1][1], 0.3)
    if abs(z) > 5: bad.append(('LGNN layers 0 / 1, net_output', z))
    for body in range(3):
        z = _agreement_z(m0[0][body][0], 0.2, m1[0][body][0], 0.2)
        if abs(z) > 5: bad.append(('LGNN layers 0 / 1, net_state body', body, z))
    assert not bad, bad


def test_wide_forms_drawn_masks():
    """g. the Dropout case of test_wide_layers_on_the_matrix_cores_match_oracle (n = 4500, 135 -> 128 -> 128 -> 64, rate 0.1 behind the first
    hidden layer): the matrix-core backward epilogue (dropout_grad of k_gemm_split) on DRAWN masks - drawn equals injected, and the keep rate."""
    from GNN import _engine as e
    n, d, hidden, max_it, rate = 4500, 64, (128, 128), 3, 0.1
    rng = np.random.default_rng(n)
    nl, al = 3, 1
    arcs = random_arcs(rng, n, 4 * n, al)
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < 0.9
    st = make_mlp(rng, al + 2 * (d + nl), list(hidden) + [d], 'selu', gain=0.7, bn_random=True)
    ou = make_mlp(rng, d + nl, [2], 'softmax', batch_normalization=False)
    mask = g['set_mask'] & g['output_mask']
    m = int(mask.sum())
    targets = np.eye(2)[rng.integers(0, 2, m)].astype(np.float32)
    weights = (rng.uniform(0.5, 1.5, m) / m).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
    graph = e.Graph(n, g['adjT'][0], g['adjT'][1], g['adjT'][2], g['arcT'][2], np.asarray(g['arcs'])[:, 2:][g['arcT'][1]], nodes, mask)
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], False)
    loop = e.Loop(graph, mst, mou, d, max_it, 0.0)
    loop.set_state0(s0)
    src = _by_source_csr(g, n)
    step = lambda **kw: loop.train_step(mst, mou, src, targets, weights, 0, None, dropout_state=[0, rate, 0, 0], dropout_output=[0, 0],
                                        bn_state=np.concatenate(st['weights'][-4:-2]), bn_output=None, **kw)
    drawn = step(seed=SEED)
    assert drawn['k'] == max_it and loop.train_forms(0)['backward'][1] == 'wide'
    ms = [loop.train_mask(0, body, 1) for body in range(max_it)]
    for body, mk in enumerate(ms):
        assert mk.shape == (n, hidden[0])
        z = (float(mk.mean()) - (1 - rate)) / np.sqrt(rate * (1 - rate) / mk.size)
        assert abs(z) <= 5, (body, float(mk.mean()), z)
    injected = step(masks_state=np.concatenate([mk.astype(np.uint8).ravel() for mk in ms]))
    assert _same_results(drawn, injected)
    assert all(np.array_equal(mk, loop.train_mask(0, body, 1)) for body, mk in enumerate(ms))


def test_mask_getter_errors_and_lifetime():
    """h. GNN_ERR_STATE before any training forward; argument errors for body == k, a position without Dropout, a net other than 0 / 1.  The
    masks outlive the backward pass (train_step has run it) and a later inference run(): the context is replaced by the next training
    forward only."""
    from GNN import _engine as e
    c = _case(0, False, False)
    fresh = e.Loop(c['loop'].graph, c['mst'], c['mou'], c['d'], MAX_IT, 0.0)
    with pytest.raises(e.EngineError):
        fresh.train_mask(0, 0, 0)
    fresh.set_state0(c['s0'])
    fresh.run()
    with pytest.raises(e.EngineError):
        fresh.train_mask(0, 0, 0)                                  # an inference run leaves no training context
    run = _step(c, SEED)
    loop = c['loop']
    for net, body, pos in ((0, MAX_IT, 0), (0, -1, 0), (0, 0, 1), (0, 0, 3), (1, 0, 2), (1, 0, -1), (2, 0, 0)):
        with pytest.raises(ValueError):
            loop.train_mask(net, body, pos)
    assert np.array_equal(loop.train_mask(1, 99, 1), run['mo'][1])   # net_output: body is ignored
    loop.run()
    assert _same_masks(run, dict(zip(('ms', 'mo'), _read_masks(loop, c['rs'], c['ro'], MAX_IT))))


def test_initial_state_generator_moments_and_seeds():
    """i. set_state0(None, seed) (k_randn) on 2048 x 8 draws: skewness and excess kurtosis of a normal sample within 5 standard errors
    (sqrt(6 / n), sqrt(24 / n)), the same seed gives the same bits, another seed a sample correlation within 5 / sqrt(n)."""
    from GNN import _engine as e
    c = _case(0, False, False)
    n = 2048
    rng = np.random.default_rng(9)
    nodes = (2 * rng.random((n, 3)) - 1).astype(np.float32)
    gd = orc.make_graph_dict(random_arcs(rng, n, 3 * n, 2), nodes, 'average')
    graph = e.Graph(n, gd['adjT'][0], gd['adjT'][1], gd['adjT'][2], gd['arcT'][2], np.asarray(gd['arcs'])[:, 2:][gd['arcT'][1]], nodes, np.ones(n, np.uint8))
    loop = e.Loop(graph, c['mst'], c['mou'], 8, 0, 0.01)           # max_iter 0: the Loop returns its initial state

    def draw(seed):
        loop.set_state0(None, seed=seed)
        assert loop.run() == 0
        return loop.state().astype(np.float64)

    a, a2, b = draw(3), draw(3), draw(4)
    assert np.array_equal(a, a2)
    cnt = a.size
    zs = (a - a.mean()) / a.std()
    skew, kurt = float(np.mean(zs ** 3)), float(np.mean(zs ** 4) - 3.0)
    corr = float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    print('mean', a.mean(), 'std', a.std(), 'skewness', skew, 'excess kurtosis', kurt, 'correlation', corr)
    assert abs(a.mean()) <= 5 * 0.1 / np.sqrt(cnt) and abs(a.std() - 0.1) <= 5 * 0.1 / np.sqrt(2 * cnt)
    assert abs(skew) <= 5 * np.sqrt(6 / cnt) and abs(kurt) <= 5 * np.sqrt(24 / cnt)
    assert abs(corr) <= 5 / np.sqrt(cnt)
    # neighbouring elements and rows of one draw
    f = a.ravel()
    assert abs(float(np.corrcoef(f[1:], f[:-1])[0, 1])) <= 5 / np.sqrt(cnt) and abs(float(np.corrcoef(a[1:].ravel(), a[:-1].ravel())[0, 1])) <= 5 / np.sqrt(cnt)
