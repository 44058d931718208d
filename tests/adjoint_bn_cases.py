"""Inputs of the frozen-BatchNormalization tests (tests/test_gpu_adjoint_bn.py; tests/test_adjoint_bn_host.py checks on the CPU what the builders
promise: that the mirror's adjoint converges on every case).  Inputs only, no reference code.

BatchNormalization arrays of every net_state: moving mean non-zero (0.1 .. 0.5 in size, either sign), moving variance in [0.25, 4], gamma in
[0.5, 1.5] in size with about a third negative, beta non-zero - the column scale s_j = gamma_j / sqrt(var_j + eps) lies between 0.25 and 3 in
size, so a missing or doubled scale shows at order 1 (at mean 0 / variance 1 / gamma 1 it would hide inside the tolerance).  The weight gain
makes up for the scale: with it the mirror's adjoint converges.

Graphs: from 37 nodes on the directed, unsorted arc lists of tests/train_graph_cases.py (hub 0, no in-arcs 1, no out-arcs 2, isolated 3, pinned
degrees); below that (the builder needs 37 nodes) a symmetric random list with an isolated node 1 and a hub 0."""
import numpy as np

import train_graph_cases as G
from oracle import gnn_oracle as orc
from util import make_mlp, random_arcs


def bn_arrays(rng, d):
    either = lambda: np.where(rng.random(d) < 0.5, -1.0, 1.0)
    gamma = np.where(rng.random(d) < 0.3, -1.0, 1.0) * rng.uniform(0.5, 1.5, d)
    beta = either() * rng.uniform(0.1, 0.5, d)
    mean = either() * rng.uniform(0.1, 0.5, d)
    var = rng.uniform(0.25, 4.0, d)
    var[0] = 4.0                                    # both ends of the range: |s_0| <= 0.75 whatever the draw (a single column is a state width too) ...
    if d > 1: var[-1] = 0.25                        # ... and |s| up to 3
    return [a.astype(np.float32) for a in (gamma, beta, mean, var)]


def frozen_net(rng, n_in, layers, act, gain, bn=True):
    net = make_mlp(rng, n_in, list(layers), act, gain=gain, batch_normalization=False)
    if bn:
        net['weights'] = net['weights'] + bn_arrays(rng, layers[-1])
        net['batch_normalization'] = True
    return net


def problem(seed, n, ds, nl=2, al=1, hidden=(7,), act='tanh', gain=0.3, mask_p=0.7, bn=True, D=None, targets_scale=1.0):
    """Graph, nets, initial state, targets of a node-based step.  Masked rows: about mask_p of them carry a target."""
    rng = np.random.default_rng(seed)
    if n >= 37:
        arcs = G.directed_graph(seed, n, degrees=True, al=al)
    else:
        arcs = random_arcs(rng, n, 2 * n, al)
        hub = n // 2
        dst = rng.permutation(np.arange(1, n))[:hub]
        extra = np.concatenate([np.zeros((hub, 1)), dst[:, None], 2 * rng.random((hub, al)) - 1], axis=1).astype(np.float32)
        arcs = np.concatenate([arcs, extra])
        _, first = np.unique(arcs[:, :2], axis=0, return_index=True)
        arcs = arcs[np.sort(first)]
        arcs = arcs[(arcs[:, 0] != 1) & (arcs[:, 1] != 1)]
    nodes = (2 * rng.random((n, nl)) - 1).astype(np.float32)
    g = orc.make_graph_dict(arcs, nodes, 'average')
    g['set_mask'] = rng.random(n) < mask_p
    g['set_mask'][0] = True
    D = ds if D is None else D
    nlc = nl if D else 0
    st = frozen_net(rng, al + 2 * (ds + nlc), list(hidden) + [ds], act, gain, bn)
    ou = make_mlp(rng, ds + nlc, [2], 'softmax', batch_normalization=False)
    m = int((g['set_mask'] & g['output_mask']).sum())
    targets = np.eye(2)[rng.integers(0, 2, m)].astype(np.float32)
    weights = (targets_scale * rng.uniform(0.5, 1.5, m)).astype(np.float32)
    s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
    return dict(g=g, st=st, ou=ou, ds=ds, D=D, s0=s0 if D else None, targets=targets, weights=weights, n=n)


# ---- 1 / 2. the one-launch iteration (mode 1) and the per-kernel chain on the same nets (mode 2) -------------------------------------------------
# rows 15 | 16 | 17 (the 16 rows of a block) and 37; state widths 1, 5, 16 | 17, 33 (a third 16-lane column pass) and 64 (a 133-wide concat: the
# chain in both modes); 1, 2 and 3 Dense layers; tanh and selu
NARROW = [dict(n=15, ds=1, hidden=()), dict(n=16, ds=5, hidden=(7,), act='selu'), dict(n=17, ds=16, hidden=(9, 6)), dict(n=37, ds=17, hidden=(7,), act='selu'),
          dict(n=37, ds=33, hidden=(12, 9)), dict(n=17, ds=64, hidden=(20,)), dict(n=16, ds=16, hidden=(), act='selu'), dict(n=15, ds=5, hidden=(6, 4), act='selu'),
          dict(n=37, ds=1, hidden=(5,))]


def narrow_problem(case):
    return problem(101, **case)


# ---- 3. many rows: 4,095 | 4,096 and 4,113 rows, the 128-wide three-layer net (k_layer_bwd below 4,096 rows, the chain from there on) and a two-layer
# wide net; the gamma and beta gradients are sums of more than one chunk partial there
LARGE = [((135, 128, 128, 64), 4095, ['per_op'] * 3, 'rows'), ((135, 128, 128, 64), 4096, ['chain3'] * 3, 'rows_aligned'),
         ((135, 128, 128, 64), 4113, ['chain3'] * 3, 'rows_aligned'), ((135, 144, 64), 4113, ['wide'] * 2, 'rows')]


def large_problem(dims, n):
    ds = dims[-1]
    nl, al = 3, 1
    assert al + 2 * (ds + nl) == dims[0]
    # (targets_scale: a loss of order 1 over ~2,900 masked rows, so that the gradients are of the small cases' size)
    return problem(131, n=n, ds=ds, nl=nl, al=al, hidden=dims[1:-1], gain=0.3, targets_scale=1.0 / 64)


def dims_of(pb):
    return [pb['st']['weights'][0].shape[0]] + [w.shape[0] for w in pb['st']['weights'][1:2 * len(pb['st']['activations']):2]]
