"""Piece format 2 of the default path (impl 2): fp32 operands as two fp16 pieces (round to nearest even, power-of-two scales) on
v_mfma_f32_32x32x16_f16, with the range guard that repeats a Loop in format 3 (three bf16 pieces) when an activation leaves the fp16 range.

The packer's cut is host code (gnn_split_f16 / gnn_split_f16_exponent) and is tested without a GPU; the rest needs one."""
import numpy as np
import pytest


def _engine():
    from GNN import _engine
    return _engine


# ---- host-side packer (no GPU) -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('scale', [1e-3, 0.07, 1.0, 37.0, 3e4])
def test_packer_pieces_sum_back(scale):
    e = _engine()
    rng = np.random.default_rng(7)
    w = (scale * rng.standard_normal(4096)).astype(np.float32)
    w[:4] = [0.0, -0.0, scale, -scale]
    p0, p1, ex = e.split_f16(w)
    m = float(np.max(np.abs(w)))
    assert 2.0 ** 14 <= m * 2.0 ** ex < 2.0 ** 15              # the largest scaled weight a factor 2 below the fp16 maximum
    assert np.all(np.isfinite(p0)) and np.all(np.isfinite(p1))
    s = np.ldexp(w.astype(np.float64), ex)
    got = p0.astype(np.float64) + p1.astype(np.float64)
    err = np.abs(got - s)
    # p0 + p1 carries 23 - 24 significant bits: relative 2^-23 while p1 is a normal fp16; below that the subnormal spacing 2^-24 bounds it
    assert np.all(err <= np.maximum(2.0 ** -23 * np.abs(s), 2.0 ** -25)), float(np.max(err / np.maximum(np.abs(s), 1e-30)))
    # round to nearest even: p0 is the fp16 nearest to the scaled value, p1 the fp16 nearest to the remainder
    assert np.array_equal(p0, s.astype(np.float32).astype(np.float16))
    assert np.array_equal(p1, (s - p0.astype(np.float64)).astype(np.float32).astype(np.float16))


def test_packer_exponent_is_a_bounded_power_of_two():
    e = _engine()
    lib = e.lib()
    import ctypes as C
    for m in (1e-30, 1e-6, 0.25, 1.0, 1.5, 65504.0, 1e20):
        ex = lib.gnn_split_f16_exponent(C.c_float(m))
        assert isinstance(ex, int) and -60 <= ex <= 60
        if 1e-15 < m < 1e15:
            assert 2.0 ** 14 <= np.float32(m) * 2.0 ** ex < 2.0 ** 15
    assert lib.gnn_split_f16_exponent(C.c_float(0.0)) == 0


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------

def _setup(n, nl, hidden, act, seed, label_scale=1.0, state_scale=0.1, gain=1.0):
    from GNN import GNN_utils as utils
    from util import make_mlp
    e = _engine()
    s = utils.syntheticGraph(n, 10.0, nl, 1, 2, seed=seed)
    n = s['n_nodes']
    rng = np.random.default_rng(seed)
    st = make_mlp(rng, 1 + 2 * (nl + 64), list(hidden) + [64], act, gain=gain, bn_random=True)
    ou = make_mlp(rng, nl + 64, [2], 'softmax', bn_random=True)
    s0 = (state_scale * rng.standard_normal((n, 64))).astype(np.float32)
    nodes = (label_scale * np.asarray(s['nodes'], np.float32)).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], nodes, np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(ou['weights'], ou['activations'], True)
    return e, graph, mst, mou, s0


def _run(e, graph, mst, mou, s0, max_it, thr, impl=2, pieces=2, form=0):
    lp = e.Loop(graph, mst, mou, 64, max_it, thr)
    assert lp.set_impl(impl) == impl
    assert lp.set_pieces(pieces) == pieces
    lp.set_tile_form(form)
    lp.set_state0(s0)
    k = lp.run()
    res = (k, lp.state(), lp.output(), lp.range_info())
    lp.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('n,form', [(4096, 1), (4096, 2), (40_000, 1), (40_000, 2)])
def test_out_of_range_labels_repeat_the_loop_in_bf16_pieces(n, form):
    """Node labels scaled to 1e5 put layer-0 operands past the fp16 range: the guard trips, the Loop is repeated with bf16 pieces, and what
    the caller gets is exactly what format 3 returns - in both tile forms."""
    e, graph, mst, mou, s0 = _setup(n, 3, (128, 128), 'selu', n + 1, label_scale=1e5)
    k2, s2, o2, (rep2, tot2) = _run(e, graph, mst, mou, s0, 5, 0.0, pieces=2, form=form)
    k3, s3, o3, (rep3, tot3) = _run(e, graph, mst, mou, s0, 5, 0.0, pieces=3, form=form)
    graph.close()
    assert rep2 and tot2 == 1 and not rep3 and tot3 == 0
    assert k2 == k3 and np.array_equal(s2, s3) and np.array_equal(o2, o3)


@pytest.mark.gpu
@pytest.mark.parametrize('n,act,hidden', [(4096, 'selu', (128, 128)), (40_000, 'tanh', (128, 128)), (100_003, 'selu', (128, 128)),
                                          (65_552, 'sigmoid', (128,))])
def test_fp16_pieces_match_bf16_pieces(n, act, hidden):
    """Format 2 against format 3 and the exact chain (impl 1): within 1e-5 (the tolerance of the default path's tests), no repeat."""
    e, graph, mst, mou, s0 = _setup(n, 3, hidden, act, n + 2, gain=0.6)
    k2, s2, o2, (rep2, _) = _run(e, graph, mst, mou, s0, 6, 0.0, pieces=2)
    k3, s3, o3, _ = _run(e, graph, mst, mou, s0, 6, 0.0, pieces=3)
    k1, s1, o1, _ = _run(e, graph, mst, mou, s0, 6, 0.0, impl=1)
    graph.close()
    assert not rep2
    assert k2 == k3 == k1
    assert not np.isnan(s2).any()
    assert np.max(np.abs(s2 - s1)) < 1e-5 and np.max(np.abs(o2 - o1)) < 1e-5
    assert np.max(np.abs(s2 - s3)) < 1e-5 and np.max(np.abs(o2 - o3)) < 1e-5


@pytest.mark.gpu
def test_small_magnitude_states_stay_accurate():
    """States of about 1e-3 (small weights and biases, tanh, no BatchNormalization shift): the second fp16 piece is a subnormal in almost
    every cut at this magnitude (below 2^-7 always), so the cut is exact to 2^-29 absolute, about 2^-19 relative (test_fp16_edges.py,
    test_cut_precision_curve) - within 1e-5 of the exact chain, and far closer in relative terms."""
    from GNN import GNN_utils as utils
    from util import make_mlp
    e = _engine()
    n, nl = 8192, 3
    s = utils.syntheticGraph(n, 10.0, nl, 1, 2, seed=5)
    n = s['n_nodes']
    rng = np.random.default_rng(5)
    st = make_mlp(rng, 1 + 2 * (nl + 64), [128, 128, 64], 'tanh', batch_normalization=False, gain=0.3)
    st['weights'] = [w * np.float32(0.01) if i == 5 else w for i, w in enumerate(st['weights'])]    # last bias small
    st['weights'][4] = (st['weights'][4] * np.float32(0.01)).astype(np.float32)                       # last kernel small: states ~1e-3
    ou = make_mlp(rng, nl + 64, [2], 'softmax', batch_normalization=False)
    nodes = (0.01 * np.asarray(s['nodes'], np.float32)).astype(np.float32)
    graph = e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], nodes, np.ones(n, np.uint8))
    mst, mou = e.Mlp(st['weights'], st['activations'], False), e.Mlp(ou['weights'], ou['activations'], False)
    s0 = (1e-3 * rng.standard_normal((n, 64))).astype(np.float32)
    k2, s2, o2, (rep, _) = _run(e, graph, mst, mou, s0, 5, 0.0, pieces=2)
    k1, s1, o1, _ = _run(e, graph, mst, mou, s0, 5, 0.0, impl=1)
    graph.close()
    assert not rep and k2 == k1
    assert 1e-4 < float(np.mean(np.abs(s1))) < 1e-2
    assert np.max(np.abs(s2 - s1)) < 1e-5
    assert np.max(np.abs(s2 - s1)) < 1e-4 * float(np.max(np.abs(s1)))
