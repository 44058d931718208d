"""gnn_fused_net_form (host code, no device): which net_state descriptions the fused inference paths cover - the decision of make_plan
(csrc/gnn_fused.hip), the one every loop takes: one to three Dense layers no wider than 128, no softmax, one activation for all hidden
layers and any of the six for the last layer."""
import itertools

import pytest

ACTS = ['linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid']
PAIRS = [(a, b) for a, b in itertools.product(ACTS, ACTS) if a != b]


def _form(dims, acts, nlc=0):
    from GNN import _engine
    return _engine.fused_net_form(dims, acts, nlc)


def _tiles(width):
    return 1 if width <= 32 else (2 if width <= 64 else 4)


def _expected_tiles(dims):
    """The table in make_plan's comment: NTL from the last width, NT from the widest hidden layer (at least NTL); (2,1) and (4,1) are not
    instantiated and become (2,2) and (4,2); a one-layer net has NT == NTL."""
    ntl = _tiles(dims[-1])
    if len(dims) == 2:
        return ntl, ntl
    nt = max(_tiles(max(dims[1:-1])), ntl)
    if nt > 1 and ntl == 1: ntl = 2
    return nt, ntl


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('dims', [(7, 3), (135, 64), (40, 128), (31, 32, 14), (23, 16, 8), (135, 128, 64), (87, 48, 40), (139, 96, 68), (20, 64, 8), (20, 128, 32),
                                  (31, 32, 32, 14), (135, 128, 128, 64), (50, 33, 64, 20), (50, 100, 20, 128), (12, 128, 128, 128)])
def test_uniform_nets_are_covered_as_before(act, dims):
    f = _form(dims, [act] * (len(dims) - 1), nlc=3)
    assert f['covered'] and not f['mixed'] and f['hidden'] == act and f['last'] == act
    assert (f['NT'], f['NTL']) == _expected_tiles(dims)


def test_tile_table_endpoints():
    assert _expected_tiles((7, 3)) == (1, 1) and _expected_tiles((135, 64)) == (2, 2) and _expected_tiles((40, 128)) == (4, 4)
    assert _expected_tiles((20, 64, 8)) == (2, 2) and _expected_tiles((20, 128, 32)) == (4, 2) and _expected_tiles((135, 128, 128, 64)) == (4, 2)
    assert _expected_tiles((139, 96, 68)) == (4, 4) and _expected_tiles((50, 33, 64, 20)) == (2, 2)


@pytest.mark.parametrize('a,b', PAIRS)
def test_last_layer_may_have_its_own_activation(a, b):
    assert len(PAIRS) == 30
    two, three = _form((23, 16, 8), [a, b]), _form((135, 128, 128, 64), [a, a, b], nlc=3)
    for f, dims in ((two, (23, 16, 8)), (three, (135, 128, 128, 64))):
        assert f['covered'] and f['mixed'] and f['hidden'] == a and f['last'] == b
        assert (f['NT'], f['NTL']) == _expected_tiles(dims)
    # the same tiles as the uniform net of the same widths: the layout does not depend on the activations
    assert (three['NT'], three['NTL']) == (4, 2) and (two['NT'], two['NTL']) == (1, 1)


@pytest.mark.parametrize('a,b', PAIRS)
def test_two_hidden_activations_are_not_covered(a, b):
    for c in ACTS:
        f = _form((135, 128, 128, 64), [a, b, c])
        assert not f['covered'] and not f['mixed'] and f['hidden'] is None and f['last'] is None and f['NT'] == f['NTL'] == 0


def test_softmax_anywhere_is_not_covered():
    assert not _form((7, 3), ['softmax'])['covered']
    for a in ACTS:
        assert not _form((23, 16, 8), [a, 'softmax'])['covered']
        assert not _form((23, 16, 8), ['softmax', a])['covered']
        assert not _form((23, 16, 16, 8), [a, 'softmax', a])['covered']
        assert not _form((23, 16, 16, 8), [a, a, 'softmax'])['covered']
        assert not _form((23, 16, 16, 8), ['softmax', 'softmax', a])['covered']


def test_widths_and_depths_outside_the_kernels_are_not_covered():
    assert _form((300, 128), ['tanh'])['covered']                       # the input width is not a layer width
    assert not _form((30, 129), ['tanh'])['covered']
    assert not _form((30, 129, 8), ['tanh', 'tanh'])['covered'] and not _form((30, 129, 8), ['tanh', 'relu'])['covered']
    assert not _form((30, 16, 200, 8), ['selu', 'selu', 'tanh'])['covered']
    assert not _form((30, 16, 16, 130), ['selu', 'selu', 'tanh'])['covered']
    assert _form((30, 128, 128, 128), ['selu', 'selu', 'tanh'])['covered']
    assert not _form((30, 16, 16, 16, 8), ['tanh'] * 4)['covered']      # four Dense layers


def test_argument_errors():
    from GNN import _engine
    with pytest.raises(ValueError):
        _engine.fused_net_form((30, 8), ['tanh', 'tanh'])
    with pytest.raises(ValueError):
        _engine.fused_net_form((30, 0), ['tanh'])
    with pytest.raises(ValueError):
        _engine.fused_net_form((30, 8), ['tanh'], nlc=-1)
