"""gnn_small_form (host code, no device): which persistent small-graph launch a net_state takes on a given number of owned nodes - the
decision of small_form (csrc/gnn_fused.hip), the one gnn_loop_decide_form takes: every layer <= 32 wide -> 16-node tiles up to 4,096 nodes,
32-node tiles up to 8,192; two or three layers with hidden layers up to 64 wide (at least one above 32), state <= 32 -> the wide form on
16-node tiles up to 4,096 nodes; concat <= 96 for all of them.  Both neighbours of every limit."""
import pytest

NOT = dict(persistent=False, tile=0, wide=False, steps=0)


def _form(dims, n_rows, acts=None, nlc=0):
    from GNN import _engine
    return _engine.small_form(dims, acts or ['selu'] * (len(dims) - 1), n_rows, nlc)


def _steps16(concat):
    return next(s for s in (4, 8, 12, 16, 20, 24) if 4 * s >= concat)


def _narrow16(concat):
    return dict(persistent=True, tile=16, wide=False, steps=_steps16(concat))


def _wide(concat):
    return dict(persistent=True, tile=16, wide=True, steps=_steps16(concat))


def test_hidden_width_limits():
    assert _form((31, 32, 14), 600) == _narrow16(31)
    assert _form((31, 33, 14), 600) == _wide(31)
    assert _form((31, 64, 14), 600) == _wide(31)
    assert _form((31, 65, 14), 600) == NOT
    assert _form((31, 32, 32, 14), 600) == _narrow16(31)
    assert _form((31, 64, 64, 14), 600) == _wide(31) and _form((31, 64, 64, 14), 600)['steps'] == 8
    assert _form((31, 64, 65, 14), 600) == NOT and _form((31, 128, 128, 14), 600) == NOT


def test_state_width_limits():
    assert _form((70, 64, 32), 600) == _wide(70)
    assert _form((70, 64, 33), 600) == NOT
    assert _form((70, 32, 32), 600) == _narrow16(70)
    assert _form((70, 32, 33), 600) == NOT
    assert _form((70, 64, 64), 600) == NOT


def test_concat_width_limits():
    assert _form((96, 64, 16), 600) == _wide(96) and _wide(96)['steps'] == 24
    assert _form((97, 64, 16), 600) == NOT
    assert _form((96, 32, 16), 600) == _narrow16(96)
    assert _form((97, 32, 16), 600) == NOT
    assert [_form((c, 48, 8), 100)['steps'] for c in (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)] == [4, 4, 8, 8, 12, 12, 16, 16, 20, 20, 24, 24]


def test_row_limits():
    assert _form((31, 64, 64, 14), 1) == _wide(31)
    assert _form((31, 64, 64, 14), 4096) == _wide(31)
    assert _form((31, 64, 64, 14), 4097) == NOT
    assert _form((31, 64, 64, 14), 8192) == NOT
    assert _form((31, 64, 64, 14), 0) == NOT and _form((31, 32, 32, 14), 0) == NOT
    # a 32-wide net keeps its forms: 16-node tiles up to 4,096 nodes, 32-node tiles (K-steps of 2) up to 8,192
    assert _form((31, 32, 32, 14), 4096) == _narrow16(31)
    for n in (4097, 8192):
        f = _form((31, 32, 32, 14), n)
        assert f == dict(persistent=True, tile=32, wide=False, steps=16)
    assert _form((31, 32, 32, 14), 8193) == NOT
    assert _form((96, 32, 16), 5000) == dict(persistent=True, tile=32, wide=False, steps=48)
    assert _form((7, 3), 5000) == dict(persistent=True, tile=32, wide=False, steps=8)


def test_one_layer_nets_and_mixed_hidden_lists():
    assert _form((7, 3), 880) == _narrow16(7)
    assert _form((70, 32), 880) == _narrow16(70)
    assert _form((70, 33), 880) == NOT and _form((70, 64), 880) == NOT          # one layer: no hidden layer to be wide, the state is
    assert _form((23, 16, 64, 8), 300) == _wide(23)
    assert _form((23, 64, 16, 8), 300) == _wide(23)
    assert _form((23, 33, 64, 8), 300) == _wide(23)
    assert _form((23, 16, 32, 8), 300) == _narrow16(23)
    assert _form((23, 16, 16, 16, 8), 300, ['tanh'] * 4) == NOT                  # four Dense layers


def test_activations():
    assert _form((23, 64, 8), 300, ['relu', 'sigmoid']) == _wide(23)             # the last layer may have its own activation
    assert _form((23, 64, 64, 8), 300, ['tanh', 'tanh', 'linear']) == _wide(23)
    assert _form((23, 16, 8), 300, ['relu', 'sigmoid']) == _narrow16(23)
    assert _form((23, 64, 64, 8), 300, ['tanh', 'relu', 'relu']) == NOT          # two different hidden activations
    assert _form((23, 16, 16, 8), 300, ['tanh', 'relu', 'relu']) == NOT
    for acts in (['softmax', 'tanh'], ['tanh', 'softmax']):
        assert _form((23, 64, 8), 300, acts) == NOT
        assert _form((23, 16, 8), 300, acts) == NOT


def test_label_columns_do_not_change_the_form():
    assert _form((31, 64, 64, 14), 600, nlc=0) == _form((31, 64, 64, 14), 600, nlc=14)


def test_argument_errors():
    from GNN import _engine
    with pytest.raises(ValueError):
        _engine.small_form((30, 8), ['tanh', 'tanh'], 100)
    with pytest.raises(ValueError):
        _engine.small_form((30, 0), ['tanh'], 100)
    with pytest.raises(ValueError):
        _engine.small_form((30, 8), ['tanh'], -1)
    with pytest.raises(ValueError):
        _engine.small_form((30, 8), ['tanh'], 100, nlc=-1)
