"""Recomputation of the bodies' activations (gnn_loop_set_train_recompute), the parts that need no GPU: the Python setter, its way through
copy(), save() / load() and the LGNN stack, and the wrappers of the two entry points."""
import json

import pytest


def _model(cls=None):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    st = MLP(1 + 2 * (4 + 3), [8, 4], 'tanh', 'glorot_normal', 'zeros')           # (BatchNormalization as MLP() builds it by default)
    ou = MLP(4 + 3, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=4, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_setter_validates_its_argument():
    gnn = _model()
    assert gnn.train_recompute is False
    gnn.set_train_recompute(True)
    assert gnn.train_recompute is True
    for bad in (1, 0, 'on', None, 1.0, [True]):
        with pytest.raises(ValueError): gnn.set_train_recompute(bad)
    assert gnn.train_recompute is True                                         # a refused call leaves the setting
    gnn.set_train_recompute(False)
    assert gnn.train_recompute is False


def test_attribute_survives_copy_save_load(tmp_path):
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    assert _model().copy().train_recompute is False
    for cls in (None, GNNgraphBased, GNNedgeBased):                            # inherited by the graph- and edge-based models
        m = _model(cls)
        m.set_train_recompute(True)
        twin = m.copy(copy_weights=False)
        assert type(twin) is type(m) and twin.train_recompute is True
        path = str(tmp_path / f'model_{cls.__name__ if cls else "node"}')
        m.save(path)
        assert type(m).load(path).train_recompute is True
        with open(f'{path}/config.json') as f: config = json.load(f)
        assert config['train_recompute'] is True
        del config['train_recompute']                                          # a model saved before the key existed
        with open(f'{path}/config.json', 'w') as f: json.dump(config, f)
        assert type(m).load(path).train_recompute is False
    off = _model()
    path = str(tmp_path / 'off')
    off.save(path)
    with open(f'{path}/config.json') as f: assert json.load(f)['train_recompute'] is False
    assert type(off).load(path).train_recompute is False


def test_lgnn_forwards_to_its_layers(tmp_path):
    from GNN.LGNN import LGNN
    lgnn = LGNN([_model(), _model()], get_state=False, get_output=True, optimizer=None, loss_function=None, loss_arguments=None, addressed_problem='c')
    assert [g.train_recompute for g in lgnn.gnns] == [False, False] and lgnn.train_recompute is False
    lgnn.set_train_recompute(True)
    assert [g.train_recompute for g in lgnn.gnns] == [True, True] and lgnn.train_recompute is True
    with pytest.raises(ValueError): lgnn.set_train_recompute('yes')
    assert [g.train_recompute for g in lgnn.copy().gnns] == [True, True]
    lgnn.set_train_recompute(False)
    assert [g.train_recompute for g in lgnn.gnns] == [False, False]


def test_engine_wrappers_are_there():
    from GNN import _engine as e
    for name in ('gnn_loop_set_train_recompute', 'gnn_loop_train_recompute_info'):
        assert name in e.EXPORTS
        assert hasattr(e.lib(), name)
    assert callable(e.Loop.set_train_recompute) and callable(e.Loop.train_recompute_info)
