"""Label projection (gnn_loop_set_label_projection), the parts that need no GPU: what the form decision answers from shapes alone
(gnn_label_projection_form) and the Python setter's way through copy() and save() / load()."""
import json

import pytest

N_ROWS = 100_000


def _form(dims, acts, ds, nl, al, mode, n_rows=N_ROWS):
    from GNN import _engine as e
    return e.label_projection_form(dims, acts, ds, nl, al, n_rows, mode)


def _concat(ds, nl, al):
    return 2 * (ds + nl) + al


# (state width, node-label columns in the concat, arc labels, layer widths, activations) -> seeded in mode 0 / 1 / 2, per-body kernel when seeded
SHAPES = [
    pytest.param(64, 14, 3, [128, 128, 64], ['selu'] * 3, (False, True, True), 2, id='mutag-widths'),          # concat 159: past the LDS tile
    pytest.param(64, 3, 1, [128, 128, 64], ['selu'] * 3, (False, False, True), 2, id='narrow-labels'),         # concat 135: covered as it stands
    pytest.param(20, 150, 2, [64, 20], ['tanh'] * 2, (False, True, True), 1, id='generic-wide'),
    pytest.param(128, 3, 1, [128, 128], ['tanh'] * 2, (False, False, False), 0, id='state-128'),               # [state | agg state] alone is 256 columns
    pytest.param(64, 14, 3, [144, 64], ['tanh'] * 2, (False, False, False), 0, id='hidden-144'),
    pytest.param(64, 14, 3, [128, 64], ['softmax', 'tanh'], (False, False, False), 0, id='softmax'),
    pytest.param(14, 0, 0, [32, 14], ['selu'] * 2, (False, False, False), 0, id='no-label-columns'),           # D = 0 (state = labels), AL = 0: IW = 0
]


@pytest.mark.parametrize('ds,nl,al,widths,acts,seeded,kernel', SHAPES)
def test_form_from_shapes(ds, nl, al, widths, acts, seeded, kernel):
    dims = [_concat(ds, nl, al)] + widths
    for mode, want in zip((0, 1, 2), seeded):
        f = _form(dims, acts, ds, nl, al, mode)
        assert f['seeded'] == want, (mode, f)
        if want:
            assert f['kernel'] == kernel and f['iw'] == 2 * nl + al and f['tiles'] == (4 if widths[0] > 64 else 2 if widths[0] > 32 else 1), (mode, f)
        else:
            assert f == dict(seeded=False, kernel=0, iw=0, tiles=0), (mode, f)
    for name, code in (('off', 0), ('auto', 1), ('always', 2)):
        assert _form(dims, acts, ds, nl, al, name) == _form(dims, acts, ds, nl, al, code)


def test_form_leaves_the_persistent_small_graph_loop_alone():
    # a narrow net on a small graph runs all bodies in one persistent launch (exact arithmetic): no projection in any mode
    dims, acts = [_concat(8, 3, 2), 16, 8], ['selu', 'selu']
    assert not _form(dims, acts, 8, 3, 2, 2, n_rows=300)['seeded']
    assert _form(dims, acts, 8, 3, 2, 2, n_rows=N_ROWS) == dict(seeded=True, kernel=1, iw=8, tiles=1)
    assert not _form(dims, acts, 8, 3, 2, 2, n_rows=0)['seeded']


def test_form_refuses_bad_arguments():
    with pytest.raises(ValueError): _form([135, 64], ['tanh'], 64, 3, 1, 'sometimes')
    with pytest.raises(ValueError): _form([135, 64], ['tanh'], 64, 3, 1, 3)
    with pytest.raises(ValueError, match='bad arguments'): _form([135, 64], ['tanh'], 0, 3, 1, 1)


def _model(cls=None):
    from GNN import losses, optimizers
    from GNN.GNN import GNNnodeBased
    from GNN.MLP import MLP
    st = MLP(1 + 2 * (4 + 3), [8, 4], 'tanh', 'glorot_normal', 'zeros', batch_normalization=False)
    ou = MLP(4 + 3, [2], 'softmax', 'glorot_normal', 'zeros', batch_normalization=False)
    return (cls or GNNnodeBased)(net_state=st, net_output=ou, optimizer=optimizers.Adam(0.02), loss_function=losses.categorical_crossentropy,
                                 loss_arguments=None, state_vect_dim=4, max_iteration=6, threshold=0.01, addressed_problem='c')


def test_python_setter_round_trip(tmp_path):
    from GNN.GNN import GNNgraphBased, GNNedgeBased
    from GNN.LGNN import LGNN
    gnn = _model()
    assert gnn.label_projection == 'off' and gnn.copy().label_projection == 'off'
    for given, kept in (('auto', 'auto'), (2, 'always'), (0, 'off'), ('always', 'always')):
        gnn.set_label_projection(given)
        assert gnn.label_projection == kept
    for bad in ('on', 3, -1, 1.5, True):
        with pytest.raises(ValueError): gnn.set_label_projection(bad)
    assert gnn.label_projection == 'always'                                # a refused call leaves the setting
    for cls in (None, GNNgraphBased, GNNedgeBased):                        # inherited by the graph- and edge-based models
        m = _model(cls)
        m.set_label_projection('auto')
        twin = m.copy(copy_weights=False)
        assert type(twin) is type(m) and twin.label_projection == 'auto'
    path = str(tmp_path / 'model')
    m.save(path)
    assert type(m).load(path).label_projection == 'auto'
    with open(f'{path}/config.json') as f: config = json.load(f)
    assert config['label_projection'] == 'auto'
    del config['label_projection']                                         # a model saved before the key existed
    with open(f'{path}/config.json', 'w') as f: json.dump(config, f)
    assert type(m).load(path).label_projection == 'off'
    lgnn = LGNN([_model(), _model()], get_state=False, get_output=True, optimizer=None, loss_function=None, loss_arguments=None, addressed_problem='c')
    lgnn.set_label_projection('auto')
    assert [g.label_projection for g in lgnn.gnns] == ['auto', 'auto']
