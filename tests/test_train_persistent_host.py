"""gnn_train_persistent_form (host code, no device): whether net_state's training-mode forward runs all its bodies in one persistent
launch, asserted on both neighbours of every limit of the predicate (gnn_train.h: small_train_form on top of net_decide_form's build_input)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXL = 3                      # GNN_FUSED_MAXL (csrc/gnn_fused.h): k_mlp_fwd takes up to one layer more
MIN_ROWS = 4096               # GNN_TRAIN_MFMA_MIN_ROWS (csrc/gnn_train_wide.hip)


@pytest.fixture(scope='module')
def e():
    from GNN import _engine
    if not os.path.exists(_engine.LIB_PATH):          # fresh checkout: cross-compile for gfx950 (no GPU needed), exactly what build() does
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'gnn_tf_2.x_amd', 'csrc'), '-j8'], stdout=subprocess.DEVNULL)
    return _engine


def taken(e, dims, acts=None, n=570, max_iter=5, rates=None):
    acts = acts if acts is not None else ['tanh'] * (len(dims) - 1)
    return e.train_persistent_form(dims, acts, n, max_iter, rates)['persistent']


def net(layers, width=16, n_in=21, d=8):
    return (n_in,) + (width,) * (layers - 1) + (d,)


def test_layer_count_limits(e):
    assert not taken(e, net(1)) and taken(e, net(2))
    assert taken(e, net(MAXL + 1)) and not taken(e, net(MAXL + 2))


def test_row_limits(e):
    assert taken(e, net(2), n=MIN_ROWS - 1) and not taken(e, net(2), n=MIN_ROWS)
    assert taken(e, net(2), n=1) and not taken(e, net(2), n=0)


@pytest.mark.parametrize('layers', [2, 3])
def test_any_dropout_rate_keeps_it_out(e, layers):
    """The kernel draws no masks: a rate in front of any Dense layer (0 .. L - 1) or of BatchNormalization (L) takes the per-body path;
    negative rates (AlphaDropout) too."""
    assert taken(e, net(layers), rates=[0.0] * (layers + 1))
    for q in range(layers + 1):
        for r in (0.25, -0.25):
            rates = [0.0] * (layers + 1)
            rates[q] = r
            assert not taken(e, net(layers), rates=rates), (q, r)


def test_softmax_only_as_last_activation(e):
    assert not taken(e, net(3), ['softmax', 'tanh', 'tanh']) and not taken(e, net(3), ['tanh', 'softmax', 'tanh'])
    assert taken(e, net(3), ['tanh', 'tanh', 'softmax']) and taken(e, net(2), ['relu', 'softmax'])


def test_max_iter_limits(e):
    assert not taken(e, net(2), max_iter=0) and taken(e, net(2), max_iter=1)


def test_workgroups_follow_the_row_chunks(e):
    """One workgroup per BatchNormalization chunk: rows_per_block is 32 up to 2,048 rows, 48 up to 3,072, 64 below 4,096."""
    for n, rows in [(1, 32), (32, 32), (33, 32), (2048, 32), (2049, 48), (3072, 48), (3073, 64), (4095, 64)]:
        f = e.train_persistent_form(net(2), ['tanh'] * 2, n, 3)
        assert f['persistent'] and f['rows'] == rows and f['workgroups'] == -(-n // rows) and f['workgroups'] <= 64, (n, f)
        assert 84 * 1024 <= f['lds'] <= 156 * 1024          # more than half a CU's LDS: one workgroup per CU


def test_byte_cap_at_its_edge(e):
    """Per body: [n, width] of the concat, of every Dense output, twice the state width and [chunks, 2 width], each rounded up to 64 floats;
    max_iter of them must fit TRAIN_PERSISTENT_MAX_BYTES."""
    dims, n = (100, 64, 64, 32), 4095
    pad = lambda floats: (floats + 63) // 64 * 64
    body = 4 * (pad(n * 100) + pad(n * 64) + pad(n * 64) + pad(n * 32) + 2 * pad(n * 32) + pad(64 * 2 * 32))
    f = e.train_persistent_form(dims, ['tanh'] * 3, n, 1)
    assert f['body_bytes'] == body
    fits = e.TRAIN_PERSISTENT_MAX_BYTES // body
    assert fits >= 2
    assert taken(e, dims, n=n, max_iter=fits) and not taken(e, dims, n=n, max_iter=fits + 1)


def test_lds_limit(e):
    """Two row tiles of the widest layer and dense_rows' partial sums must fit 156 KiB of LDS: 64-row workgroups take layers up to 184 wide."""
    assert taken(e, (21, 184, 8), n=4095) and not taken(e, (21, 188, 8), n=4095)
    assert taken(e, (21, 188, 8), n=2048)                # 32-row workgroups: half the tiles
