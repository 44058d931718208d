"""Host side of the training surface: the gradient clipping of the NumPy optimizers (the mirror of gnn_loop_set_clipping) against
the formulas written out here, optimizer configs, and the regularizer identifiers MLP() accepts.  No GPU."""
import numpy as np
import pytest

from GNN import optimizers, regularizers
from GNN.MLP import MLP

SHAPES = [(7, 5), (5,), (5, 3), (3,), (3,), (2,)]
SCALES = [3.0, 0.1, 1.0, 0.01, 2.0, 0.3]          # arrays above and below every threshold used below


def _arrays(seed):
    rng = np.random.default_rng(seed)
    grads = [(c * rng.standard_normal(s)).astype(np.float32) for s, c in zip(SHAPES, SCALES)]
    return grads, [rng.standard_normal(s).astype(np.float32) for s in SHAPES]


def _clip(grads, clipvalue=None, clipnorm=None, global_clipnorm=None):
    """clipvalue, then clipnorm per array, then global_clipnorm over all arrays, in float64."""
    out = []
    for g in grads:
        g = np.array(g, np.float64)
        if clipvalue is not None:
            g = np.minimum(np.maximum(g, -clipvalue), clipvalue)
        if clipnorm is not None:
            g = g * clipnorm / max(np.linalg.norm(g.ravel()), clipnorm)
        out.append(g)
    if global_clipnorm is not None:
        norm = np.sqrt(sum(float(np.sum(g * g)) for g in out))
        out = [g * global_clipnorm / max(norm, global_clipnorm) for g in out]
    return out


def _make(name, **clip):
    return optimizers.Adam(0.01, **clip) if name == 'Adam' else optimizers.SGD(0.01, momentum=0.9, **clip)


@pytest.mark.parametrize('name', ['Adam', 'SGD'])
@pytest.mark.parametrize('clip', [dict(clipvalue=0.3), dict(clipnorm=0.8), dict(global_clipnorm=1.5), dict(clipvalue=0.3, clipnorm=0.4)])
def test_apply_gradients_clips_as_defined(name, clip):
    """Two steps (the second one runs on non-zero slots): a clipping optimizer on the raw gradients == a plain one on the gradients
    clipped here."""
    clipping, plain = _make(name, **clip), _make(name)
    _, w1 = _arrays(0)
    w2 = [a.copy() for a in w1]
    for step in range(2):
        grads, _ = _arrays(10 + step)
        want = _clip(grads, **clip)
        assert any(np.max(np.abs(a - b)) > 1e-3 for a, b in zip(want, grads))          # the thresholds are active
        w1 = clipping.apply_gradients(zip(grads, w1))
        w2 = plain.apply_gradients(zip(want, w2))
        for a, b in zip(w1, w2):
            assert a.dtype == np.float32 and np.max(np.abs(a.astype(np.float64) - b)) <= 1e-7 * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize('name', ['Adam', 'SGD'])
def test_thresholds_above_every_norm_change_nothing(name):
    grads, w = _arrays(1)
    top = 10.0 * np.sqrt(sum(float(np.sum(np.square(g, dtype=np.float64))) for g in grads))
    for clip in (dict(clipvalue=top, clipnorm=top), dict(clipvalue=top, global_clipnorm=top)):
        a = _make(name, **clip).apply_gradients(zip(grads, w))
        b = _make(name).apply_gradients(zip(grads, w))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('cls', [optimizers.Adam, optimizers.SGD])
def test_clipping_arguments_are_checked(cls):
    with pytest.raises(ValueError):
        cls(0.01, clipnorm=1, global_clipnorm=1)
    for name in ('clipnorm', 'clipvalue', 'global_clipnorm'):
        for bad in (0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError):
                cls(0.01, **{name: bad})


def test_configs_list_clipping_only_when_set():
    assert optimizers.Adam(0.01).get_config() == dict(learning_rate=0.01, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    assert optimizers.SGD(0.1, 0.5).get_config() == dict(learning_rate=0.1, momentum=0.5)
    assert optimizers.serialize(optimizers.Adam(0.01)) == {'class_name': 'Adam', 'config': dict(learning_rate=0.01, beta_1=0.9, beta_2=0.999, epsilon=1e-7)}
    back = optimizers.deserialize(optimizers.serialize(optimizers.Adam(0.01, clipnorm=0.5)))
    assert isinstance(back, optimizers.Adam) and back.clipnorm == 0.5 and back.clipvalue is None and back.global_clipnorm is None
    assert back.get_config()['clipnorm'] == 0.5 and back.device_clip_args() == (0.0, 0.5, 0.0)
    back = optimizers.deserialize(optimizers.serialize(optimizers.SGD(0.1, clipvalue=2.0, global_clipnorm=3.0)))
    assert back.device_clip_args() == (2.0, 0.0, 3.0) and optimizers.SGD(0.1).device_clip_args() == (0.0, 0.0, 0.0)


def test_regularizer_identifiers():
    assert regularizers.get(None) is None
    assert regularizers.get('l2') == regularizers.L1L2(l2=0.01) and regularizers.get('l1') == regularizers.L1L2(l1=0.01)
    assert regularizers.get('l1_l2') == regularizers.L1L2(0.01, 0.01)
    reg = regularizers.l2(0.3)
    assert regularizers.get(reg) is reg
    with pytest.raises(ValueError):
        regularizers.get('l3')
    net = MLP(5, [4, 3], 'tanh', 'zeros', 'zeros', kernel_regularizer='l1_l2')
    assert len(net.dense_layers) == 2
    for layer in net.dense_layers:
        assert layer.kernel_regularizer == regularizers.L1L2(0.01, 0.01) and layer.bias_regularizer is None
    assert regularizers.device_coefficients(net.dense_layers) == ([0.01, 0.0, 0.01, 0.0], [0.01, 0.0, 0.01, 0.0])


def test_device_coefficients_leave_custom_regularizers_to_the_host():
    class Mine(regularizers.L1L2):
        def __call__(self, w):
            return 2.0 * super().__call__(w)

    plain = MLP(5, [4, 3], 'tanh', 'zeros', 'zeros')
    assert regularizers.device_coefficients(plain.dense_layers) == ([0.0] * 4, [0.0] * 4)
    mixed = MLP(5, [4, 3], 'tanh', 'zeros', 'zeros', kernel_regularizer=[regularizers.l1(0.2), None], bias_regularizer=[None, regularizers.l2(0.3)])
    assert regularizers.device_coefficients(mixed.dense_layers) == ([0.2, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.3])
    custom = MLP(5, [4, 3], 'tanh', 'zeros', 'zeros', kernel_regularizer=[regularizers.l1(0.2), Mine(l2=0.1)])
    assert regularizers.device_coefficients(custom.dense_layers) is None
