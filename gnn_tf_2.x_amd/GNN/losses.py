"""NumPy stand-ins for the tf.keras.losses callables the starter passes as ``loss_function`` (reference starter.py:82).
They act on host arrays AFTER the device loop; they are not part of the hot path."""
import numpy as np

_EPS = 1e-7   # Keras backend epsilon


def _smoothed(y_true, label_smoothing, classes):
    """Keras label smoothing: t <- t (1 - s) + s / classes (classes = the row width for categorical, 2 for binary targets)."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f'label_smoothing must lie in [0, 1], got {label_smoothing!r}')
    return y_true * np.float32(1.0 - label_smoothing) + np.float32(label_smoothing / classes) if label_smoothing else y_true


def categorical_crossentropy(y_true, y_pred, from_logits: bool = False, label_smoothing: float = 0.0, **_):
    y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    y_true = _smoothed(y_true, label_smoothing, y_true.shape[-1])
    if from_logits:
        z = y_pred - y_pred.max(axis=-1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=-1, keepdims=True))
    else:
        p = y_pred / y_pred.sum(axis=-1, keepdims=True)
        logp = np.log(np.clip(p, _EPS, 1 - _EPS))
    return -(y_true * logp).sum(axis=-1)


def binary_crossentropy(y_true, y_pred, from_logits: bool = False, label_smoothing: float = 0.0, **_):
    y = _smoothed(np.asarray(y_true, np.float32), label_smoothing, 2)
    if from_logits:
        z = np.asarray(y_pred, np.float32)
        return (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean(axis=-1)
    p = np.clip(np.asarray(y_pred, np.float32), _EPS, 1 - _EPS)
    return -(y * np.log(p) + (1 - y) * np.log(1 - p)).mean(axis=-1)


def mean_squared_error(y_true, y_pred, **_):
    return np.square(np.asarray(y_pred, np.float32) - np.asarray(y_true, np.float32)).mean(axis=-1)


def mean_absolute_error(y_true, y_pred, **_):
    return np.abs(np.asarray(y_pred, np.float32) - np.asarray(y_true, np.float32)).mean(axis=-1)


def huber(y_true, y_pred, delta: float = 1.0, **_):
    """e = y_pred - y_true: mean of e^2 / 2 where |e| <= delta, delta (|e| - delta / 2) beyond."""
    if not (np.isfinite(delta) and delta > 0):
        raise ValueError(f'delta must be finite and > 0, got {delta!r}')
    e = np.abs(np.asarray(y_pred, np.float32) - np.asarray(y_true, np.float32))
    d = np.float32(delta)
    return np.where(e <= d, 0.5 * e * e, d * (e - 0.5 * d)).mean(axis=-1)


mse = mean_squared_error
mae = mean_absolute_error


def device_loss_kind(fn, loss_args) -> int:
    """Loss code of gnn_loop_train_step for the callables above (0 categorical_crossentropy, 1 mean_squared_error,
    2 categorical_crossentropy(from_logits=True), 3 binary_crossentropy, 4 binary_crossentropy(from_logits=True),
    5 mean_absolute_error, 6 huber)."""
    if fn is categorical_crossentropy:
        return 2 if loss_args.get('from_logits', False) else 0
    if fn is mean_squared_error:
        return 1
    if fn is binary_crossentropy:
        return 4 if loss_args.get('from_logits', False) else 3
    if fn is mean_absolute_error:
        return 5
    if fn is huber:
        return 6
    raise NotImplementedError(f'training with loss {getattr(fn, "__name__", fn)!r} is not implemented on the MI355X engine '
                              f'(available: GNN.losses.categorical_crossentropy, binary_crossentropy, mean_squared_error, '
                              f'mean_absolute_error, huber)')


def device_loss_params(fn, loss_args) -> tuple:
    """(label_smoothing, huber_delta) of gnn_loop_set_loss_params / gnn_loss_grad_ex for the callable and its loss_arguments: the
    smoothing of the two crossentropies, the delta of huber, the defaults (0, 1) otherwise."""
    smoothing = float(loss_args.get('label_smoothing', 0.0)) if fn in (categorical_crossentropy, binary_crossentropy) else 0.0
    delta = float(loss_args.get('delta', 1.0)) if fn is huber else 1.0
    return smoothing, delta
