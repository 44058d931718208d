"""Weight regularizers with the call convention of ``tf.keras.regularizers`` (what the reference hands to ``MLP(...,
kernel_regularizer=, bias_regularizer=)``, reference MLP.py:11-13, and sums into the loss in GNN_BaseClass.py:223-228).
L1L2 regularizers run on the device with the rest of the training step (``device_coefficients`` -> gnn_mlp_set_regularizers);
the NumPy code here is their host mirror, and the path of a custom ``Regularizer`` subclass."""
from __future__ import annotations

import numpy as np


class Regularizer:
    def __call__(self, w) -> float:
        raise NotImplementedError

    def gradient(self, w) -> np.ndarray:
        raise NotImplementedError


class L1L2(Regularizer):
    def __init__(self, l1: float = 0.0, l2: float = 0.0):
        self.l1, self.l2 = float(l1), float(l2)

    def __call__(self, w) -> float:
        w = np.asarray(w, dtype=np.float64)
        return float(self.l1 * np.sum(np.abs(w)) + self.l2 * np.sum(w * w))

    def gradient(self, w) -> np.ndarray:
        w = np.asarray(w, dtype=np.float64)
        return (self.l1 * np.sign(w) + 2.0 * self.l2 * w).astype(np.float32)

    def get_config(self):
        return dict(l1=self.l1, l2=self.l2)

    def __eq__(self, other):
        return type(other) is type(self) and (other.l1, other.l2) == (self.l1, self.l2)

    def __hash__(self):
        return hash((type(self), self.l1, self.l2))


def l1(l: float = 0.01) -> L1L2:
    return L1L2(l1=l)


def l2(l: float = 0.01) -> L1L2:
    return L1L2(l2=l)


def l1_l2(l1: float = 0.01, l2: float = 0.01) -> L1L2:
    return L1L2(l1=l1, l2=l2)


def get(identifier):
    """``None``, a ``Regularizer`` (or any callable with ``.gradient``), or one of the Keras names 'l1', 'l2', 'l1_l2' (Keras defaults,
    0.01), as tf.keras.regularizers.get; the reference starter hands strings to MLP() (starter.py:55-66)."""
    if identifier is None or isinstance(identifier, Regularizer) or callable(identifier):
        return identifier
    if isinstance(identifier, str) and identifier in ('l1', 'l2', 'l1_l2'):
        return {'l1': l1, 'l2': l2, 'l1_l2': l1_l2}[identifier]()
    raise ValueError(f'unknown regularizer {identifier!r}')


def device_coefficients(dense_layers):
    """([l1 per array], [l2 per array]) in [W1, b1, W2, b2, ...] order for gnn_mlp_set_regularizers (0 where a layer has none), or
    ``None`` when some regularizer is not exactly an L1L2 with finite coefficients >= 0: that model keeps the host path."""
    c1, c2 = [], []
    for layer in dense_layers:
        for reg in (layer.kernel_regularizer, layer.bias_regularizer):
            if reg is None:
                c1.append(0.0); c2.append(0.0)
            elif type(reg) is L1L2 and np.isfinite(reg.l1) and np.isfinite(reg.l2) and reg.l1 >= 0 and reg.l2 >= 0:
                c1.append(reg.l1); c2.append(reg.l2)
            else:
                return None
    return c1, c2


def penalty_and_gradients(dense_layers) -> tuple[float, list]:
    """Sum of the penalties of ``dense_layers`` (reference GNN_BaseClass.py:223-228) and, per layer, the pair of gradients
    (d / d kernel, d / d bias), ``None`` where a layer has no regularizer."""
    total, grads = 0.0, []
    for layer in dense_layers:
        gk = gb = None
        for reg, attr in ((layer.kernel_regularizer, 'kernel'), (layer.bias_regularizer, 'bias')):
            if reg is None:
                continue
            if not (callable(reg) and hasattr(reg, 'gradient')):
                raise TypeError('regularizers must come from GNN.regularizers (a callable with a .gradient(w) method)')
            w = getattr(layer, attr)
            total += reg(w)
            if attr == 'kernel': gk = reg.gradient(w)
            else: gb = reg.gradient(w)
        grads.append((gk, gb))
    return total, grads


def any_regularizer(dense_layers) -> bool:
    return any(l.kernel_regularizer is not None or l.bias_regularizer is not None for l in dense_layers)
