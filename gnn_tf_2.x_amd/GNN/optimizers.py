"""Host-side optimizers standing in for tf.keras.optimizers (reference starter.py:81).  The trainable arrays of the two MLPs
are a few hundred KB, so the update runs in NumPy; gradients come from the device (gnn_loop_train_step)."""
import numpy as np

from GNN import schedules


class Optimizer:
    """Slots (Adam moments, SGD velocity) live either on the device (with the gnn_mlp: gnn_loop_optimizer_step) or on the host
    (apply_gradients), the step counter here.  A model that changes path (a regularizer appears, device_optimizer is toggled) restarts
    BOTH together - slots and counter - like a new Keras optimizer would; `_slot_token` changes then, which makes Sequential.bind_optimizer
    zero the device slots."""
    _path = None
    _slot_token = None
    clipnorm = clipvalue = global_clipnorm = None
    iterations = 0

    def _set_learning_rate(self, learning_rate):
        """A number, or a GNN.optimizers.schedules object (or its serialized dict, as get_config() lists it): the rate of a step is then
        schedule(iterations), iterations counted from 0 and advanced by every successful step."""
        if isinstance(learning_rate, dict):
            learning_rate = schedules.deserialize(learning_rate)
        self.learning_rate = learning_rate
        self._config['learning_rate'] = schedules.serialize(learning_rate) if isinstance(learning_rate, schedules.LearningRateSchedule) else learning_rate

    def _rate(self):
        """The learning rate of the NEXT step."""
        lr = self.learning_rate
        return lr(self.iterations) if isinstance(lr, schedules.LearningRateSchedule) else lr

    def _set_clipping(self, clipnorm, clipvalue, global_clipnorm):
        """The tf.keras optimizer arguments of the same names.  Applied to the gradients of one apply_gradients call in this order:
        clipvalue c: g <- min(max(g, -c), c) per entry; clipnorm c: g_a <- g_a c / max(|g_a|_2, c) per array; global_clipnorm c:
        g <- g c / max(|g|_2, c) with the norm over all arrays of the call.  The order (value, norm, global) is a definition of this
        package, written down from memory of Keras' OptimizerV2: it has not been checked against TensorFlow."""
        if clipnorm is not None and global_clipnorm is not None:
            raise ValueError('clipnorm and global_clipnorm exclude each other (as in tf.keras)')
        for name, v in (('clipnorm', clipnorm), ('clipvalue', clipvalue), ('global_clipnorm', global_clipnorm)):
            if v is None:
                continue
            if not (np.isfinite(v) and v > 0):
                raise ValueError(f'{name} must be finite and > 0, got {v!r}')
            self._config[name] = v          # listed only when set: the configs of optimizers without clipping stay as they were
        self.clipnorm, self.clipvalue, self.global_clipnorm = clipnorm, clipvalue, global_clipnorm

    def device_clip_args(self):
        """(clipvalue, clipnorm, global_clipnorm) of include/gnn_hip.h:gnn_loop_set_clipping, 0 = off."""
        return float(self.clipvalue or 0.0), float(self.clipnorm or 0.0), float(self.global_clipnorm or 0.0)

    def _clipped(self, grads):
        """The host mirror of the device-side clipping (gnn_loop_set_clipping), in float64."""
        grads = [np.asarray(g, np.float64) for g in grads]
        if self.clipvalue is not None:
            grads = [np.clip(g, -self.clipvalue, self.clipvalue) for g in grads]
        if self.clipnorm is not None:
            grads = [g * (self.clipnorm / max(np.sqrt(np.sum(g * g)), self.clipnorm)) for g in grads]
        if self.global_clipnorm is not None:
            f = self.global_clipnorm / max(np.sqrt(sum(np.sum(g * g) for g in grads)), self.global_clipnorm)
            grads = [g * f for g in grads]
        return grads

    def get_config(self):
        return dict(self._config)

    def reset(self):
        self._slot_token = object()
        self.iterations, self._slots = 0, None

    def _enter(self, path):
        if self._path is not None and self._path != path:
            self.reset()
        self._path = path

    def device_step_args(self):
        """(kind, hyper[<= 4]) of include/gnn_hip.h:gnn_loop_arm_optimizer for the NEXT step; None: host only.  The step is counted by
        device_step_done() once it has succeeded (a failed gnn_loop_train_step must not advance the bias correction or a schedule)."""
        return None

    def device_step_done(self):
        self.iterations += 1

    _slots = None
    _n_slots = 1

    def apply_gradients(self, grads_and_vars):
        """[(grad, array)] -> list of updated arrays, in order (arrays are identified by position across calls).  The float64 mirror of
        the device rule of the same kind (include/gnn_hip.h, gnn_loop_optimizer_step): _update() per array on the clipped gradients."""
        self._enter('host')
        grads_and_vars = list(grads_and_vars)
        if self._slots is None:
            self._slots = [[np.zeros_like(p, dtype=np.float64) for _ in range(self._n_slots)] for _, p in grads_and_vars]
        lr, t = self._rate(), self.iterations + 1
        out = [self._update(np.asarray(p, np.float64), g, slots, lr, t).astype(np.float32)
               for g, (_, p), slots in zip(self._clipped([g for g, _ in grads_and_vars]), grads_and_vars, self._slots)]
        self.iterations += 1
        return out

    def _update(self, p, g, slots, lr, t):
        """p, g float64; slots: this array's list of float64 slot arrays, updated in place; lr: the rate of this step; t: its number
        from 1.  Returns the new p."""
        raise NotImplementedError


class Adam(Optimizer):
    """Keras Adam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p <- p - lr_t m / (sqrt(v) + epsilon); amsgrad: vhat = max(vhat, v) in place
    of v."""
    _n_slots = 3

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None, clipvalue=None, global_clipnorm=None):
        self._config = dict(learning_rate=learning_rate, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)
        if amsgrad: self._config['amsgrad'] = True         # listed only when set: the config of a plain Adam stays as it was
        self._set_learning_rate(learning_rate)
        self._set_clipping(clipnorm, clipvalue, global_clipnorm)
        self.beta_1, self.beta_2, self.epsilon, self.amsgrad = beta_1, beta_2, epsilon, bool(amsgrad)

    _m = property(lambda self: None if self._slots is None else [s[0] for s in self._slots])      # the host-side moments, per array
    _v = property(lambda self: None if self._slots is None else [s[1] for s in self._slots])

    def _lr_t(self, lr, t):
        return lr * np.sqrt(1 - self.beta_2 ** t) / (1 - self.beta_1 ** t)

    def device_step_args(self):
        self._enter('device')
        return (2 if self.amsgrad else 1), [self._lr_t(self._rate(), self.iterations + 1), self.beta_1, self.beta_2, self.epsilon]

    def _update(self, p, g, slots, lr, t):
        m, v, vhat = slots
        m[...] = self.beta_1 * m + (1 - self.beta_1) * g
        v[...] = self.beta_2 * v + (1 - self.beta_2) * g * g
        if self.amsgrad: vhat[...] = np.maximum(vhat, v)
        return p - self._lr_t(lr, t) * m / (np.sqrt(vhat if self.amsgrad else v) + self.epsilon)


class SGD(Optimizer):
    """v <- momentum v - lr g; p <- p + v, or with nesterov p <- p + momentum v - lr g."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None, global_clipnorm=None):
        self._config = dict(learning_rate=learning_rate, momentum=momentum)
        if nesterov: self._config['nesterov'] = True
        self._set_learning_rate(learning_rate)
        self._set_clipping(clipnorm, clipvalue, global_clipnorm)
        self.momentum, self.nesterov = momentum, bool(nesterov)

    def device_step_args(self):
        self._enter('device')
        return 0, [self._rate(), self.momentum] + ([1.0] if self.nesterov else [])

    def _update(self, p, g, slots, lr, t):
        vel, = slots
        vel[...] = self.momentum * vel - lr * g
        return p + (self.momentum * vel - lr * g if self.nesterov else vel)


class RMSprop(Optimizer):
    """r <- rho r + (1 - rho) g^2; centered: a <- rho a + (1 - rho) g and d = max(r - a^2, 0), else d = r.  momentum == 0:
    p <- p - lr g / (sqrt(d) + epsilon); momentum > 0: q <- momentum q + lr g / sqrt(d + epsilon), p <- p - q.  (The two places of
    epsilon are written down from memory of tf.keras 2.x and have not been checked against TensorFlow.)"""
    _n_slots = 3

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, clipnorm=None, clipvalue=None, global_clipnorm=None):
        if not (np.isfinite(momentum) and momentum >= 0 and np.isfinite(epsilon) and epsilon >= 0):
            raise ValueError('momentum and epsilon must be finite and >= 0')
        self._config = dict(learning_rate=learning_rate, rho=rho, momentum=momentum, epsilon=epsilon, centered=centered)
        self._set_learning_rate(learning_rate)
        self._set_clipping(clipnorm, clipvalue, global_clipnorm)
        self.rho, self.momentum, self.epsilon, self.centered = rho, momentum, epsilon, bool(centered)

    def device_step_args(self):
        self._enter('device')
        return (4 if self.centered else 3), [self._rate(), self.rho, self.momentum, self.epsilon]

    def _update(self, p, g, slots, lr, t):
        r, q, a = slots
        r[...] = self.rho * r + (1 - self.rho) * g * g
        d = r
        if self.centered:
            a[...] = self.rho * a + (1 - self.rho) * g
            d = np.maximum(r - a * a, 0.0)
        if self.momentum > 0:
            q[...] = self.momentum * q + lr * g / np.sqrt(d + self.epsilon)
            return p - q
        return p - lr * g / (np.sqrt(d) + self.epsilon)


class Adagrad(Optimizer):
    """s <- s + g^2 (from zero); p <- p - lr g / (sqrt(initial_accumulator_value + s) + epsilon)."""

    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, clipnorm=None, clipvalue=None, global_clipnorm=None):
        if not (np.isfinite(initial_accumulator_value) and initial_accumulator_value >= 0 and np.isfinite(epsilon) and epsilon >= 0):
            raise ValueError('initial_accumulator_value and epsilon must be finite and >= 0')
        self._config = dict(learning_rate=learning_rate, initial_accumulator_value=initial_accumulator_value, epsilon=epsilon)
        self._set_learning_rate(learning_rate)
        self._set_clipping(clipnorm, clipvalue, global_clipnorm)
        self.initial_accumulator_value, self.epsilon = initial_accumulator_value, epsilon

    def device_step_args(self):
        self._enter('device')
        return 5, [self._rate(), self.initial_accumulator_value, self.epsilon]

    def _update(self, p, g, slots, lr, t):
        s, = slots
        s[...] = s + g * g
        return p - lr * g / (np.sqrt(self.initial_accumulator_value + s) + self.epsilon)


class Adamax(Optimizer):
    """m <- b1 m + (1 - b1) g; u <- max(b2 u, |g|); p <- p - lr / (1 - b1^t) m / (u + epsilon)."""
    _n_slots = 2

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clipvalue=None, global_clipnorm=None):
        if not (np.isfinite(epsilon) and epsilon >= 0):
            raise ValueError('epsilon must be finite and >= 0')
        self._config = dict(learning_rate=learning_rate, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)
        self._set_learning_rate(learning_rate)
        self._set_clipping(clipnorm, clipvalue, global_clipnorm)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon

    def device_step_args(self):
        self._enter('device')
        return 6, [self._rate() / (1 - self.beta_1 ** (self.iterations + 1)), self.beta_1, self.beta_2, self.epsilon]

    def _update(self, p, g, slots, lr, t):
        m, u = slots
        m[...] = self.beta_1 * m + (1 - self.beta_1) * g
        u[...] = np.maximum(self.beta_2 * u, np.abs(g))
        return p - lr / (1 - self.beta_1 ** t) * m / (u + self.epsilon)


def serialize(opt) -> dict:
    """{'class_name', 'config'} (stands in for tf.keras.optimizers.serialize, reference GNN.py:105); a schedule is listed in the
    same form under 'learning_rate'."""
    return {'class_name': type(opt).__name__, 'config': opt.get_config()} if isinstance(opt, Optimizer) else None


def deserialize(d):
    if d is None:
        return None
    return {c.__name__: c for c in (Adam, SGD, RMSprop, Adagrad, Adamax)}[d['class_name']](**d['config'])
