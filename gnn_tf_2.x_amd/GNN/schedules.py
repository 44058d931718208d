"""Learning-rate schedules standing in for tf.keras.optimizers.schedules (reachable as GNN.optimizers.schedules): an optimizer's
``learning_rate`` may be one of these objects.  The rate of a step is ``schedule(iterations)`` with the optimizer's step counter,
counted from 0; the device step receives it as an ordinary per-step hyper-parameter, so a schedule costs nothing on the device."""
import math


class LearningRateSchedule:
    def __call__(self, step) -> float:
        raise NotImplementedError

    def get_config(self) -> dict:
        return dict(self._config)


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ^ (step / decay_steps); staircase: the exponent is floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self._config = dict(initial_learning_rate=initial_learning_rate, decay_steps=decay_steps, decay_rate=decay_rate, staircase=staircase)
        self.initial_learning_rate, self.decay_steps, self.decay_rate, self.staircase = initial_learning_rate, decay_steps, decay_rate, staircase

    def __call__(self, step):
        p = step / self.decay_steps
        return float(self.initial_learning_rate * self.decay_rate ** (math.floor(p) if self.staircase else p))


class InverseTimeDecay(LearningRateSchedule):
    """initial_learning_rate / (1 + decay_rate * step / decay_steps); staircase: step / decay_steps is floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False):
        self._config = dict(initial_learning_rate=initial_learning_rate, decay_steps=decay_steps, decay_rate=decay_rate, staircase=staircase)
        self.initial_learning_rate, self.decay_steps, self.decay_rate, self.staircase = initial_learning_rate, decay_steps, decay_rate, staircase

    def __call__(self, step):
        p = step / self.decay_steps
        return float(self.initial_learning_rate / (1 + self.decay_rate * (math.floor(p) if self.staircase else p)))


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] while step <= boundaries[0], values[i] while boundaries[i - 1] < step <= boundaries[i], values[-1] beyond."""

    def __init__(self, boundaries, values):
        boundaries, values = list(boundaries), list(values)
        if len(values) != len(boundaries) + 1:
            raise ValueError('PiecewiseConstantDecay needs one value more than boundaries')
        self._config = dict(boundaries=boundaries, values=values)
        self.boundaries, self.values = boundaries, values

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return float(v)
        return float(self.values[-1])


class CosineDecay(LearningRateSchedule):
    """initial_learning_rate * ((1 - alpha) * (1 + cos(pi * min(step, decay_steps) / decay_steps)) / 2 + alpha)."""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0):
        self._config = dict(initial_learning_rate=initial_learning_rate, decay_steps=decay_steps, alpha=alpha)
        self.initial_learning_rate, self.decay_steps, self.alpha = initial_learning_rate, decay_steps, alpha

    def __call__(self, step):
        cosine = 0.5 * (1 + math.cos(math.pi * min(step, self.decay_steps) / self.decay_steps))
        return float(self.initial_learning_rate * ((1 - self.alpha) * cosine + self.alpha))


_CLASSES = {c.__name__: c for c in (ExponentialDecay, InverseTimeDecay, PiecewiseConstantDecay, CosineDecay)}


def serialize(schedule) -> dict:
    return {'class_name': type(schedule).__name__, 'config': schedule.get_config()}


def deserialize(d):
    return _CLASSES[d['class_name']](**d['config'])
