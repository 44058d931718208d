"""Host side of the optimizers, losses and learning-rate schedules of the device training step: the float64 mirrors in
GNN/optimizers.py against torch.optim where the rules coincide exactly and against a second spelling where they do not, the losses
against finite differences, the schedules against their closed forms.  `loss64` below is the float64 statement of the loss kinds
of include/gnn_hip.h that tests/test_gpu_train_rules.py holds the device against."""
import math

import numpy as np
import pytest

EPS_K = 1e-7

LOSS_KINDS = {'cce': 0, 'mse': 1, 'cce_logits': 2, 'bce': 3, 'bce_logits': 4, 'mae': 5, 'huber': 6}


def loss64(name, targets, out, weights, smoothing=0.0, delta=1.0):
    """(sum_i w_i L(t_i, o_i), d / d o [n, T]) in float64, written from the definitions in include/gnn_hip.h."""
    t, o, w = np.asarray(targets, np.float64), np.asarray(out, np.float64), np.asarray(weights, np.float64)
    T = o.shape[-1]
    if name in ('cce', 'cce_logits'): t = t * (1 - smoothing) + smoothing / T
    if name in ('bce', 'bce_logits'): t = t * (1 - smoothing) + smoothing / 2
    if name == 'cce':
        s = o.sum(-1, keepdims=True)
        p = o / s
        inside = (p >= EPS_K) & (p <= 1 - EPS_K)
        pc = np.clip(p, EPS_K, 1 - EPS_K)
        L = -(t * np.log(pc)).sum(-1)
        gp = np.where(inside, -t / pc, 0.0)
        d = (gp - (gp * p).sum(-1, keepdims=True)) / s
    elif name == 'cce_logits':
        z = o - o.max(-1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(-1, keepdims=True))
        L = -(t * logp).sum(-1)
        d = np.exp(logp) * t.sum(-1, keepdims=True) - t
    elif name == 'bce':
        inside = (o >= EPS_K) & (o <= 1 - EPS_K)
        pc = np.clip(o, EPS_K, 1 - EPS_K)
        L = -(t * np.log(pc) + (1 - t) * np.log(1 - pc)).mean(-1)
        d = np.where(inside, (1 - t) / (1 - pc) - t / pc, 0.0) / T
    elif name == 'bce_logits':
        L = (np.maximum(o, 0) - o * t + np.log1p(np.exp(-np.abs(o)))).mean(-1)
        d = (1 / (1 + np.exp(-o)) - t) / T
    elif name == 'mae':
        L = np.abs(o - t).mean(-1)
        d = np.sign(o - t) / T
    elif name == 'huber':
        e = o - t
        quad = np.abs(e) <= delta
        L = np.where(quad, e * e / 2, delta * (np.abs(e) - delta / 2)).mean(-1)
        d = np.where(quad, e, delta * np.sign(e)) / T
    elif name == 'mse':
        L = ((o - t) ** 2).mean(-1)
        d = 2 * (o - t) / T
    else:
        raise ValueError(name)
    return float(np.sum(w * L)), d * w[:, None]


def loss_inputs(name, rng, n, T=3):
    """float32 (targets, outputs) for a loss: probabilities / logits / regression values away from the kinks and the clip range."""
    if name == 'cce':
        o = rng.uniform(0.05, 1.0, (n, T))
        return np.eye(T)[rng.integers(0, T, n)].astype(np.float32), (o / o.sum(-1, keepdims=True)).astype(np.float32)
    if name == 'cce_logits':
        return np.eye(T)[rng.integers(0, T, n)].astype(np.float32), rng.uniform(-3, 3, (n, T)).astype(np.float32)
    if name == 'bce':
        return rng.integers(0, 2, (n, T)).astype(np.float32), rng.uniform(0.05, 0.95, (n, T)).astype(np.float32)
    if name == 'bce_logits':
        z = rng.uniform(0.1, 4, (n, T)) * rng.choice([-1.0, 1.0], (n, T))
        return rng.integers(0, 2, (n, T)).astype(np.float32), z.astype(np.float32)
    t = rng.uniform(-1, 1, (n, T))
    gap = rng.choice([-1.0, 1.0], (n, T)) * np.where(rng.random((n, T)) < 0.5, rng.uniform(0.05, 0.25, (n, T)), rng.uniform(0.35, 1.0, (n, T)))
    return t.astype(np.float32), (t + gap).astype(np.float32)      # |o - t| stays 0.05 away from 0 and from delta = 0.3


def edge_rows():
    """{loss: (targets, outputs, what the row is about)} at the clip limits and the kinks, T = 3."""
    big = np.float32(1) - np.float32(1e-8)                         # rounds to 1 in float32: clipped like 1
    return {'bce': (np.array([[1, 0, 1], [0, 1, 0]], np.float32), np.array([[0, 1e-8, 1], [big, 1, 0]], np.float32)),
            'mae': (np.array([[0.25, -0.5, 1]], np.float32), np.array([[0.25, -0.5, 1]], np.float32)),
            'huber': (np.array([[0, 0, 0]], np.float32), np.array([[0.5, -0.5, 0.5]], np.float32))}      # |e| == delta = 0.5 exactly


CASES = [('bce', 0.0), ('bce', 0.2), ('bce_logits', 0.0), ('bce_logits', 0.2), ('mae', 0.0), ('huber', 0.0), ('cce', 0.1), ('cce_logits', 0.1),
         ('cce', 1.0)]


# ---- optimizers -------------------------------------------------------------------------------------------------------
def _run_mirror(opt, p0, grads):
    trace = []
    p64 = p0.copy()
    for g in grads:                         # apply_gradients returns float32 arrays: _update is the same arithmetic, kept in float64
        slots = opt._slots
        if slots is None:
            opt._slots = slots = [[np.zeros_like(p64) for _ in range(opt._n_slots)]]
        p64 = opt._update(p64, g, slots[0], opt._rate(), opt.iterations + 1)
        opt.iterations += 1
        trace.append(p64.copy())
    return trace


def _problem(seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(7), [rng.standard_normal(7) for _ in range(5)]


@pytest.mark.parametrize('name', ['sgd_nesterov', 'rmsprop', 'rmsprop_centered', 'adagrad'])
def test_host_mirrors_match_torch_where_the_rules_coincide(name):
    torch = pytest.importorskip('torch')
    from GNN import optimizers
    p0, grads = _problem()
    mine, theirs = {
        'sgd_nesterov': (lambda: optimizers.SGD(0.01, momentum=0.9, nesterov=True), lambda p: torch.optim.SGD([p], lr=0.01, momentum=0.9, nesterov=True)),
        'rmsprop': (lambda: optimizers.RMSprop(0.001, rho=0.9, epsilon=1e-7), lambda p: torch.optim.RMSprop([p], lr=0.001, alpha=0.9, eps=1e-7)),
        'rmsprop_centered': (lambda: optimizers.RMSprop(0.001, rho=0.9, epsilon=1e-7, centered=True),
                             lambda p: torch.optim.RMSprop([p], lr=0.001, alpha=0.9, eps=1e-7, centered=True)),
        'adagrad': (lambda: optimizers.Adagrad(0.001, initial_accumulator_value=0.1, epsilon=1e-7),
                    lambda p: torch.optim.Adagrad([p], lr=0.001, initial_accumulator_value=0.1, eps=1e-7)),
    }[name]
    trace = _run_mirror(mine(), p0, grads)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    topt = theirs(tp)
    worst = 0.0
    for g, want in zip(grads, trace):
        tp.grad = torch.tensor(g, dtype=torch.float64)
        topt.step()
        worst = max(worst, float(np.max(np.abs(tp.detach().numpy() - want))))
    print(name, 'largest difference', worst)
    assert worst <= 1e-12


def _second_spelling(name, p0, grads, lr, h):
    """Entry by entry with Python floats, from the rule table of include/gnn_hip.h."""
    out = []
    p = [float(x) for x in p0]
    s = [[0.0, 0.0, 0.0] for _ in p]
    for t, g in enumerate(grads, 1):
        for i, gi in enumerate(g):
            gi = float(gi)
            if name == 'amsgrad':
                b1, b2, eps = h
                s[i][0] = b1 * s[i][0] + (1 - b1) * gi
                s[i][1] = b2 * s[i][1] + (1 - b2) * gi * gi
                s[i][2] = max(s[i][2], s[i][1])
                p[i] -= lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) * s[i][0] / (math.sqrt(s[i][2]) + eps)
            elif name == 'adamax':
                b1, b2, eps = h
                s[i][0] = b1 * s[i][0] + (1 - b1) * gi
                s[i][1] = max(b2 * s[i][1], abs(gi))
                p[i] -= lr / (1 - b1 ** t) * s[i][0] / (s[i][1] + eps)
            else:
                rho, mom, eps, centered = h
                s[i][0] = rho * s[i][0] + (1 - rho) * gi * gi
                den = s[i][0]
                if centered:
                    s[i][2] = rho * s[i][2] + (1 - rho) * gi
                    den = max(s[i][0] - s[i][2] ** 2, 0.0)
                s[i][1] = mom * s[i][1] + lr * gi / math.sqrt(den + eps)
                p[i] -= s[i][1]
        out.append(np.array(p))
    return out


@pytest.mark.parametrize('name', ['rmsprop_momentum', 'rmsprop_momentum_centered', 'amsgrad', 'adamax'])
def test_host_mirrors_match_a_second_spelling(name):
    from GNN import optimizers
    p0, grads = _problem(1)
    if name == 'amsgrad':
        opt, want = optimizers.Adam(0.01, 0.9, 0.99, 1e-7, amsgrad=True), _second_spelling('amsgrad', p0, grads, 0.01, (0.9, 0.99, 1e-7))
    elif name == 'adamax':
        opt, want = optimizers.Adamax(0.01, 0.9, 0.99, 1e-7), _second_spelling('adamax', p0, grads, 0.01, (0.9, 0.99, 1e-7))
    else:
        c = name.endswith('centered')
        opt, want = optimizers.RMSprop(0.01, 0.9, 0.8, 1e-7, centered=c), _second_spelling('rmsprop', p0, grads, 0.01, (0.9, 0.8, 1e-7, c))
    worst = max(float(np.max(np.abs(a - b))) for a, b in zip(_run_mirror(opt, p0, grads), want))
    print(name, 'largest difference', worst)
    assert worst <= 1e-12


def test_apply_gradients_is_the_float32_image_of_the_rule_and_counts_steps():
    """apply_gradients (what the host path calls) goes through the same _update, clips first, keeps slots per array and counts."""
    from GNN import optimizers
    p0, grads = _problem(2)
    for make in (lambda **kw: optimizers.RMSprop(0.01, momentum=0.5, centered=True, **kw), lambda **kw: optimizers.Adagrad(0.01, **kw),
                 lambda **kw: optimizers.Adamax(0.01, **kw), lambda **kw: optimizers.Adam(0.01, amsgrad=True, **kw),
                 lambda **kw: optimizers.SGD(0.01, 0.9, nesterov=True, **kw)):
        opt, ref = make(clipvalue=0.5), make()
        p = [p0.astype(np.float32), p0[:3].astype(np.float32)]
        for g in grads[:3]:
            new = opt.apply_gradients([(g, p[0]), (g[:3], p[1])])
            want = ref.apply_gradients([(np.clip(g, -0.5, 0.5), p[0]), (np.clip(g[:3], -0.5, 0.5), p[1])])
            assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(new, want))
            assert np.array_equal(new[0][:3], new[1])                    # the slots of the two arrays are separate and alike
            p = new
        assert opt.iterations == 3 and not np.array_equal(p[0], p0.astype(np.float32))


def test_device_step_arguments():
    from GNN import optimizers
    assert optimizers.SGD(0.1, 0.9).device_step_args() == (0, [0.1, 0.9])                 # as before: the third value defaults to 0
    assert optimizers.SGD(0.1, 0.9, nesterov=True).device_step_args() == (0, [0.1, 0.9, 1.0])
    assert optimizers.Adam(0.01, amsgrad=True).device_step_args()[0] == 2 and optimizers.Adam(0.01).device_step_args()[0] == 1
    assert optimizers.RMSprop(0.01, 0.8, 0.5, 1e-6).device_step_args() == (3, [0.01, 0.8, 0.5, 1e-6])
    assert optimizers.RMSprop(centered=True).device_step_args()[0] == 4
    assert optimizers.Adagrad(0.01, 0.2, 1e-6).device_step_args() == (5, [0.01, 0.2, 1e-6])
    opt = optimizers.Adamax(0.01, 0.9, 0.99, 1e-6)
    assert opt.device_step_args() == (6, [0.01 / (1 - 0.9), 0.9, 0.99, 1e-6])
    opt.device_step_done()
    assert opt.device_step_args()[1][0] == 0.01 / (1 - 0.9 ** 2)
    for bad in (lambda: optimizers.RMSprop(epsilon=-1.0), lambda: optimizers.RMSprop(momentum=float('nan')),
                lambda: optimizers.Adagrad(initial_accumulator_value=-0.1), lambda: optimizers.Adamax(epsilon=float('inf'))):
        with pytest.raises(ValueError):
            bad()


# ---- losses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,smoothing', CASES)
def test_loss_gradients_match_central_differences(name, smoothing):
    rng = np.random.default_rng(7)
    t, o = loss_inputs(name, rng, 8)
    w = rng.uniform(0.5, 1.5, 8)
    o = o.astype(np.float64)
    delta = 0.3
    _, d = loss64(name, t, o, w, smoothing, delta)
    fd = np.zeros_like(d)
    h = 1e-6
    for idx in np.ndindex(*o.shape):
        up, dn = o.copy(), o.copy()
        up[idx] += h; dn[idx] -= h
        fd[idx] = (loss64(name, t, up, w, smoothing, delta)[0] - loss64(name, t, dn, w, smoothing, delta)[0]) / (2 * h)
    err = float(np.max(np.abs(fd - d))) / float(np.max(np.abs(d)))
    print(name, smoothing, 'relative error', err)
    assert err <= 1e-6
    if name == 'huber':
        e = np.abs(o - t)
        assert (e < delta).any() and (e > delta).any()


@pytest.mark.parametrize('name,smoothing', CASES)
def test_numpy_losses_agree_with_the_float64_losses(name, smoothing):
    from GNN import losses
    rng = np.random.default_rng(8)
    t, o = loss_inputs(name, rng, 64)
    fn, args = {'bce': (losses.binary_crossentropy, {}), 'bce_logits': (losses.binary_crossentropy, {'from_logits': True}),
                'mae': (losses.mean_absolute_error, {}), 'huber': (losses.huber, {'delta': 0.3}), 'cce': (losses.categorical_crossentropy, {}),
                'cce_logits': (losses.categorical_crossentropy, {'from_logits': True})}[name]
    if smoothing: args = dict(args, label_smoothing=smoothing)
    rows = fn(t, o, **args)
    assert rows.shape == (64,)
    assert losses.device_loss_kind(fn, args) == LOSS_KINDS[name]
    assert losses.device_loss_params(fn, args) == (smoothing, 0.3 if name == 'huber' else 1.0)
    worst = max(abs(float(rows[i]) - loss64(name, t[i:i + 1], o[i:i + 1], [1.0], smoothing, 0.3)[0]) for i in range(64))
    print(name, smoothing, 'largest difference', worst)
    assert worst <= 1e-6


def test_loss_edges_by_value():
    from GNN import losses
    rows = edge_rows()
    t, o = rows['bce']
    loss, d = loss64('bce', t, o, [1.0, 1.0])
    assert np.isfinite(loss) and np.all(d == 0.0)                    # p in {0, 1e-8, 1 - 1e-8, 1}: clipped, so no gradient
    assert np.isfinite(losses.binary_crossentropy(t, o)).all()
    t, o = rows['mae']
    loss, d = loss64('mae', t, o, [1.0])
    assert loss == 0.0 and np.all(d == 0.0)                          # sign(0) = 0
    assert losses.mean_absolute_error(t, o)[0] == 0.0 and losses.mae is losses.mean_absolute_error
    t, o = rows['huber']
    loss, d = loss64('huber', t, o, [1.0], delta=0.5)
    assert loss == 0.125 and np.array_equal(d[0], np.array([0.5, -0.5, 0.5]) / 3)        # |e| == delta: e^2 / 2, gradient e
    assert losses.huber(t, o, delta=0.5)[0] == np.float32(0.125)
    # label smoothing 1 with T = 3: every target is 1 / 3, whatever it was
    o = np.array([[0.2, 0.3, 0.5]], np.float32)
    a = loss64('cce', [[1, 0, 0]], o, [1.0], smoothing=1.0)
    b = loss64('cce', [[1 / 3, 1 / 3, 1 / 3]], o, [1.0])
    assert abs(a[0] - b[0]) <= 1e-15 and np.max(np.abs(a[1] - b[1])) <= 1e-15
    assert abs(float(losses.categorical_crossentropy([[0, 0, 1]], o, label_smoothing=1.0)[0]) - b[0]) <= 1e-6
    with pytest.raises(ValueError):
        losses.categorical_crossentropy([[0, 0, 1]], o, label_smoothing=1.5)
    with pytest.raises(ValueError):
        losses.huber(t, o, delta=0.0)


# ---- schedules and configs ----------------------------------------------------------------------------------------------
def test_schedules_match_their_closed_forms_and_round_trip():
    from GNN import optimizers
    S = optimizers.schedules
    cases = [
        (S.ExponentialDecay(0.01, 2, 0.5), {0: 0.01, 1: 0.01 * 0.5 ** 0.5, 3: 0.01 * 0.5 ** 1.5}),
        (S.ExponentialDecay(0.01, 2, 0.5, staircase=True), {0: 0.01, 1: 0.01, 2: 0.005, 3: 0.005, 4: 0.0025}),
        (S.InverseTimeDecay(0.02, 5, 0.5), {0: 0.02, 1: 0.02 / 1.1, 6: 0.02 / 1.6}),
        (S.InverseTimeDecay(0.02, 5, 0.5, staircase=True), {0: 0.02, 1: 0.02, 4: 0.02, 5: 0.02 / 1.5, 6: 0.02 / 1.5}),
        (S.PiecewiseConstantDecay([2, 4], [1.0, 0.5, 0.1]), {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.5, 4: 0.5, 5: 0.1, 50: 0.1}),
        (S.CosineDecay(0.1, 4), {0: 0.1, 1: 0.05 * (1 + math.cos(math.pi / 4)), 4: 0.0, 5: 0.0}),
        (S.CosineDecay(0.1, 4, alpha=0.2), {0: 0.1, 1: 0.1 * (0.8 * 0.5 * (1 + math.cos(math.pi / 4)) + 0.2), 5: 0.02}),
    ]
    for sched, want in cases:
        for step, rate in want.items():
            assert abs(sched(step) - rate) <= 1e-15, (type(sched).__name__, step, sched(step), rate)
        for make in (optimizers.Adam, optimizers.SGD, optimizers.RMSprop, optimizers.Adagrad, optimizers.Adamax):
            opt = make(sched)
            import json
            back = optimizers.deserialize(json.loads(json.dumps(optimizers.serialize(opt))))      # (a model's save / load goes through JSON)
            assert type(back) is type(opt) and type(back.learning_rate) is type(sched) and back.get_config() == opt.get_config()
            assert [back.learning_rate(s) for s in range(8)] == [sched(s) for s in range(8)]
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([2, 4], [1.0, 0.5])


def test_the_rate_of_a_step_is_the_schedule_at_the_iteration_count():
    from GNN import optimizers
    sched = optimizers.schedules.ExponentialDecay(0.01, 2, 0.5, staircase=True)
    opt = optimizers.SGD(sched)
    seen = []
    for _ in range(5):
        seen.append(opt.device_step_args()[1][0])
        assert opt.device_step_args()[1][0] == seen[-1]              # asking twice (a failed step is retried) does not advance it
        opt.device_step_done()
    assert seen == [0.01, 0.01, 0.005, 0.005, 0.0025]
    adam = optimizers.Adam(sched, 0.9, 0.999)
    for t in range(1, 4):
        assert adam.device_step_args()[1][0] == sched(t - 1) * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        adam.device_step_done()
    host = optimizers.SGD(sched)                                       # the host path counts the same way
    p = np.zeros(1, np.float32)
    for want in seen:
        new = host.apply_gradients([(np.ones(1), p)])
        assert abs(float(p[0] - new[0][0]) - want) <= 1e-8           # (p is stored as float32: two roundings of 2^-25 |p|, |p| < 0.04)
        p = new[0]


def test_configs_of_the_existing_optimizers_are_unchanged():
    from GNN import optimizers
    assert optimizers.Adam(0.01).get_config() == {'learning_rate': 0.01, 'beta_1': 0.9, 'beta_2': 0.999, 'epsilon': 1e-7}
    assert list(optimizers.Adam(0.01).get_config()) == ['learning_rate', 'beta_1', 'beta_2', 'epsilon']
    assert optimizers.SGD(0.01, momentum=0.9).get_config() == {'learning_rate': 0.01, 'momentum': 0.9}
    assert list(optimizers.SGD(0.01, momentum=0.9, clipnorm=1.0).get_config()) == ['learning_rate', 'momentum', 'clipnorm']
    assert optimizers.Adam(0.01, amsgrad=True).get_config()['amsgrad'] is True and optimizers.SGD(0.01, nesterov=True).get_config()['nesterov'] is True
    for opt in (optimizers.Adam(0.01, amsgrad=True), optimizers.SGD(0.01, 0.9, nesterov=True, clipvalue=0.5), optimizers.RMSprop(0.01, centered=True, momentum=0.5),
                optimizers.Adagrad(0.01, global_clipnorm=2.0), optimizers.Adamax(0.01)):
        back = optimizers.deserialize(optimizers.serialize(opt))
        assert type(back) is type(opt) and back.get_config() == opt.get_config() and back.device_step_args() == opt.device_step_args()
