"""GNN models with the reference's public surface (``GNN/GNN.py``), running ``Loop`` on the MI355X.

``Loop(g)`` = reference GNN.py:251-280: loop-invariant aggregates, iterate ``state <- net_state([state | labels |
Adjacency^T.state | aggregated labels])`` while some node moved by more than ``threshold`` (relative L2, strict '>') and
``k < max_iteration``, then ``net_output`` on the rows selected by ``set_mask & output_mask``.  The whole loop is one
call into ``libgnn_hip.so`` (``gnn_loop_run``); Python only converts the graph once and copies results back.

Extensions over the reference signature (needed because TensorFlow's RNG stream cannot be reproduced):
``Loop(g, training=False, state0=None)`` takes an injected initial state for ``state_vect_dim > 0``; without it the
engine draws N(0, 0.1^2) from its own generator seeded by ``self.seed``.
"""
from __future__ import annotations

import weakref
from typing import Optional, Union

import numpy as np

from GNN import _engine
from GNN.GNN_BaseClass import BaseClass
from GNN.MLP import Sequential, clone_model
from GNN.graph_class import GraphObject, GraphTensor


class GNNnodeBased(BaseClass):
    """GNN for node-based problems."""

    def __init__(self, net_state: Sequential, net_output: Sequential, optimizer, loss_function, loss_arguments: Optional[dict],
                 state_vect_dim: int, max_iteration: int, threshold: float, addressed_problem: str,
                 extra_metrics: Optional[dict] = None, extra_metrics_arguments: Optional[dict[str, dict]] = None,
                 path_writer: str = 'writer/', namespace: str = 'GNN') -> None:
        if not isinstance(state_vect_dim, int) or state_vect_dim < 0: raise TypeError('param <state_vect_dim> must be int>=0')
        super().__init__(optimizer, loss_function, loss_arguments, addressed_problem, extra_metrics, extra_metrics_arguments,
                         path_writer, namespace)
        self.net_state = net_state
        self.net_output = net_output
        self.max_iteration = max_iteration
        self.state_threshold = threshold
        self.state_vect_dim = state_vect_dim
        self.seed = 0
        self.device = 0
        self.impl = 2           # 2: fused kernel, fp16-split MFMA (fastest, fp32-accurate); 1: fused, bit-exact f32 MFMA; 0: one kernel per TF op
        self.gradient_mode = 'unrolled'     # set_gradient_mode
        self.adjoint_max_iteration = None
        self.adjoint_threshold = None
        self.adjoint_batch_normalization = None     # set_gradient_mode(..., batch_normalization='frozen')
        self.adjoint_label_gradients = False        # set_gradient_mode(..., label_gradients=True)
        self.adjoint_solver = 'picard'              # set_gradient_mode(..., adjoint_solver='anderson', anderson_window=5)
        self.anderson_window = 5
        self.label_projection = 'off'       # set_label_projection
        self.train_recompute = False        # set_train_recompute
        self.wide_state = 'off'             # set_wide_state

    def set_train_recompute(self, enable: bool) -> None:
        """Activation recomputation in the unrolled training step (off by default).  Back-propagation through the unrolled loop keeps every
        body's activations from the forward pass until the backward pass reaches them - memory that grows with max_iteration.  With this
        on, the forward keeps each body's output state alone and the backward pass rebuilds a body's activations right before it walks the
        body: one more forward pass per body, the same loss and gradients bit for bit.  Works with every net the unrolled step handles
        (BatchNormalization, Dropout, all three GNN types, the LGNN joint steps); without effect in gradient mode 'fixed_point'.
        Kept by copy() (so by LKO) and by save() / load()."""
        if not isinstance(enable, bool): raise ValueError('param <enable> must be a bool')
        self.train_recompute = enable

    def set_label_projection(self, mode) -> None:
        """The fused Loop for wide node / arc labels.  The fused kernels hold a node's whole net_state input in on-chip memory, which
        caps it at about 144 columns (with state_vect_dim 64: about 7 node-label columns); wider inputs run one kernel per operation.
        With the projection the label terms of net_state's first layer are computed once per Loop and every iteration runs that layer
        over [state | aggregated state] only.  'off' / 0 (default), 'auto' / 1: where the fused path does not cover the net as it
        stands, 'always' / 2: wherever applicable.  A form of the default arithmetic (impl 2): states and outputs within 1e-5 of the
        reference, the iteration count the exact one; impl 1 / 0 and training-mode Loops run as without it.  Kept by copy() (so by LKO)
        and by save() / load()."""
        code = _engine.label_projection_mode(mode)
        self.label_projection = {v: k for k, v in _engine.LABEL_PROJECTION_MODES.items()}[code]

    def set_wide_state(self, mode) -> None:
        """The fused Loop for state_vect_dim 68 .. 128.  The fused kernels keep the net_state input of 32 nodes per wave in on-chip memory,
        eight waves per workgroup, and [state | aggregated state] alone is past that for a state wider than 72: such a model runs one
        kernel per operation.  With this form the iteration kernel runs on 4 to 7 waves per workgroup, as many as fit, and loads its tiles
        with a loader for wide rows.  'off' / 0 (default), 'auto' / 1: where it was measured faster than one kernel per operation,
        'always' / 2: wherever it is covered.  state_vect_dim a multiple of 4; with about a dozen label columns at 128, or any label width
        together with set_label_projection.  The arithmetic per node is unchanged (impl 1 stays bit-exact, impl 2 within 1e-5);
        training-mode Loops run as without it.  Kept by copy() (so by LKO) and by save() / load()."""
        code = _engine.wide_state_mode(mode)
        self.wide_state = {v: k for k, v in _engine.WIDE_STATE_MODES.items()}[code]

    def set_gradient_mode(self, mode: str, max_iteration: Optional[int] = None, threshold: Optional[float] = None, *,
                          batch_normalization: Optional[str] = None, label_gradients: bool = False, adjoint_solver: str = 'picard',
                          anderson_window: int = 5) -> None:
        """How train() differentiates the state loop.  'unrolled' (default): back-propagation through every executed body.
        'fixed_point': the gradient at the converged state (Almeida-Pineda; Scarselli et al. 2009, section III) - the inference Loop
        finds the state, ONE body is recorded there, the adjoint iteration z <- g + J^T z runs until no node's z moves by more than
        ``threshold`` (relative L2, default: the model's state threshold) or ``max_iteration`` iterations (default: the model's), and one
        weight-gradient pass with the final z gives net_state's gradients.  These are not a sum over bodies: ``mean`` does NOT divide them
        by the iteration count.  Needs a net_state without Dropout and BatchNormalization (NotImplementedError); net_output is free.
        ``batch_normalization='frozen'`` (opt-in; None by default) accepts a net_state that ends in BatchNormalization - what MLP() builds by
        default - and runs that layer on its MOVING statistics, as in fine-tuning: this is the map the inference Loop iterates, a per-row
        affine map.  gamma and beta train like any other array; the moving statistics of net_state are NOT updated by train() in this mode
        (net_output's are).  Dropout in net_state stays refused.
        ``label_gradients=True`` (opt-in; False by default): the fixed-point backward pass also returns the gradient with respect to the node
        labels (edge-based: and the arc labels) this model saw - the direct part through net_output plus (d body / d labels)^T z at the fixed
        point.  It is what the joint steps of an LGNN ('parallel' / 'residual') hand from layer i + 1 to layer i; needs state_vect_dim > 0.
        ``adjoint_solver='anderson'`` (opt-in; 'picard' by default): the adjoint system (I - J^T) z = g is solved by Anderson mixing over the last
        ``anderson_window`` (1 .. 8, default 5) difference pairs of the iteration instead of the plain iteration, whose count grows like
        1 / (1 - rho) with rho the spectral radius contraction_estimate() reports: the same stopping rule on the residual, a fraction of the
        iterations where rho is close to 1, the same count where it is small.  The gradients agree with 'picard' to the threshold, not bit for bit,
        and the step takes 2 window + 2 more scratch buffers of [nodes, state_vect_dim] floats.  It presumes a contraction as the mode itself
        does: without one the Loop has no fixed point and the gradient means nothing.  Both keywords combine with the two above; in 'unrolled'
        mode they are stored and have no effect, as ``max_iteration`` / ``threshold``.
        Kept by copy() (so by LKO) and by save() / load()."""
        if mode not in ('unrolled', 'fixed_point'): raise ValueError("param <mode> not in ['unrolled', 'fixed_point']")
        if batch_normalization not in (None, 'frozen'): raise ValueError("param <batch_normalization> not in [None, 'frozen']")
        if not isinstance(label_gradients, bool): raise ValueError('param <label_gradients> must be a bool')
        if adjoint_solver not in ('picard', 'anderson'): raise ValueError("param <adjoint_solver> not in ['picard', 'anderson']")
        if isinstance(anderson_window, bool) or not isinstance(anderson_window, (int, np.integer)) or not 1 <= int(anderson_window) <= 8:
            raise ValueError('param <anderson_window> must be an int in [1, 8]')
        if mode == 'fixed_point' and label_gradients and self.state_vect_dim == 0:
            raise NotImplementedError('fixed_point label gradients need state_vect_dim > 0: with 0 the unrolled label gradient is the gradient of '
                                      'the INITIAL state, which a fixed point does not depend on')
        if mode == 'fixed_point' and any(float(r) != 0.0 for r in self.net_state.dropout_rates()):
            raise NotImplementedError('fixed_point gradients need a net_state without Dropout and BatchNormalization: its training-mode '
                                      'forward must be the inference forward')
        if mode == 'fixed_point' and self.net_state.batch_normalization and batch_normalization is None:
            raise NotImplementedError('fixed_point gradients need a net_state without Dropout and BatchNormalization: its training-mode '
                                      "forward must be the inference forward (batch_normalization='frozen' runs it on its moving statistics)")
        if max_iteration is not None and int(max_iteration) < 1: raise ValueError('param <max_iteration> must be >= 1 or None')
        if threshold is not None and not float(threshold) >= 0.0: raise ValueError('param <threshold> must be >= 0 or None')
        self.gradient_mode = mode
        self.adjoint_max_iteration = None if max_iteration is None else int(max_iteration)
        self.adjoint_threshold = None if threshold is None else float(threshold)
        self.adjoint_batch_normalization = batch_normalization
        self.adjoint_label_gradients = label_gradients
        self.adjoint_solver = adjoint_solver
        self.anderson_window = int(anderson_window)

    def contraction_estimate(self, g: Union[GraphObject, GraphTensor], iterations: int = 32, v0=None, seed: int = 0) -> dict:
        """How far net_state's map is from a contraction on graph ``g`` at the state the Loop finds - the condition under which
        'fixed_point' gradients (and the Loop itself, near its fixed point) converge.  Power iteration on J^T, J = d body / d state at that
        state with BatchNormalization on its moving statistics: ``growth[t]`` = |J^T v_t| over the unit vectors the iteration runs through,
        started from ``v0`` [nodes, state_vect_dim] or (None) normal draws keyed on ``seed``.  Returns dict(growth, done, k, last, rho,
        contractive): ``rho``, the geometric mean of the later half of growth, estimates the spectral radius of J, ``contractive`` is
        rho < 1, ``k`` the Loop's iteration count, ``done`` < iterations says the vector became 0 (or not finite) there.  Works in either
        gradient mode and changes nothing of the model.  Needs state_vect_dim > 0 and a net_state without Dropout (NotImplementedError);
        ``iterations`` from 1 to 1024 (ValueError).  An LGNN layer is estimated on the relabelled graph (update_graph)."""
        iterations = int(iterations)
        if not 1 <= iterations <= 1024: raise ValueError('param <iterations> must lie in [1, 1024]')
        if self.state_vect_dim == 0:
            raise NotImplementedError('contraction_estimate needs state_vect_dim > 0: with 0 the Loop iterates on the node labels themselves')
        if any(float(r) != 0.0 for r in self.net_state.dropout_rates()):
            raise NotImplementedError('contraction_estimate needs a net_state without Dropout: the map the inference Loop iterates')
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        loop = self._device_loop(g.device_graph(self.device))
        self._prepare_loop(g, loop)
        loop.set_state0(None, self.seed)
        return loop.contraction_estimate(self.net_state.device_mlp(self.device), iterations, v0, seed, dropout_state=self.net_state.dropout_rates())

    def _gradient_config(self) -> dict:
        config = {'mode': self.gradient_mode, 'max_iteration': self.adjoint_max_iteration, 'threshold': self.adjoint_threshold}
        # (written only when set: the dicts and files of models without it are what they were)
        if self.adjoint_batch_normalization is not None: config['batch_normalization'] = self.adjoint_batch_normalization
        if self.adjoint_label_gradients: config['label_gradients'] = True
        if self.adjoint_solver != 'picard' or self.anderson_window != 5: config.update(adjoint_solver=self.adjoint_solver, anderson_window=self.anderson_window)
        return config

    def _frozen_state_bn(self) -> bool:
        """net_state's BatchNormalization runs on its moving statistics in train(): they are not updated."""
        return self.gradient_mode == 'fixed_point' and self.adjoint_batch_normalization == 'frozen'

    # ---- copies, weights ---------------------------------------------------------------------------------------------
    def copy(self, *, path_writer: str = '', namespace: str = '', copy_weights: bool = True):
        optimizer = self.optimizer
        if hasattr(optimizer, 'get_config'):
            optimizer = optimizer.__class__(**optimizer.get_config())
        new = self.__class__(net_state=clone_model(self.net_state, copy_weights), net_output=clone_model(self.net_output, copy_weights),
                             optimizer=optimizer, loss_function=self.loss_function, loss_arguments=self.loss_args,
                             max_iteration=self.max_iteration, threshold=self.state_threshold,
                             addressed_problem=self.addressed_problem, extra_metrics=self.extra_metrics,
                             extra_metrics_arguments=self.mt_args, state_vect_dim=self.state_vect_dim,
                             path_writer=path_writer or self.path_writer + '_copied/', namespace=namespace or 'GNN')
        new.set_gradient_mode(self.gradient_mode, self.adjoint_max_iteration, self.adjoint_threshold, batch_normalization=self.adjoint_batch_normalization,
                              label_gradients=self.adjoint_label_gradients, adjoint_solver=self.adjoint_solver, anderson_window=self.anderson_window)
        new.set_label_projection(self.label_projection)
        new.set_train_recompute(self.train_recompute)
        new.set_wide_state(self.wide_state)
        return new

    def save(self, path: str):
        """Save the model to folder <path>, without extra_metrics (reference GNN.py:93-111; the reference writes two Keras
        SavedModels, here: architecture + weights of each net as JSON + .npz)."""
        import json, os
        from GNN import losses, optimizers
        from GNN.MLP import sequential_config
        if path[-1] != '/': path += '/'
        os.makedirs(path, exist_ok=True)
        for name, net in (('net_state', self.net_state), ('net_output', self.net_output)):
            np.savez(f'{path}{name}.npz', *net.get_weights())
            with open(f'{path}{name}.json', 'w') as f:
                json.dump(sequential_config(net), f)
        loss_name = getattr(self.loss_function, '__name__', None)
        with open(f'{path}config.json', 'w') as f:
            json.dump({'loss_function': loss_name if hasattr(losses, str(loss_name)) else None, 'loss_arguments': self.loss_args,
                       'optimizer': optimizers.serialize(self.optimizer), 'max_iteration': self.max_iteration, 'threshold': self.state_threshold,
                       'addressed_problem': self.addressed_problem, 'state_vect_dim': self.state_vect_dim,
                       'gradient_mode': self._gradient_config(), 'label_projection': self.label_projection,
                       'train_recompute': self.train_recompute, 'wide_state': self.wide_state}, f)

    @classmethod
    def load(cls, path: str, path_writer=None, namespace: str = 'GNN', extra_metrics=None, extra_metrics_arguments=None):
        """Load a model saved by save() (reference GNN.py:114-149, same arguments): the GNN type is the calling class."""
        import json
        from GNN import losses, optimizers
        from GNN.MLP import sequential_from_config
        if path[-1] != '/': path += '/'
        if path_writer is None: path_writer = f'{path}writer'
        with open(f'{path}config.json') as f:
            config = json.load(f)
        optz = optimizers.deserialize(config.pop('optimizer', None))
        loss_name = config.pop('loss_function', None)
        loss = getattr(losses, loss_name) if loss_name else None
        gradient = config.pop('gradient_mode', None) or {'mode': 'unrolled'}      # (a model saved before the mode existed: unrolled)
        projection = config.pop('label_projection', None) or 'off'                # (a model saved before the key existed: off)
        recompute = bool(config.pop('train_recompute', False))                    # (likewise)
        wide_state = config.pop('wide_state', None) or 'off'                      # (likewise)
        nets = []
        for name in ('net_state', 'net_output'):
            with open(f'{path}{name}.json') as f:
                arch = json.load(f)
            with np.load(f'{path}{name}.npz') as z:
                weights = [z[f'arr_{i}'] for i in range(len(z.files))]
            nets.append(sequential_from_config(arch, weights))
        model = cls(net_state=nets[0], net_output=nets[1], optimizer=optz, loss_function=loss, extra_metrics=extra_metrics,
                    extra_metrics_arguments=extra_metrics_arguments, path_writer=path_writer, namespace=namespace, **config)
        model.set_gradient_mode(gradient['mode'], gradient.get('max_iteration'), gradient.get('threshold'),
                                batch_normalization=gradient.get('batch_normalization'), label_gradients=bool(gradient.get('label_gradients', False)),
                                adjoint_solver=gradient.get('adjoint_solver', 'picard'), anderson_window=int(gradient.get('anderson_window', 5)))
        model.set_label_projection(projection)
        model.set_train_recompute(recompute)
        model.set_wide_state(wide_state)
        return model

    def get_dense_layers(self):
        return self.net_state.dense_layers + self.net_output.dense_layers

    def trainable_variables(self):
        return [self.net_state.trainable_variables], [self.net_output.trainable_variables]

    def get_weights(self):
        return [self.net_state.get_weights()], [self.net_output.get_weights()]

    def set_weights(self, weights_state, weights_output) -> None:
        assert len(weights_state) == len(weights_output) == 1
        self.net_state.set_weights(weights_state[0])
        self.net_output.set_weights(weights_output[0])

    # ---- inference -----------------------------------------------------------------------------------------------------
    def __call__(self, g: Union[GraphObject, GraphTensor]):
        return self.Loop(g, training=False)[-1]

    def evaluate_single_graph(self, g: Union[GraphObject, GraphTensor], training: bool) -> tuple:
        """(iterations, summed loss, targets, output) of one graph (reference GNN.py:180-199)."""
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        targs = self.get_filtered_tensor(g, g.targets)
        loss_weights = self.get_filtered_tensor(g, g.sample_weights)
        it, _, out = self.Loop(g, training=training, _want_state=False)      # the state (N x Ds floats) is not needed here: stays on the device
        loss = self.loss_function(targs, out, **self.loss_args) * loss_weights
        return it, np.sum(loss), targs, out

    def _device_loop(self, dev_graph: _engine.Graph) -> _engine.Loop:
        """One gnn_loop per (this model, device graph), created on first use."""
        cache = dev_graph.__dict__.setdefault('_loops', {})
        # the C loop is configured once: a changed max_iteration / state_threshold / state_vect_dim needs a new one
        key = (id(self), int(self.max_iteration), float(self.state_threshold), int(self.state_vect_dim))
        owner, loop = cache.get(key, (None, None))
        if owner is None or owner() is not self:
            for old in [k for k in cache if k[0] == id(self)]:
                del cache[old]
            loop = _engine.Loop(dev_graph, self.net_state.device_mlp(self.device), self.net_output.device_mlp(self.device),
                                self.state_vect_dim, self.max_iteration, self.state_threshold)
            cache[key] = (weakref.ref(self), loop)
        if getattr(loop, '_impl_set', None) != self.impl:      # (gnn_loop_set_impl checks the fused path, which re-packs the weight images when the weights
            loop.set_impl(self.impl)                          #  have changed - 0.17 ms after every optimizer step; the next inference Loop packs them anyway)
            loop._impl_set = self.impl
        gradient = (self.gradient_mode, self.adjoint_max_iteration, self.adjoint_threshold, self.adjoint_batch_normalization, self.adjoint_label_gradients)
        if getattr(loop, '_gradient_set', ('unrolled', None, None, None, False)) != gradient:
            # (the flags belong to the fixed-point modes; an unrolled model that carries the keywords sets the plain mode)
            fixed = gradient[0] != 'unrolled'
            loop.set_gradient_mode(*gradient[:3], batch_normalization=gradient[3] if fixed else None, label_gradients=gradient[4] if fixed else False)
            loop._gradient_set = gradient
        solver = (self.adjoint_solver, self.anderson_window) if self.gradient_mode != 'unrolled' else ('picard', 5)
        if getattr(loop, '_solver_set', ('picard', 5)) != solver:
            loop.set_adjoint_solver(*solver)
            loop._solver_set = solver
        if getattr(loop, '_projection_set', 'off') != self.label_projection:
            loop.set_label_projection(self.label_projection)
            loop._projection_set = self.label_projection
        if getattr(loop, '_wide_state_set', 'off') != self.wide_state:
            loop.set_wide_state(self.wide_state)
            loop._wide_state_set = self.wide_state
        if getattr(loop, '_recompute_set', False) != self.train_recompute:
            loop.set_train_recompute(self.train_recompute)
            loop._recompute_set = self.train_recompute
        return loop

    def _prerun(self, graphs) -> list:
        """evaluate() over several graphs (reference GNN_BaseClass.py:165-189 walks them one after the other): their device Loops in ONE
        gnn_loop_run_many call - the persistent launches of small graphs run side by side - and the Loop() calls that follow take these
        results instead of running again.  Returns the loops it marked (evaluate clears the marks when it is done)."""
        if len(graphs) < 2 or not all(isinstance(g, GraphTensor) for g in graphs):
            return []
        loops = [self._device_loop(g.device_graph(self.device)) for g in graphs]
        if len({id(lp) for lp in loops}) != len(loops):
            return []                                       # the same graph twice in the list: one after the other, as before
        if self.state_vect_dim > 0:
            for lp in loops: lp.set_state0(None, self.seed)
        for lp, k in zip(loops, _engine.Loop.run_many(loops)):
            lp._fresh = k
        return loops

    def _run(self, dev_graph: _engine.Graph, training: bool, state0) -> tuple[float, _engine.Loop]:
        loop = self._device_loop(dev_graph)
        if not training and state0 is None and getattr(loop, '_fresh', None) is not None:
            k, loop._fresh = loop._fresh, None              # run by _prerun a moment ago, with these weights and this initial state
            return k, loop
        if self.state_vect_dim > 0:
            loop.set_state0(state0, self.seed)
        if training:
            return self._train_forward(loop), loop
        return loop.run(False), loop

    def _train_forward(self, loop) -> float:
        """Loop(training=True) (reference GNN.py:251-280 with the Keras layers in training mode): Dropout with fresh masks,
        BatchNormalization on batch statistics (the moving statistics are updated as Keras does on every training-mode call).
        The loop then holds the training-mode state / outputs."""
        self._train_calls = getattr(self, '_train_calls', 0) + 1
        # gamma / beta are read from the device copies (bn_state = None) and the moving statistics are updated there as well
        k, _ = loop.train_forward(self.net_state.device_mlp(self.device), self.net_output.device_mlp(self.device), None,
                                  dropout_state=self.net_state.dropout_rates(), dropout_output=self.net_output.dropout_rates(),
                                  seed=self.seed * 1000003 + self._train_calls, bn_state=None, bn_output=None)
        loop.update_moving_statistics(getattr(self.net_state.layers[-1], 'momentum', 0.99), getattr(self.net_output.layers[-1], 'momentum', 0.99))
        if self.net_state.batch_normalization: self.net_state.mark_device_newer()
        if self.net_output.batch_normalization: self.net_output.mark_device_newer()
        return k

    # ---- training -------------------------------------------------------------------------------------------------------
    _graph_based = False

    def training_step(self, g: GraphTensor, mean: bool, *, state0=None, masks_state=None, masks_output=None) -> dict:
        """One batch: device gradients (gnn_loop_train_step), net_state gradients divided by the iteration count when
        ``mean`` (reference GNN_BaseClass.py:241; not in gradient mode 'fixed_point', whose gradients are no sum over bodies), optimizer update, BatchNormalization moving statistics.  L1L2 kernel / bias
        regularizers, the optimizer's clipvalue / clipnorm / global_clipnorm and the loss with its label_smoothing / delta
        (``loss_arguments``) are part of the device step.  Returns the raw
        result of the device step (loss with the penalty, k, gradients with the regularizer terms) for inspection."""
        from GNN import losses
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        if self.optimizer is None or not hasattr(self.optimizer, 'apply_gradients'):
            raise TypeError('train() needs an optimizer with apply_gradients, e.g. GNN.optimizers.Adam()')
        kind = losses.device_loss_kind(self.loss_function, self.loss_args)
        if self._graph_based and not g.loop_mask().all():
            raise ValueError('graph-based GNN needs set_mask and output_mask all True')
        loop = self._device_loop(g.device_graph(self.device))
        self._prepare_loop(g, loop)
        loop.set_loss_params(*losses.device_loss_params(self.loss_function, self.loss_args))
        if self.state_vect_dim > 0:
            self.seed += 1
            loop.set_state0(state0, self.seed)
        targets = self.get_filtered_tensor(g, g.targets)
        weights = self.get_filtered_tensor(g, g.sample_weights)
        self._train_calls = getattr(self, '_train_calls', 0) + 1
        from GNN import regularizers
        dev_s, dev_o = self.net_state.device_mlp(self.device), self.net_output.device_mlp(self.device)
        # Device-side optimizer step (weights, slots and gradients stay in HBM) when nothing of the step lives on the host: an
        # optimizer that knows the engine's update rules, and kernel / bias regularizers that are L1L2 (or none): their gradients,
        # the penalty and the optimizer's gradient clipping run on the device too.  A custom Regularizer keeps the host path.
        coef_s, coef_o = regularizers.device_coefficients(self.net_state.dense_layers), regularizers.device_coefficients(self.net_output.dense_layers)
        on_device = (getattr(self, 'device_optimizer', True) and coef_s is not None and coef_o is not None
                     and hasattr(self.optimizer, 'device_step_args'))
        step_args = self.optimizer.device_step_args() if on_device else None
        dev_s.set_regularizers(coef_s if step_args is not None else None)       # (host path: the terms are added below, in NumPy)
        dev_o.set_regularizers(coef_o if step_args is not None else None)
        if step_args is not None:
            loop.set_clipping(*self.optimizer.device_clip_args())
            self.net_state.bind_optimizer(self.optimizer)
            self.net_output.bind_optimizer(self.optimizer)
            bn_s, bn_o = self.net_state.layers[-1], self.net_output.layers[-1]
            loop.arm_optimizer(step_args[0], step_args[1], mean, getattr(bn_s, 'momentum', 0.99), getattr(bn_o, 'momentum', 0.99))
        res = loop.train_step(dev_s, dev_o, None, targets, weights,
                              kind, g.nodegraph_csr() if self._graph_based else None, dropout_state=self.net_state.dropout_rates(),
                              dropout_output=self.net_output.dropout_rates(), masks_state=masks_state, masks_output=masks_output,
                              seed=self.seed * 1000003 + self._train_calls,
                              bn_state=None if step_args is not None else self.net_state.bn_gamma_beta(),
                              bn_output=None if step_args is not None else self.net_output.bn_gamma_beta())
        if step_args is not None:
            self.optimizer.device_step_done()          # counted only now: a failed step (exception above) leaves t where it was
            self.net_state.mark_device_newer()
            self.net_output.mark_device_newer()
            return res
        k = res['k']
        # regularizer terms are part of the taped loss (reference GNN_BaseClass.py:223-235): their gradients join the device ones
        for net, key in ((self.net_state, 'grads_state'), (self.net_output, 'grads_output')):
            pen, rg = regularizers.penalty_and_gradients(net.dense_layers)
            res['loss'] += pen
            for li, (gk, gb) in enumerate(rg):
                if gk is not None: res[key][2 * li] = res[key][2 * li] + gk
                if gb is not None: res[key][2 * li + 1] = res[key][2 * li + 1] + gb
        # (fixed-point mode: net_state's gradients are one pass at the converged state, not a sum over k bodies - nothing to average)
        gs = [a / k for a in res['grads_state']] if (mean and k and self.gradient_mode == 'unrolled') else res['grads_state']
        ws, wo = self.net_state.trainable_variables, self.net_output.trainable_variables
        new = self.optimizer.apply_gradients(zip(gs + res['grads_output'], ws + wo))
        self.net_state.set_trainable(new[:len(ws)])
        self.net_output.set_trainable(new[len(ws):])
        # (a frozen BatchNormalization took no batch statistics: its moving statistics stay)
        if not self._frozen_state_bn(): self.net_state.update_moving_statistics(res['bn_batch_state'])
        if loop.n_masked: self.net_output.update_moving_statistics(res['bn_batch_output'])
        return res

    def _prepare_loop(self, g: GraphTensor, loop) -> None:
        """Hook for subclasses that need more than the node mask on the device loop."""

    def Loop(self, g: Union[GraphObject, GraphTensor], *, training: bool = False, state0=None, _want_state: bool = True):
        """(k, state [N, Ds], out [M, T]) with k a float as in the reference (GNN.py:267, :280).  _want_state=False (internal:
        evaluate / test) leaves the state on the device and returns None in its place."""
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        k, loop = self._run(g.device_graph(self.device), training, state0)
        return k, (loop.state() if _want_state else None), loop.output()


class GNNedgeBased(GNNnodeBased):
    """GNN for edge-based problems: node-based state loop, then net_output on [state(i0) | state(i1) | arc label] of the
    arcs selected by set_mask & output_mask (reference GNN.py:286-302; the pairing of index pairs and arc labels by position
    is the reference's)."""

    def _prerun(self, graphs) -> list:
        return []                                           # (the per-arc readout is configured inside Loop: one graph after the other)

    def Loop(self, g: Union[GraphObject, GraphTensor], *, training: bool = False, state0=None, _want_state: bool = True):
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        dev = g.device_graph(self.device)
        loop = self._device_loop(dev)
        self._prepare_loop(g, loop)
        if self.state_vect_dim > 0:
            loop.set_state0(state0, self.seed)
        k = self._train_forward(loop) if training else loop.run(False)
        return k, (loop.state() if _want_state else None), loop.output()

    def _prepare_loop(self, g: GraphTensor, loop, own_labels: bool = False) -> None:
        """own_labels: the loop runs on an LGNN-derived graph, which carries its own (widened) arc labels on the device."""
        if not getattr(loop, '_edge_ready', False):
            entry_dst, arc_labels, mask = g.edge_readout_arrays()
            loop.set_edge_readout(entry_dst, None if own_labels else arc_labels, mask)
            loop._edge_ready = True


class GNNgraphBased(GNNnodeBased):
    """GNN for graph-based problems: node-based Loop followed by the NodeGraph readout (reference GNN.py:318-333)."""

    _graph_based = True

    @staticmethod
    def get_filtered_tensor(g: GraphTensor, inp):
        return np.asarray(inp, dtype=np.float32)      # targets are per graph: never filtered (reference GNN.py:313-315)

    def Loop(self, g: Union[GraphObject, GraphTensor], *, training: bool = False, state0=None, _want_state: bool = True):
        if g.NodeGraph is None: raise ValueError('WRONG GNN. NodeGraph is None: GNN is graph-based, while problem is non graph-based.')
        if isinstance(g, GraphObject): g = GraphTensor.fromGraphObject(g)
        if not g.loop_mask().all():
            # the reference multiplies NodeGraph [N, G] with the masked node outputs [M, T]: a shape error unless M == N
            raise ValueError('graph-based GNN needs set_mask and output_mask all True (NodeGraph rows must match node outputs)')
        k, loop = self._run(g.device_graph(self.device), training, state0)
        return k, (loop.state() if _want_state else None), loop.readout(*g.nodegraph_csr())
