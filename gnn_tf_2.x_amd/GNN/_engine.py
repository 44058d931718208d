"""ctypes binding of include/gnn_hip.h (libgnn_hip.so).  This is the only door from Python into the product.

There is no CPU fallback: if the library is missing or no MI355X is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GNN_HIP_LIBRARY: another build of the same library (the diagnostic build `make DIAG=1` -> libgnn_hip_diag.so); never a fallback
LIB_PATH = os.environ.get('GNN_HIP_LIBRARY') or os.path.join(_HERE, 'libgnn_hip.so')

ACT_CODES = {'linear': 0, None: 0, 'relu': 1, 'selu': 2, 'elu': 3, 'tanh': 4, 'sigmoid': 5, 'softmax': 6}

EXPORTS = ['gnn_last_error', 'gnn_version', 'gnn_device_count', 'gnn_device_synchronize', 'gnn_graph_create', 'gnn_graph_create_from_arcs',
           'gnn_graph_derive', 'gnn_graph_derive_edge', 'gnn_graph_set_arc_order', 'gnn_graph_update_labels', 'gnn_graph_get_nodes', 'gnn_graph_dims', 'gnn_graph_destroy',
           'gnn_mlp_create', 'gnn_mlp_set_weights', 'gnn_mlp_get_weights', 'gnn_mlp_reset_optimizer', 'gnn_mlp_forward', 'gnn_mlp_destroy', 'gnn_loop_create',
           'gnn_loop_set_state0', 'gnn_loop_run', 'gnn_loop_get_state', 'gnn_loop_get_output', 'gnn_loop_readout', 'gnn_loop_set_edge_readout', 'gnn_loop_train_step',
           'gnn_loop_train_forward', 'gnn_loop_train_backward', 'gnn_loop_arm_optimizer', 'gnn_loop_optimizer_step', 'gnn_loop_update_moving_statistics', 'gnn_loss_grad',
           'gnn_loss_grad_ex', 'gnn_loop_set_loss_params', 'gnn_train_forms', 'gnn_loop_train_forms', 'gnn_loop_train_mask', 'gnn_fused_net_form', 'gnn_small_form',
           'gnn_loop_set_train_persistent', 'gnn_train_persistent_form', 'gnn_loop_train_info',
           'gnn_loop_set_train_recompute', 'gnn_loop_train_recompute_info',
           'gnn_loop_set_gradient_mode', 'gnn_loop_adjoint_info', 'gnn_adjoint_form', 'gnn_loop_train_arena_bytes',
           'gnn_loop_set_gradient_mode_ex', 'gnn_adjoint_form_ex', 'gnn_loop_adjoint_z', 'gnn_loop_train_backward_chained',
           'gnn_loop_contraction_estimate', 'gnn_loop_contraction_vector', 'gnn_loop_set_adjoint_solver', 'gnn_loop_adjoint_solver_info',
           'gnn_mlp_set_regularizers', 'gnn_loop_set_clipping', 'gnn_loop_grad_sqnorm', 'gnn_loop_optimizer_step_scaled',
           'gnn_counters_get', 'gnn_lgnn_run', 'gnn_loop_run_many', 'gnn_loop_set_impl', 'gnn_loop_gate_info', 'gnn_loop_set_pieces', 'gnn_loop_range_info', 'gnn_split_f16_exponent', 'gnn_split_f16', 'gnn_loop_set_persistent', 'gnn_loop_set_tile_form', 'gnn_loop_body_kernel', 'gnn_loop_set_gather_form', 'gnn_gather_program_build', 'gnn_graph_gather_program_info', 'gnn_gather_program_compact', 'gnn_graph_gather_program_format', 'gnn_graph_set_program_entries', 'gnn_loop_set_tile_schedule', 'gnn_loop_set_label_projection', 'gnn_loop_get_label_projection', 'gnn_label_projection_form', 'gnn_loop_set_wide_state', 'gnn_wide_state_form', 'gnn_loop_body_launch', 'gnn_loop_set_grid_limit', 'gnn_loop_set_wide_loader', 'gnn_tile_schedule_build', 'gnn_graph_tile_schedule_info', 'gnn_loop_drop_cached_aggregates', 'gnn_loop_set_profiling', 'gnn_loop_get_timing', 'gnn_loop_get_exchange_timing', 'gnn_loop_destroy', 'gnn_shard_range',
           'gnn_comm_unique_id', 'gnn_comm_create', 'gnn_comm_allreduce_max', 'gnn_comm_destroy', 'gnn_halo_plan', 'gnn_graph_create_halo',
           'gnn_comm_create_loopback', 'gnn_graph_set_full_adjacency', 'gnn_loop_set_slice_exchange', 'gnn_loop_run_group', 'gnn_loop_readout_group', 'gnn_graph_update_labels_group']

_lib = None


class EngineError(RuntimeError):
    pass


def lib():
    """Load libgnn_hip.so once.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                              f'or `make -C gnn_tf_2.x_amd/csrc`')
        _lib = C.CDLL(LIB_PATH)
        _lib.gnn_last_error.restype = C.c_char_p
        for name in EXPORTS:
            if name != 'gnn_last_error':
                getattr(_lib, name).restype = C.c_int
    return _lib


def loss_grad(loss_kind: int, targets, out, sample_weights, label_smoothing: float = 0.0, huber_delta: float = 1.0):
    """gnn_loss_grad_ex: (sum_i w_i L(t_i, out_i), d / d out) for the loss_kind codes of gnn_loop_train_step (GNN.losses.device_loss_kind)."""
    t, o, w = _f32(targets), _f32(out), _f32(sample_weights)
    if t.shape != o.shape or w.shape != (o.shape[0],): raise ValueError(f'targets {t.shape}, outputs {o.shape}, weights {w.shape} do not match')
    d = np.zeros_like(o)
    loss = C.c_double()
    _check(lib().gnn_loss_grad_ex(C.c_int(loss_kind), C.c_int64(o.shape[0]), C.c_int(o.shape[1]), _fp(t), _fp(o), _fp(w), C.c_double(label_smoothing),
                                  C.c_double(huber_delta), C.byref(loss), _fp(d)))
    return float(loss.value), d


FORM_NAMES = {0: 'per_op', 1: 'mlp_fwd', 2: 'wide', 3: 'chain3', 4: 'wgrad_bf', 5: 'wgrad_f32', 6: 'adjoint_narrow'}      # GNN_FORM_* of include/gnn_hip.h


def _forms_dict(out):
    names = [FORM_NAMES[int(v)] for v in out[3:]]
    return dict(forward=names[0::3], backward=names[1::3], wgrad=names[2::3], build_input=bool(out[1]), sweep_rows=int(out[2]))


def train_forms(dims, activations, rates=None, n_rows=0, producer_dropout=True) -> dict:
    """gnn_train_forms (host code, no device): the kernels a net of this description takes in a training step on n_rows rows -
    dict(forward, backward, wgrad: one name of FORM_NAMES per Dense layer; build_input; sweep_rows).  rates: Dropout rate in front of every
    Dense layer and of BatchNormalization (default: none); producer_dropout: net_state (True) or net_output."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    r = _f32(rates if rates is not None else np.zeros(L + 1), (L + 1,))
    out = np.zeros(3 + 3 * L, np.int32)
    _check(lib().gnn_train_forms(C.c_int(L), _ip(d), _ip(a), _fp(r), C.c_int64(int(n_rows)), C.c_int(bool(producer_dropout)), _ip(out)))
    return _forms_dict(out)


ACT_NAMES = {v: k for k, v in ACT_CODES.items() if k is not None}


def fused_net_form(dims, activations, nlc=0) -> dict:
    """gnn_fused_net_form (host code, no device): what the fused inference paths make of a net_state of this description (nlc: node-label
    columns in the concat) - dict(covered; hidden, last: activation names of the hidden layers and of the last layer; NT, NTL: 32-feature
    tiles of the instantiated kernel; mixed: the last layer has an activation of its own).  A net that is not covered has covered = False
    and None / 0 elsewhere."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    out = np.zeros(6, np.int32)
    _check(lib().gnn_fused_net_form(C.c_int(L), _ip(d), _ip(a), C.c_int(int(nlc)), _ip(out)))
    if not out[0]: return dict(covered=False, hidden=None, last=None, NT=0, NTL=0, mixed=False)
    return dict(covered=True, hidden=ACT_NAMES[int(out[1])], last=ACT_NAMES[int(out[2])], NT=int(out[3]), NTL=int(out[4]), mixed=bool(out[5]))


def small_form(dims, activations, n_rows, nlc=0) -> dict:
    """gnn_small_form (host code, no device): the persistent small-graph launch a net_state of this description takes on n_rows owned
    nodes - dict(persistent; tile: 16 or 32 nodes per tile, 0 when not persistent; wide: the form with hidden layers up to 64 wide;
    steps: first-layer K-steps kept in registers).  Single GPU, not disabled and not profiling are the loop's part of the decision."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    out = np.zeros(3, np.int32)
    _check(lib().gnn_small_form(C.c_int(L), _ip(d), _ip(a), C.c_int(int(nlc)), C.c_int64(int(n_rows)), _ip(out)))
    return dict(persistent=bool(out[0]), tile=int(out[0]), wide=bool(out[1]), steps=int(out[2]))


LABEL_PROJECTION_MODES = {'off': 0, 'auto': 1, 'always': 2}      # modes of gnn_loop_set_label_projection


def label_projection_mode(mode) -> int:
    """'off' | 'auto' | 'always' or 0 | 1 | 2 -> the mode code of gnn_loop_set_label_projection."""
    if isinstance(mode, str):
        if mode not in LABEL_PROJECTION_MODES: raise ValueError("param <mode> not in ['off', 'auto', 'always']")
        return LABEL_PROJECTION_MODES[mode]
    if isinstance(mode, bool) or int(mode) != mode or int(mode) not in (0, 1, 2): raise ValueError('param <mode> not in [0, 1, 2]')
    return int(mode)


def label_projection_form(dims, activations, state_dim, nl, al, n_rows, mode) -> dict:
    """gnn_label_projection_form (host code, no device): what Loop.set_label_projection(mode) answers for a net_state of this description
    (dims[0]: the whole concat) with state width state_dim, nl node-label columns in the concat and al arc-label columns on n_rows owned
    nodes - dict(seeded; kernel: 0, or 1 = k_fused_generic, 2 = k_fused_full; iw: projected label columns; tiles: 32-feature tiles of P).
    impl 2, a single GPU, no feature-sliced exchange and not profiling are the loop's part, taken at their defaults."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    out = np.zeros(4, np.int32)
    _check(lib().gnn_label_projection_form(C.c_int(L), _ip(d), _ip(a), C.c_int(int(state_dim)), C.c_int(int(nl)), C.c_int(int(al)),
                                           C.c_int64(int(n_rows)), C.c_int(label_projection_mode(mode)), _ip(out)))
    return dict(seeded=bool(out[0]), kernel=int(out[1]), iw=int(out[2]), tiles=int(out[3]))


WIDE_STATE_MODES = LABEL_PROJECTION_MODES       # modes of gnn_loop_set_wide_state: the same three
wide_state_mode = label_projection_mode


def wide_state_form(dims, activations, state_dim, nl, al, n_rows, mode, label_projection='off') -> dict:
    """gnn_wide_state_form (host code, no device): what Loop.set_wide_state(mode) answers for a net_state of this description (arguments as
    label_projection_form) with the label projection in mode label_projection - dict(taken; kernel: 0, or 1 = k_fused_generic; waves: waves
    per workgroup of the launch, 4 .. 7; seeded: the launch is the label projection's).  impl 2, a single GPU and no feature-sliced exchange
    are the loop's part, taken at their defaults."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    out = np.zeros(4, np.int32)
    _check(lib().gnn_wide_state_form(C.c_int(L), _ip(d), _ip(a), C.c_int(int(state_dim)), C.c_int(int(nl)), C.c_int(int(al)), C.c_int64(int(n_rows)),
                                     C.c_int(wide_state_mode(mode)), C.c_int(label_projection_mode(label_projection)), _ip(out)))
    return dict(taken=bool(out[0]), kernel=int(out[1]), waves=int(out[2]), seeded=bool(out[3]))


TRAIN_PERSISTENT_MAX_BYTES = 256 << 20      # GNN_TRAIN_PERSISTENT_MAX_BYTES of include/gnn_hip.h


def train_persistent_form(dims, activations, n_rows, max_iter, rates=None) -> dict:
    """gnn_train_persistent_form (host code, no device): whether a net_state of this description runs the training-mode forward of all
    its bodies in ONE persistent launch on n_rows rows, as far as the net, the rows and the byte cap decide - dict(persistent; workgroups;
    rows: rows per workgroup; lds: bytes of LDS per workgroup; body_bytes: what one body's caches count towards TRAIN_PERSISTENT_MAX_BYTES).
    One GPU, allowed, not profiling and "the grid is resident at once" are the loop's part (Loop.set_train_persistent)."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    r = _f32(rates if rates is not None else np.zeros(L + 1), (L + 1,))
    out = np.zeros(5, np.int32)
    _check(lib().gnn_train_persistent_form(C.c_int(L), _ip(d), _ip(a), _fp(r), C.c_int64(int(n_rows)), C.c_int(int(max_iter)), _ip(out)))
    return dict(persistent=bool(out[0]), workgroups=int(out[1]), rows=int(out[2]), lds=int(out[3]), body_bytes=int(out[4]))


SOLVER_NAMES = {0: 'picard', 1: 'anderson'}       # gnn_loop_set_adjoint_solver
SOLVER_CODES = {'picard': 0, 'anderson': 1, 0: 0, 1: 1}
GATHER_NAMES = {0: 'generic', 1: 'rows', 2: 'rows_aligned', 3: 'narrow'}       # gather form of gnn_loop_adjoint_info / gnn_adjoint_form
ADJOINT_REFUSALS = {0: None, 1: 'batch_normalization', 2: 'dropout'}
ADJOINT_FROZEN_BN = 1           # GNN_ADJOINT_FROZEN_BN of include/gnn_hip.h (gnn_loop_set_gradient_mode_ex, gnn_adjoint_form_ex)


ADJOINT_LABEL_GRADIENTS = 2     # GNN_ADJOINT_LABEL_GRADIENTS
KEEP_D_NODES, KEEP_D_ARC_LABELS = 1, 2      # GNN_KEEP_D_NODES, GNN_KEEP_D_ARC_LABELS (gnn_loop_train_backward_chained)


def adjoint_flags(batch_normalization, label_gradients: bool = False) -> int:
    """The flags of gnn_loop_set_gradient_mode_ex for the keywords ``batch_normalization`` (None or 'frozen') and ``label_gradients`` (a bool)
    of the Python layers."""
    if batch_normalization not in (None, 'frozen'): raise ValueError("param <batch_normalization> not in [None, 'frozen']")
    if not isinstance(label_gradients, (bool, np.bool_)): raise ValueError('param <label_gradients> must be a bool')
    return (ADJOINT_FROZEN_BN if batch_normalization == 'frozen' else 0) | (ADJOINT_LABEL_GRADIENTS if label_gradients else 0)
NARROW_REFUSALS = {0: None, 3: 'layers', 4: 'width', 5: 'concat', 6: 'rows', 7: 'softmax'}      # why the one-launch iteration of narrow nets is not taken


def adjoint_form(dims, activations, n_rows, rates=None, batch_normalization=False, *, frozen_bn=None) -> dict:
    """gnn_adjoint_form (host code, no device): what an adjoint iteration of the fixed-point gradient launches for a net_state of this
    description on n_rows rows - dict(eligible; reason: None, 'batch_normalization' or 'dropout'; gather: a name of GATHER_NAMES;
    backward: one name of FORM_NAMES per Dense layer; narrow_refusal: None when an iteration is ONE launch (k_adjoint_narrow), else why
    not: 'layers' (> 3), 'width' (> 64), 'concat' (> 96), 'rows' (>= 4,096 or none), 'softmax').  The state width is dims[-1].
    frozen_bn='frozen' (gnn_adjoint_form_ex with GNN_ADJOINT_FROZEN_BN): the report for a loop set with that flag - a net with
    batch_normalization is then eligible, with the forms of its Dense chain."""
    L = len(dims) - 1
    if L < 1 or len(activations) != L: raise ValueError('dims needs one entry more than activations')
    d = np.ascontiguousarray(dims, np.int32)
    a = np.asarray([ACT_CODES[x] for x in activations], np.int32)
    r = _f32(rates if rates is not None else np.zeros(L + 1), (L + 1,))
    out = np.zeros(4 + L, np.int32)
    flags = adjoint_flags(frozen_bn)
    if flags:
        _check(lib().gnn_adjoint_form_ex(C.c_int(L), _ip(d), _ip(a), _fp(r), C.c_int(bool(batch_normalization)), C.c_int(flags), C.c_int64(int(n_rows)), _ip(out)))
    else:
        _check(lib().gnn_adjoint_form(C.c_int(L), _ip(d), _ip(a), _fp(r), C.c_int(bool(batch_normalization)), C.c_int64(int(n_rows)), _ip(out)))
    return dict(eligible=bool(out[0]), reason=ADJOINT_REFUSALS[int(out[1])], gather=GATHER_NAMES[int(out[2])],
                backward=[FORM_NAMES[int(v)] for v in out[3:3 + L]], narrow_refusal=NARROW_REFUSALS[int(out[3 + L])])


def contraction_summary(growth, done: int, k: float) -> dict:
    """The result dict of Loop.contraction_estimate from what the C call returns (host arithmetic, float64)."""
    g = np.asarray(growth, np.float32)[:done].copy()
    tail = g[done // 2:done].astype(np.float64)
    if done == 0 or np.any(g == 0): rho = 0.0
    else:
        with np.errstate(all='ignore'): rho = float(np.exp(np.mean(np.log(tail))))
    return dict(growth=g, done=int(done), k=float(k), last=float(g[-1]) if done else 0.0, rho=rho, contractive=bool(rho < 1.0))


def split_f16(values, exponent=None):
    """The host-side fp16 x 2 cut of the default path's weight image (gnn_split_f16 / gnn_split_f16_exponent): returns (p0, p1, e) with
    p0 = fp16(v 2^e), p1 = fp16(v 2^e - p0); e defaults to the weight-scale exponent of max |values|."""
    v = np.ascontiguousarray(values, np.float32).ravel()
    if exponent is None:
        exponent = int(lib().gnn_split_f16_exponent(C.c_float(float(np.max(np.abs(v))) if v.size else 0.0)))
    p0, p1 = np.empty(v.size, np.uint16), np.empty(v.size, np.uint16)
    lib().gnn_split_f16(v.ctypes.data_as(C.c_void_p), C.c_int(v.size), C.c_int(int(exponent)), p0.ctypes.data_as(C.c_void_p), p1.ctypes.data_as(C.c_void_p))
    return p0.view(np.float16), p1.view(np.float16), int(exponent)


def _check(rc: int):
    if rc == 0:
        return
    msg = lib().gnn_last_error().decode(errors='replace')
    if rc == -1:
        raise ValueError(msg)
    if rc == -5:
        raise NotImplementedError(msg)
    raise EngineError(f'[gnn_status {rc}] {msg}')


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f'expected shape {tuple(shape)}, got {a.shape}')
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def device_count() -> int:
    n = C.c_int(0)
    _check(lib().gnn_device_count(C.byref(n)))
    return n.value


def require_device(device: int = 0) -> None:
    n = device_count()
    if n <= device:
        raise EngineError(f'no HIP device {device} visible ({n} found): this engine only runs on MI355X (gfx950)')


def shard_range(n_nodes: int, rank: int, world: int) -> tuple[int, int]:
    b, n = C.c_int64(0), C.c_int64(0)
    _check(lib().gnn_shard_range(C.c_int64(n_nodes), C.c_int(rank), C.c_int(world), C.byref(b), C.byref(n)))
    return b.value, n.value


def gather_program(indptr, adj_src, adj_w):
    """gnn_gather_program_build (host code): (hdr [tiles, 2] int32, ent [batches, 64, 2] uint32) of the full 32-row tiles of a CSR graph;
    ent[..., 0] is the source word, ent[..., 1] the weight's bits."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    adj_src = np.ascontiguousarray(adj_src, dtype=np.int32)
    adj_w = _f32(adj_w)
    n_rows = indptr.size - 1
    hdr = np.zeros((n_rows // 32, 2), np.int32)
    nb = C.c_int64(0)
    _check(lib().gnn_gather_program_build(C.c_int64(n_rows), _ip(indptr), _ip(adj_src), _fp(adj_w), _ip(hdr), None, C.byref(nb)))
    ent = np.zeros((nb.value, 64, 2), np.int32)
    _check(lib().gnn_gather_program_build(C.c_int64(n_rows), _ip(indptr), _ip(adj_src), _fp(adj_w), None, _ip(ent), C.byref(nb)))
    return hdr, ent.view(np.uint32)


def gather_program_compact(hdr, ent):
    """gnn_gather_program_compact (host code): (words [batches, 64] uint32, roww [tiles, 32] float32) of a program built by gather_program -
    its source words and one weight per tile-local row; NotImplementedError when a row's entries differ in their weights' bits."""
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    ent = np.ascontiguousarray(ent).view(np.int32)
    words, roww = np.zeros(ent.shape[:2], np.int32), np.zeros((hdr.shape[0], 32), np.float32)
    _check(lib().gnn_gather_program_compact(C.c_int64(hdr.shape[0]), _ip(hdr), C.c_int64(ent.shape[0]), _ip(ent), _ip(words), _fp(roww)))
    return words.view(np.uint32), roww


def tile_schedule(cost, waves: int, kind: int):
    """gnn_tile_schedule_build (host code): order [slots] int32, order[slot] = the tile that ticket `slot` of a launch of `waves` waves
    stands for; cost[t] = real entries (arcs) of tile t; kind 0 the identity, 1 the balanced order."""
    cost = np.ascontiguousarray(cost, dtype=np.int64)
    order = np.full(cost.size, -1, np.int32)
    _check(lib().gnn_tile_schedule_build(C.c_int64(cost.size), cost.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(int(waves)), C.c_int(int(kind)),
                                         _ip(order)))
    return order


def halo_plan(n_nodes: int, world: int, indptr, adj_src):
    """gnn_halo_plan: (slot [n_nodes] int32, counts [world], block) of the boundary exchange for a whole CSR-by-destination graph."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    adj_src = np.ascontiguousarray(adj_src, dtype=np.int32)
    slot = np.empty(n_nodes, np.int32)
    counts = np.zeros(world, np.int64)
    block = C.c_int64(0)
    _check(lib().gnn_halo_plan(C.c_int64(n_nodes), C.c_int(world), _ip(indptr), _ip(adj_src), _ip(slot),
                               counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(block)))
    return slot, counts, int(block.value)


def shard_halo(n_nodes: int, rank: int, world: int, indptr, adj_src, nodes, plan=None):
    """Arguments of Graph.halo for one rank: sources renumbered into the compact index space
    [own rows | block of boundary rows per rank] and the node labels in the same space."""
    slot, counts, block = plan if plan is not None else halo_plan(n_nodes, world, indptr, adj_src)
    rb, nr = shard_range(n_nodes, rank, world)
    shard = ((n_nodes + world - 1) // world + 31) // 32 * 32
    indptr = np.asarray(indptr)
    e0, e1 = int(indptr[rb]), int(indptr[rb + nr])
    src = np.asarray(adj_src)[e0:e1].astype(np.int64)
    owner = src // shard
    mine = owner == rank
    if np.any(~mine & (slot[src] < 0)):
        raise ValueError('halo plan does not cover a remote source')
    remapped = np.where(mine, src - rb, shard + owner * block + slot[src]).astype(np.int32)
    nodes = np.asarray(nodes, np.float32)
    rep = np.zeros((shard + world * block, nodes.shape[1]), np.float32)
    rep[:nr] = nodes[rb:rb + nr]
    for q in range(world):
        qb, qn = shard_range(n_nodes, q, world)
        ids = qb + np.nonzero(slot[qb:qb + qn] >= 0)[0]
        rep[shard + q * block: shard + q * block + len(ids)] = nodes[ids]
    send = np.nonzero(slot[rb:rb + nr] >= 0)[0].astype(np.int32)
    return dict(block=block, send_rows=send, adj_src=remapped, nodes=rep, row_begin=rb, n_rows=nr, e0=e0, e1=e1)


def shard_csr(n_nodes: int, rank: int, world: int, indptr, *per_entry_arrays):
    """Node-range shard of a CSR-by-destination graph: (row_begin, n_rows, local indptr, sliced per-entry arrays...).
    Source ids inside the slices stay GLOBAL (every rank keeps a full replica of the state)."""
    rb, nr = shard_range(n_nodes, rank, world)
    indptr = np.asarray(indptr)
    e0, e1 = int(indptr[rb]), int(indptr[rb + nr])
    return (rb, nr, (indptr[rb:rb + nr + 1] - e0).astype(np.int32)) + tuple(np.asarray(a)[e0:e1] for a in per_entry_arrays)


class Graph:
    """Device-resident graph (gnn_graph).  CSR "by destination" as produced by graph_class.GraphTensor."""

    def __init__(self, n_nodes, indptr, adj_src, adj_w, arc_w, arc_labels, nodes, mask, row_begin=0, device=0, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        require_device(device)
        indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        adj_src = np.ascontiguousarray(adj_src, dtype=np.int32)
        adj_w, arc_w = _f32(adj_w), _f32(arc_w)
        arc_labels, nodes = _f32(arc_labels), _f32(nodes)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        n_rows, n_arcs = len(indptr) - 1, len(adj_src)
        if arc_labels.ndim != 2 or arc_labels.shape[0] != n_arcs or nodes.ndim != 2 or nodes.shape[0] != n_nodes:
            raise ValueError('arc_labels must be [n_arcs, AL] and nodes [n_nodes, NL]')
        if len(adj_w) != n_arcs or len(arc_w) != n_arcs or len(mask) != n_rows:
            raise ValueError('inconsistent array lengths')
        _check(lib().gnn_graph_create(C.c_int64(n_nodes), C.c_int64(row_begin), C.c_int64(n_rows), C.c_int64(n_arcs),
                                      _ip(indptr), _ip(adj_src), _fp(adj_w), _fp(arc_w), _fp(arc_labels),
                                      C.c_int(arc_labels.shape[1]), _fp(nodes), C.c_int(nodes.shape[1]),
                                      mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(device), C.byref(self._h)))

    @classmethod
    def halo(cls, n_nodes_global, rank, world, block, send_rows, indptr, adj_src_replica, adj_w, arc_w, arc_labels, nodes_replica, mask, device=0):
        """gnn_graph_create_halo: shard whose per-iteration exchange moves only boundary rows (see shard_halo)."""
        require_device(device)
        indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        adj = np.ascontiguousarray(adj_src_replica, dtype=np.int32)
        send = np.ascontiguousarray(send_rows, dtype=np.int32)
        adj_w, arc_w, arc_labels, nodes_replica = _f32(adj_w), _f32(arc_w), _f32(arc_labels), _f32(nodes_replica)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if len(adj_w) != len(adj) or len(arc_w) != len(adj) or arc_labels.shape[0] != len(adj) or len(mask) != len(indptr) - 1:
            raise ValueError('inconsistent array lengths')
        h = C.c_void_p()
        _check(lib().gnn_graph_create_halo(C.c_int64(n_nodes_global), C.c_int(rank), C.c_int(world), C.c_int64(block), C.c_int64(len(send)), _ip(send),
                                           C.c_int64(len(adj)), _ip(indptr), _ip(adj), _fp(adj_w), _fp(arc_w), _fp(arc_labels), C.c_int(arc_labels.shape[1]),
                                           _fp(nodes_replica), C.c_int(nodes_replica.shape[1]), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(device), C.byref(h)))
        return cls(None, None, None, None, None, None, None, None, _handle=h)

    @classmethod
    def from_arcs(cls, n_nodes, arc_src, arc_dst, arc_labels, aggregation_mode, nodes, mask, device=0):
        """gnn_graph_create_from_arcs: device-side COO -> CSR build.  Returns (Graph, indptr, adj_src, adj_w, arc_id, arc_w):
        the handle and the host mirrors of Adjacency^T / ArcNode^T."""
        require_device(device)
        modes = {'sum': 0, 'normalized': 1, 'average': 2}
        if aggregation_mode not in modes: raise ValueError('ERROR: Unknown aggregation mode')
        arc_src = np.ascontiguousarray(arc_src, dtype=np.int32)
        arc_dst = np.ascontiguousarray(arc_dst, dtype=np.int32)
        arc_labels, nodes = _f32(arc_labels), _f32(nodes)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        e = len(arc_src)
        if len(arc_dst) != e or arc_labels.shape[0] != e or nodes.shape[0] != n_nodes or len(mask) != n_nodes:
            raise ValueError('inconsistent array lengths')
        indptr, adj_src, arc_id = np.zeros(n_nodes + 1, np.int32), np.zeros(e, np.int32), np.zeros(e, np.int32)
        adj_w, arc_w = np.zeros(e, np.float32), np.zeros(e, np.float32)
        h = C.c_void_p()
        _check(lib().gnn_graph_create_from_arcs(C.c_int64(n_nodes), C.c_int64(e), _ip(arc_src), _ip(arc_dst), _fp(arc_labels),
                                                C.c_int(arc_labels.shape[1]), C.c_int(modes[aggregation_mode]), _fp(nodes), C.c_int(nodes.shape[1]),
                                                mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(device), C.byref(h), _ip(indptr), _ip(adj_src),
                                                _fp(adj_w), _ip(arc_id), _fp(arc_w)))
        return cls(None, None, None, None, None, None, None, None, _handle=h), indptr, adj_src, adj_w, arc_id, arc_w

    def dims(self):
        n, r, e, m = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        nl, al = C.c_int(), C.c_int()
        _check(lib().gnn_graph_dims(self._h, C.byref(n), C.byref(r), C.byref(e), C.byref(nl), C.byref(al), C.byref(m)))
        return dict(n_nodes=n.value, n_rows=r.value, n_arcs=e.value, NL=nl.value, AL=al.value, n_masked=m.value)

    def derive(self, extra: int) -> 'Graph':
        h = C.c_void_p()
        _check(lib().gnn_graph_derive(self._h, C.c_int(extra), C.byref(h)))
        d = Graph(None, None, None, None, None, None, None, None, _handle=h)
        d._base = self            # a derived graph uses arrays of its base (CSR, boundary rows): keep it alive
        return d

    def derive_edge(self, extra_nodes: int, extra_arcs: int) -> 'Graph':
        h = C.c_void_p()
        _check(lib().gnn_graph_derive_edge(self._h, C.c_int(extra_nodes), C.c_int(extra_arcs), C.byref(h)))
        d = Graph(None, None, None, None, None, None, None, None, _handle=h)
        d._base = self
        return d

    def gather_program_info(self) -> dict:
        """gnn_graph_gather_program_info: size and host build time of the graph's gather program (all zero while it has none)."""
        t, b, n, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        _check(lib().gnn_graph_gather_program_info(self._h, C.byref(t), C.byref(b), C.byref(n), C.byref(ms)))
        return dict(tiles=t.value, batches=b.value, bytes=n.value, build_ms=ms.value)

    def gather_program_format(self) -> int:
        """gnn_graph_gather_program_format: entry format of the program on the device - 0 none (yet), 8, or 4 (source words + one weight per row)."""
        n = C.c_int(0)
        _check(lib().gnn_graph_gather_program_format(self._h, C.byref(n)))
        return n.value

    def set_program_entries(self, entries: int) -> int:
        """gnn_graph_set_program_entries (A/B runs, tests): 0 the library's choice, 8 or 4; drops the program and its schedules and returns
        the format held from now on (8 where 4 is not available, 0 without a program)."""
        used = C.c_int(0)
        _check(lib().gnn_graph_set_program_entries(self._h, C.c_int(int(entries)), C.byref(used)))
        return used.value

    def tile_schedule_info(self) -> dict:
        """gnn_graph_tile_schedule_info: slots of the program kernel's tile schedule, the kind built so far (0 none, 1 ascending only, 2 the
        balanced order too), body and tail sizes of the balanced order and its host build time."""
        s, k, b, t, ms = C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        _check(lib().gnn_graph_tile_schedule_info(self._h, C.byref(s), C.byref(k), C.byref(b), C.byref(t), C.byref(ms)))
        return dict(slots=s.value, kind=k.value, body=b.value, tail=t.value, build_ms=ms.value)

    def set_arc_order(self, arc_id, arc_labels_orig) -> None:
        arc_id = np.ascontiguousarray(arc_id, dtype=np.int32)
        _check(lib().gnn_graph_set_arc_order(self._h, _ip(arc_id), _fp(_f32(arc_labels_orig))))

    def update_labels(self, base: 'Graph', loop: 'Loop', get_state: bool, get_output: bool) -> None:
        _check(lib().gnn_graph_update_labels(self._h, base._h, loop._h, C.c_int(bool(get_state)), C.c_int(bool(get_output))))

    def set_full_adjacency(self, n_global: int, indptr, adj_src, adj_w):
        """gnn_graph_set_full_adjacency: the whole graph's CSR by destination (global ids) for the feature-sliced exchange."""
        ip, src, w = np.ascontiguousarray(indptr, np.int32), np.ascontiguousarray(adj_src, np.int32), _f32(adj_w)
        _check(lib().gnn_graph_set_full_adjacency(self._h, C.c_int64(n_global), _ip(ip), _ip(src), _fp(w)))

    @staticmethod
    def update_labels_group(dsts, bases, loops, get_state: bool, get_output: bool) -> None:
        """gnn_graph_update_labels_group: the relabelling step for all ranks of a loopback group."""
        n = len(loops)
        arr = lambda xs: (C.c_void_p * n)(*[x._h for x in xs])
        _check(lib().gnn_graph_update_labels_group(arr(dsts), arr(bases), arr(loops), C.c_int(n), C.c_int(bool(get_state)), C.c_int(bool(get_output))))

    def nodes(self) -> np.ndarray:
        d = self.dims()
        out = np.empty((d['n_nodes'], d['NL']), dtype=np.float32)
        _check(lib().gnn_graph_get_nodes(self._h, _fp(out)))
        return out

    def close(self):
        if self._h:
            lib().gnn_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mlp:
    """Device-resident Sequential (gnn_mlp): Keras get_weights() list + activation names."""

    def __init__(self, weights, activations, batch_normalization, bn_eps=1e-3, device=0):
        require_device(device)
        self._h = C.c_void_p()
        self.n = len(activations)
        self.activations = list(activations)
        self.batch_normalization = bool(batch_normalization)
        for a in activations:
            if a not in ACT_CODES:
                raise ValueError(f'unsupported activation {a!r}')
        w, b, bn = self._pack(weights)
        self.dims = np.array([w[0].shape[0]] + [x.shape[1] for x in w], dtype=np.int32)
        acts = np.array([ACT_CODES[a] for a in activations], dtype=np.int32)
        wp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in w])
        bp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in b])
        _check(lib().gnn_mlp_create(C.c_int(self.n), _ip(self.dims), _ip(acts), wp, bp, _fp(bn), C.c_float(bn_eps),
                                    C.c_int(device), C.byref(self._h)))

    def _pack(self, weights):
        n = self.n
        if len(weights) != 2 * n + (4 if self.batch_normalization else 0):
            raise ValueError(f'expected {2 * n + (4 if self.batch_normalization else 0)} weight arrays, got {len(weights)}')
        w = [_f32(weights[2 * l]) for l in range(n)]
        b = [_f32(weights[2 * l + 1]) for l in range(n)]
        for l in range(n):
            if w[l].ndim != 2 or b[l].shape != (w[l].shape[1],) or (l and w[l].shape[0] != w[l - 1].shape[1]):
                raise ValueError(f'layer {l}: inconsistent weight shapes')
        bn = None
        if self.batch_normalization:
            bn = np.ascontiguousarray(np.concatenate([_f32(a).ravel() for a in weights[2 * n:]]))
            if bn.size != 4 * w[-1].shape[1]:
                raise ValueError('BatchNormalization arrays must each have the output width')
        return w, b, bn

    def set_weights(self, weights):
        w, b, bn = self._pack(weights)
        if [x.shape for x in w] != [(int(self.dims[l]), int(self.dims[l + 1])) for l in range(self.n)]:
            raise ValueError('weight shapes differ from the ones this MLP was created with')
        wp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in w])
        bp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in b])
        _check(lib().gnn_mlp_set_weights(self._h, wp, bp, _fp(bn)))

    def get_weights(self):
        """gnn_mlp_get_weights: the Keras get_weights() list as it is on the device now."""
        w = [np.empty((int(self.dims[l]), int(self.dims[l + 1])), np.float32) for l in range(self.n)]
        b = [np.empty((int(self.dims[l + 1]),), np.float32) for l in range(self.n)]
        f = int(self.dims[-1])
        bn = np.empty(4 * f, np.float32) if self.batch_normalization else None
        wp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in w])
        bp = (C.POINTER(C.c_float) * self.n)(*[_fp(x) for x in b])
        _check(lib().gnn_mlp_get_weights(self._h, wp, bp, _fp(bn)))
        out = []
        for l in range(self.n):
            out += [w[l], b[l]]
        if bn is not None:
            out += [bn[i * f:(i + 1) * f].copy() for i in range(4)]
        return out

    def reset_optimizer(self):
        """gnn_mlp_reset_optimizer: zero optimizer slots for the next device-side step (a new optimizer object took over)."""
        _check(lib().gnn_mlp_reset_optimizer(self._h))

    def set_regularizers(self, coefficients):
        """gnn_mlp_set_regularizers: ([l1 per array], [l2 per array]) in [W1, b1, W2, b2, ...] order (GNN.regularizers.device_coefficients);
        None clears them.  Remembered here, so that the call per training step costs nothing while they stay the same."""
        key = None if coefficients is None else (tuple(coefficients[0]), tuple(coefficients[1]))
        if key is not None and not any(key[0]) and not any(key[1]): key = None
        if key == getattr(self, '_reg_set', None):
            return
        if key is None:
            _check(lib().gnn_mlp_set_regularizers(self._h, None, None))
        else:
            if len(key[0]) != 2 * self.n or len(key[1]) != 2 * self.n: raise ValueError(f'expected {2 * self.n} coefficients per list')
            _check(lib().gnn_mlp_set_regularizers(self._h, (C.c_double * (2 * self.n))(*key[0]), (C.c_double * (2 * self.n))(*key[1])))
        self._reg_set = key

    def forward(self, x):
        x = _f32(x)
        if x.ndim != 2 or x.shape[1] != self.dims[0]:
            raise ValueError(f'expected [n, {self.dims[0]}] input')
        y = np.empty((x.shape[0], int(self.dims[-1])), dtype=np.float32)
        _check(lib().gnn_mlp_forward(self._h, C.c_int64(x.shape[0]), _fp(x), _fp(y)))
        return y

    def close(self):
        if self._h:
            lib().gnn_mlp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator (one process per GPU), or one member of an in-process loopback group (Comm.loopback)."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int, _handle=None):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        if _handle is not None:
            self._h = _handle
            return
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(lib().gnn_comm_create(buf, C.c_int(rank), C.c_int(world), C.c_int(device), C.byref(self._h)))

    @classmethod
    def loopback(cls, world: int, device: int = 0) -> list:
        """gnn_comm_create_loopback: `world` communicators on ONE device (the sharded path on a single GPU; tests only)."""
        require_device(device)
        hs = (C.c_void_p * world)()
        _check(lib().gnn_comm_create_loopback(C.c_int(world), C.c_int(device), hs))
        return [cls(None, r, world, device, _handle=C.c_void_p(hs[r])) for r in range(world)]

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(lib().gnn_comm_unique_id(buf))
        return bytes(buf)

    def allreduce_max(self, value: float) -> float:
        v = C.c_double(value)
        _check(lib().gnn_comm_allreduce_max(self._h, C.byref(v)))
        return v.value

    def close(self):
        if self._h:
            lib().gnn_comm_destroy(self._h)
            self._h = C.c_void_p()


class Loop:
    """One configured GNN.Loop on the device (gnn_loop)."""

    def __init__(self, graph: Graph, net_state: Mlp, net_output: Mlp, state_dim: int, max_iter: int, threshold: float,
                 comm: Comm | None = None):
        self._h = C.c_void_p()
        self._keep = (graph, net_state, net_output, comm)
        self.graph = graph
        d = graph.dims()
        self.n_rows, self.n_masked = d['n_rows'], d['n_masked']
        self.Ds = state_dim if state_dim else d['NL']
        self.T = int(net_output.dims[-1])
        self.state_dim = state_dim
        self.max_iter = int(max_iter)
        _check(lib().gnn_loop_create(graph._h, net_state._h, net_output._h, C.c_int(state_dim), C.c_int(max_iter),
                                     C.c_float(threshold), comm._h if comm else None, C.byref(self._h)))

    def set_state0(self, state0=None, seed: int = 0):
        if state0 is not None:
            state0 = _f32(state0, (self.n_rows, self.Ds))
        _check(lib().gnn_loop_set_state0(self._h, _fp(state0), C.c_uint64(seed)))

    def set_edge_readout(self, entry_dst, arc_labels, arc_mask):
        """Switch to the per-arc readout of GNNedgeBased (reference GNN.py:289-302)."""
        entry_dst = np.ascontiguousarray(entry_dst, dtype=np.int32)
        arc_labels = _f32(arc_labels) if arc_labels is not None else None      # None: the (derived) graph owns its arc labels
        arc_mask = np.ascontiguousarray(arc_mask, dtype=np.uint8)
        if not (len(entry_dst) == len(arc_mask)) or (arc_labels is not None and arc_labels.shape[0] != len(arc_mask)):
            raise ValueError('entry_dst, arc_labels and arc_mask must have one row per arc')
        _check(lib().gnn_loop_set_edge_readout(self._h, _ip(entry_dst), _fp(arc_labels) if arc_labels is not None else None,
                                               arc_mask.ctypes.data_as(C.POINTER(C.c_uint8))))
        self.n_masked = int(arc_mask.sum())

    def train_step(self, net_state: 'Mlp', net_output: 'Mlp', src_csr, targets, sample_weights, loss_kind: int, ng_csr=None,
                   dropout_state=None, dropout_output=None, masks_state=None, masks_output=None, seed: int = 0,
                   bn_state=None, bn_output=None):
        """gnn_loop_train_step: loss, iteration count, raw gradients (lists shaped like the trainable arrays) and the
        BatchNormalization batch statistics of every call."""
        sip, sdst, sw = (np.ascontiguousarray(src_csr[0], np.int32), np.ascontiguousarray(src_csr[1], np.int32), _f32(src_csr[2])) if src_csr is not None else (None, None, None)
        targets, sample_weights = _f32(targets), _f32(sample_weights)
        ls, lo = net_state.n, net_output.n
        ds_ = _f32(dropout_state if dropout_state is not None else np.zeros(ls + 1))
        do_ = _f32(dropout_output if dropout_output is not None else np.zeros(lo + 1))

        def shapes(net):
            out = []
            for l in range(net.n):
                out += [(int(net.dims[l]), int(net.dims[l + 1])), (int(net.dims[l + 1]),)]
            if net.batch_normalization:
                out += [(int(net.dims[-1]),), (int(net.dims[-1]),)]
            return out

        shp_s, shp_o = shapes(net_state), shapes(net_output)
        gs = np.zeros(sum(int(np.prod(x)) for x in shp_s), np.float32)
        go = np.zeros(sum(int(np.prod(x)) for x in shp_o), np.float32)
        fs, fo = int(net_state.dims[-1]), int(net_output.dims[-1])
        bns = np.zeros((max(1, self.max_iter), 2, fs), np.float32)      # the C side writes k <= max_iteration rows
        bno = np.zeros((2, fo), np.float32)
        ms = np.ascontiguousarray(masks_state, np.uint8) if masks_state is not None else None
        mo = np.ascontiguousarray(masks_output, np.uint8) if masks_output is not None else None
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None
        if ng_csr is not None:
            ngi, ngn, ngw = np.ascontiguousarray(ng_csr[0], np.int32), np.ascontiguousarray(ng_csr[1], np.int32), _f32(ng_csr[2])
            n_graphs = len(ngi) - 1
        else:
            ngi = ngn = ngw = None
            n_graphs = 0
        bs = _f32(bn_state) if bn_state is not None else None
        bo = _f32(bn_output) if bn_output is not None else None
        loss, k = C.c_float(), C.c_float()
        _check(lib().gnn_loop_train_step(self._h, _ip(sip), _ip(sdst), _fp(sw), _fp(targets), _fp(sample_weights),
                                         C.c_int64(targets.shape[0]), C.c_int(loss_kind), C.c_int(n_graphs), _ip(ngi), _ip(ngn), _fp(ngw),
                                         _fp(ds_), _fp(do_), u8(ms), u8(mo), C.c_uint64(seed), _fp(bs), _fp(bo), C.byref(loss), C.byref(k),
                                         _fp(gs), _fp(go), _fp(bns), _fp(bno)))

        def split(flat, shp):
            out, off = [], 0
            for x in shp:
                cnt = int(np.prod(x))
                out.append(flat[off:off + cnt].reshape(x).copy())
                off += cnt
            return out

        kk = int(k.value)
        # (fixed-point modes: the k bodies were the inference Loop's - net_state has no batch statistics, bn_batch_state is left unwritten)
        if getattr(self, '_gradient_mode', 0) != 0: kk = 0
        res = dict(loss=float(loss.value), k=float(k.value), grads_state=split(gs, shp_s), grads_output=split(go, shp_o),
                   bn_batch_state=bns[:kk], bn_batch_output=bno)
        if getattr(self, '_gradient_mode', 0) != 0:
            info = self.adjoint_info()
            res.update(adjoint_iterations=info['iterations'], adjoint_converged=info['converged'])
        return res

    def set_slice_exchange(self, on=True, form=None):
        """gnn_loop_set_slice_exchange: feature-sliced all-to-all instead of the all-gather of state rows.  on: any truthy value (True, 1,
        numpy.bool_) switches it on in the default form, falsy switches it off.  form (keyword, only with on): 'oneshot' (default: whole slice,
        then one grouped all-to-all) or 'pipelined' (the return all-to-all block by block beside the aggregation on a second stream of the
        communicator - bit-identical in loopback groups and over the tests' stand-in transport, but never yet run over RCCL with more than
        one rank, hence never implied by `on`)."""
        if form not in (None, 'oneshot', 'pipelined'):
            raise ValueError("form must be 'oneshot' or 'pipelined'")
        code = 0 if not on else (1 if form == 'pipelined' else 2)
        _check(lib().gnn_loop_set_slice_exchange(self._h, C.c_int(code)))

    def update_moving_statistics(self, bn_momentum_state: float = 0.99, bn_momentum_output: float = 0.99):
        """gnn_loop_update_moving_statistics: the moving statistics of both nets from the last train_forward, on the device."""
        _check(lib().gnn_loop_update_moving_statistics(self._h, C.c_float(bn_momentum_state), C.c_float(bn_momentum_output)))

    def arm_optimizer(self, kind: int, hyper, mean: bool, bn_momentum_state: float = 0.99, bn_momentum_output: float = 0.99):
        """gnn_loop_arm_optimizer: the next train_step() also applies the optimizer update on the device."""
        h = _f32(np.asarray(list(hyper) + [0.0] * (4 - len(hyper)), np.float32))
        _check(lib().gnn_loop_arm_optimizer(self._h, C.c_int(kind), _fp(h), C.c_int(1 if mean else 0), C.c_float(bn_momentum_state),
                                            C.c_float(bn_momentum_output)))

    def optimizer_step(self, kind: int, hyper, state_grad_scale: float = 1.0, bn_momentum_state: float = 0.99, bn_momentum_output: float = 0.99):
        """gnn_loop_optimizer_step: apply the gradients of the last backward pass on the device."""
        h = _f32(np.asarray(list(hyper) + [0.0] * (4 - len(hyper)), np.float32))
        _check(lib().gnn_loop_optimizer_step(self._h, C.c_int(kind), _fp(h), C.c_float(state_grad_scale), C.c_float(bn_momentum_state),
                                             C.c_float(bn_momentum_output)))

    def set_clipping(self, clipvalue: float = 0.0, clipnorm: float = 0.0, global_clipnorm: float = 0.0):
        """gnn_loop_set_clipping (0 = off): holds for every later armed train_step() / optimizer_step() of this loop."""
        key = (float(clipvalue), float(clipnorm), float(global_clipnorm))
        if key != getattr(self, '_clip_set', (0.0, 0.0, 0.0)):
            _check(lib().gnn_loop_set_clipping(self._h, C.c_double(key[0]), C.c_double(key[1]), C.c_double(key[2])))
            self._clip_set = key

    def set_loss_params(self, label_smoothing: float = 0.0, huber_delta: float = 1.0):
        """gnn_loop_set_loss_params: label smoothing and Huber delta of the loss inside every later train_step() of this loop."""
        key = (float(label_smoothing), float(huber_delta))
        if key != getattr(self, '_loss_params_set', (0.0, 1.0)):
            _check(lib().gnn_loop_set_loss_params(self._h, C.c_double(key[0]), C.c_double(key[1])))
            self._loss_params_set = key

    def grad_sqnorm(self, state_grad_scale: float = 1.0):
        """gnn_loop_grad_sqnorm: (sum of squares of this loop's scaled and value-clipped gradients, regularizer penalty of both nets)."""
        sq, pen = C.c_double(), C.c_double()
        _check(lib().gnn_loop_grad_sqnorm(self._h, C.c_float(state_grad_scale), C.byref(sq), C.byref(pen)))
        return sq.value, pen.value

    def optimizer_step_scaled(self, kind: int, hyper, state_grad_scale: float, grad_scale: float, bn_momentum_state: float = 0.99,
                              bn_momentum_output: float = 0.99):
        """gnn_loop_optimizer_step_scaled: optimizer_step() with the factor of a global norm that spans several loops."""
        h = _f32(np.asarray(list(hyper) + [0.0] * (4 - len(hyper)), np.float32))
        _check(lib().gnn_loop_optimizer_step_scaled(self._h, C.c_int(kind), _fp(h), C.c_float(state_grad_scale), C.c_double(grad_scale),
                                                    C.c_float(bn_momentum_state), C.c_float(bn_momentum_output)))

    @staticmethod
    def _grad_shapes(net: 'Mlp'):
        out = []
        for l in range(net.n):
            out += [(int(net.dims[l]), int(net.dims[l + 1])), (int(net.dims[l + 1]),)]
        if net.batch_normalization:
            out += [(int(net.dims[-1]),), (int(net.dims[-1]),)]
        return out

    def train_forward(self, net_state: 'Mlp', net_output: 'Mlp', src_csr, dropout_state=None, dropout_output=None,
                      masks_state=None, masks_output=None, seed: int = 0, bn_state=None, bn_output=None):
        """gnn_loop_train_forward: training-mode Loop; returns (k, node-level outputs [n_masked, T]).  The loop's state() /
        output() / readout() then hold the training-mode results, and train_backward() may be called once."""
        sip, sdst, sw = (np.ascontiguousarray(src_csr[0], np.int32), np.ascontiguousarray(src_csr[1], np.int32), _f32(src_csr[2])) if src_csr is not None else (None, None, None)
        ds_ = _f32(dropout_state if dropout_state is not None else np.zeros(net_state.n + 1))
        do_ = _f32(dropout_output if dropout_output is not None else np.zeros(net_output.n + 1))
        ms = np.ascontiguousarray(masks_state, np.uint8) if masks_state is not None else None
        mo = np.ascontiguousarray(masks_output, np.uint8) if masks_output is not None else None
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None
        bs = _f32(bn_state) if bn_state is not None else None
        bo = _f32(bn_output) if bn_output is not None else None
        k = C.c_float()
        out = np.zeros((self.n_masked, self.T), np.float32)
        _check(lib().gnn_loop_train_forward(self._h, _ip(sip), _ip(sdst), _fp(sw), _fp(ds_), _fp(do_), u8(ms), u8(mo), C.c_uint64(seed),
                                            _fp(bs), _fp(bo), C.byref(k), _fp(out)))
        self._train_nets = (net_state, net_output, int(k.value))
        return float(k.value), out

    def _backward_buffers(self, d_out_nodes):
        """What both backward calls share: (d_out [n_masked, T], flat gradient buffers of both nets, batch-statistics buffers, `finish`), where
        finish(d_nodes, d_arcs) splits the filled buffers into the result dict."""
        net_state, net_output, kk = self._train_nets
        if getattr(self, '_gradient_mode', 0) != 0: kk = 0       # (fixed-point modes: no batch statistics of net_state, as in train_step)
        shp_s, shp_o = self._grad_shapes(net_state), self._grad_shapes(net_output)
        gs = np.zeros(sum(int(np.prod(x)) for x in shp_s), np.float32)
        go = np.zeros(sum(int(np.prod(x)) for x in shp_o), np.float32)
        bns = np.zeros((max(1, kk), 2, int(net_state.dims[-1])), np.float32)
        bno = np.zeros((2, int(net_output.dims[-1])), np.float32)
        d_out = _f32(d_out_nodes)
        if d_out.shape != (self.n_masked, self.T): raise ValueError(f'd_out_nodes shape {d_out.shape} != {(self.n_masked, self.T)}')

        def split(flat, shp):
            out, off = [], 0
            for x in shp:
                cnt = int(np.prod(x))
                out.append(flat[off:off + cnt].reshape(x).copy())
                off += cnt
            return out

        def finish(dn, da):
            return dict(grads_state=split(gs, shp_s), grads_output=split(go, shp_o), bn_batch_state=bns[:kk], bn_batch_output=bno, d_nodes=dn, d_arcs=da)

        return d_out, gs, go, bns, bno, finish

    def train_backward(self, d_out_nodes, d_state_extra=None, want_d_nodes: bool = False, want_d_arcs: bool = False):
        """gnn_loop_train_backward: dict(grads_state, grads_output (raw sums over the iterations), bn_batch_state,
        bn_batch_output, d_nodes [N, NL] or None)."""
        d_out, gs, go, bns, bno, finish = self._backward_buffers(d_out_nodes)
        dse = None
        if d_state_extra is not None:
            dse = _f32(d_state_extra)
            if dse.shape != (self.n_rows, self.Ds): raise ValueError(f'd_state_extra shape {dse.shape} != {(self.n_rows, self.Ds)}')
        dims = self.graph.dims()
        dn = np.zeros((self.n_rows, dims['NL']), np.float32) if want_d_nodes else None
        da = np.zeros((dims['n_arcs'], dims['AL']), np.float32) if want_d_arcs else None
        _check(lib().gnn_loop_train_backward(self._h, _fp(d_out), _fp(dse), _fp(gs), _fp(go), _fp(bns), _fp(bno), _fp(dn), _fp(da)))
        return finish(dn, da)

    def train_backward_chained(self, d_out_nodes, next_loop=None, get_state: bool = False, get_output: bool = False, keep_label_gradients=False):
        """gnn_loop_train_backward_chained: train_backward() for a stack whose label gradients stay on the device.  keep_label_gradients: what is
        computed and stays in this loop's training scratch until its next train_forward() - KEEP_D_NODES, KEEP_D_ARC_LABELS (edge-based loops),
        their sum, or True for both; name what the layer below will read.  next_loop: the loop of the layer above, whose last backward pass kept
        them - its columns with this loop's state (get_state) take the place of d_state_extra, its masked rows with this loop's outputs
        (get_output) are added to d_out_nodes.  Bit-identical to chaining two train_backward() calls through host arrays.  Returns the dict of
        train_backward() with d_nodes = d_arcs = None."""
        keep = (KEEP_D_NODES | KEEP_D_ARC_LABELS) if keep_label_gradients is True else int(keep_label_gradients)
        d_out, gs, go, bns, bno, finish = self._backward_buffers(d_out_nodes)
        _check(lib().gnn_loop_train_backward_chained(self._h, _fp(d_out), next_loop._h if next_loop is not None else None, C.c_int(bool(get_state)),
                                                     C.c_int(bool(get_output)), _fp(gs), _fp(go), _fp(bns), _fp(bno), C.c_int(keep)))
        return finish(None, None)

    def train_forms(self, net: int = 0) -> dict:
        """gnn_loop_train_forms: what the last train_forward() / train_step() decided for net_state (0) or net_output (1), as train_forms()."""
        out = np.zeros(3 + 3 * self._keep[1 + net].n, np.int32)
        _check(lib().gnn_loop_train_forms(self._h, C.c_int(net), _ip(out)))
        return _forms_dict(out)

    def train_mask(self, net: int, body: int, pos: int) -> np.ndarray:
        """gnn_loop_train_mask (introspection for tests): the keep mask [rows, width] (bool) that the last train_forward() / train_step()
        applied at Dropout position pos of net_state (net 0, body < k) or net_output (net 1) - injected or drawn."""
        count = C.c_int64()
        _check(lib().gnn_loop_train_mask(self._h, C.c_int(net), C.c_int(body), C.c_int(pos), None, C.byref(count)))
        width = int(self._keep[1 + net].dims[pos])
        out = np.zeros(count.value, np.uint8)
        _check(lib().gnn_loop_train_mask(self._h, C.c_int(net), C.c_int(body), C.c_int(pos), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(count)))
        return out.reshape(-1, width).astype(bool)

    def set_impl(self, impl: int) -> int:
        used = C.c_int(0)
        _check(lib().gnn_loop_set_impl(self._h, C.c_int(impl), C.byref(used)))
        return used.value

    def gate_info(self) -> tuple:
        """gnn_loop_gate_info: (the last run was repeated on the bit-exact path because a gate of the default path was not certified, how
        often that has happened on this loop)."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().gnn_loop_gate_info(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), int(b.value)

    def set_pieces(self, pieces: int) -> int:
        """gnn_loop_set_pieces: piece format of impl 2 - 2 = two fp16 pieces per operand (default), 3 = three bf16 pieces.  For A/B runs and
        tests, not a user-facing mode."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_pieces(self._h, C.c_int(int(pieces)), C.byref(used)))
        return used.value

    def range_info(self) -> tuple:
        """gnn_loop_range_info: (the last run was repeated with bf16 pieces because an activation left the fp16 range, how often that has
        happened on this loop)."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().gnn_loop_range_info(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), int(b.value)

    def set_persistent(self, enable: bool) -> bool:
        """gnn_loop_set_persistent: allow / forbid the one-launch-per-Loop path of small graphs; returns whether it will be used."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_persistent(self._h, C.c_int(bool(enable)), C.byref(used)))
        return bool(used.value)

    def set_train_persistent(self, enable: bool) -> bool:
        """gnn_loop_set_train_persistent: allow / forbid the persistent training forward of small batches (all bodies of net_state in one
        launch, bit-identical to one launch per kernel and body); returns whether a training forward without Dropout in net_state would
        take it on this loop now.  What the last forward actually took: train_info()."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_train_persistent(self._h, C.c_int(bool(enable)), C.byref(used)))
        return bool(used.value)

    def set_train_recompute(self, enable, cacheless: bool = True) -> bool:
        """gnn_loop_set_train_recompute: recomputation of the bodies' activations in the unrolled training step (off by default).  The forward
        keeps each body's output state, statistics and gate alone; the backward pass rebuilds a body's cache right before it walks the body.
        Every result equals the default step's bit for bit.  cacheless=False: the first pass runs the ordinary kernels on scratch instead of
        the cache-less forms (A/B runs).  Returns whether a training forward of this loop would take the mode now (False in the fixed-point
        gradient modes); NotImplementedError on a sharded loop."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_train_recompute(self._h, C.c_int((1 if cacheless else 2) if enable else 0), C.byref(used)))
        return bool(used.value)

    def train_recompute_info(self) -> dict:
        """gnn_loop_train_recompute_info: dict(state_only: the last train_forward() / train_step() kept the bodies' states alone; replayed: bodies
        rebuilt by the last backward pass; cacheless_chain: 1 when the first pass launched the cache-less three-layer chain, 0 when the
        ordinary kernels ran on scratch)."""
        out = np.zeros(3, np.int32)
        _check(lib().gnn_loop_train_recompute_info(self._h, _ip(out)))
        return dict(state_only=bool(out[0]), replayed=int(out[1]), cacheless_chain=int(out[2]))

    def set_gradient_mode(self, mode, max_iteration=None, threshold=None, *, batch_normalization=None, label_gradients: bool = False) -> int:
        """gnn_loop_set_gradient_mode: 'unrolled' / 0 (default: back-propagation through the executed bodies) or 'fixed_point' / 1 (the
        gradient at the converged state: inference Loop, one recorded body, adjoint iteration z <- g + J^T z, one weight-gradient pass).
        max_iteration / threshold of the adjoint iteration: None = the loop's own.  In fixed-point mode grads_state is NOT a sum over bodies
        (never divide it by k), train_step() reports adjoint_iterations / adjoint_converged, and net_state must have neither Dropout nor
        BatchNormalization (NotImplementedError).  'fixed_point_chain' / 2: fixed point without the one-launch iteration of narrow nets (A/B runs, tests).
        batch_normalization='frozen' (gnn_loop_set_gradient_mode_ex with GNN_ADJOINT_FROZEN_BN): a net_state that ends in BatchNormalization is
        accepted, on its moving statistics, which the step leaves untouched; gamma and beta train.  None: gnn_loop_set_gradient_mode.
        label_gradients=True (GNN_ADJOINT_LABEL_GRADIENTS): train_backward(want_d_nodes / want_d_arcs) and train_backward_chained(keep_label_gradients=...) work
        in the fixed-point modes - the direct part plus the label columns of the recorded body's d concat for z_final; refused with state_vect_dim 0."""
        code = {'unrolled': 0, 'fixed_point': 1, 'fixed_point_chain': 2, 0: 0, 1: 1, 2: 2}.get(mode)
        if code is None: raise ValueError("gradient mode must be 'unrolled' or 'fixed_point'")
        flags = adjoint_flags(batch_normalization, label_gradients)
        used = C.c_int(0)
        if flags:
            _check(lib().gnn_loop_set_gradient_mode_ex(self._h, C.c_int(code), C.c_int(int(max_iteration) if max_iteration else 0),
                                                       C.c_float(-1.0 if threshold is None else float(threshold)), C.c_int(flags), C.byref(used)))
        else:
            _check(lib().gnn_loop_set_gradient_mode(self._h, C.c_int(code), C.c_int(int(max_iteration) if max_iteration else 0),
                                                    C.c_float(-1.0 if threshold is None else float(threshold)), C.byref(used)))
        self._gradient_mode = used.value
        return used.value

    def adjoint_info(self) -> dict:
        """gnn_loop_adjoint_info: dict(iterations, converged, gather) of the last backward pass in fixed-point mode."""
        it, cv, fm = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().gnn_loop_adjoint_info(self._h, C.byref(it), C.byref(cv), C.byref(fm)))
        return dict(iterations=int(it.value), converged=bool(cv.value), gather=GATHER_NAMES[int(fm.value)])

    def set_adjoint_solver(self, solver='picard', window: int = 5) -> int:
        """gnn_loop_set_adjoint_solver: how the backward pass of the fixed-point modes solves (I - J^T) z = g.  'picard' / 0 (default): the iteration
        z <- g + J^T z; 'anderson' / 1: Anderson mixing over the last ``window`` (1 .. 8) difference pairs - the same gate on the residual, far fewer
        iterations where the spectral radius of J is close to 1, 2 window + 2 more [n_rows, Ds] scratch buffers, other bits than 'picard'."""
        code = SOLVER_CODES.get(solver)
        if code is None: raise ValueError("adjoint solver must be 'picard' or 'anderson'")
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= int(window) <= 8: raise ValueError('window must be an int in [1, 8]')
        used = C.c_int(0)
        _check(lib().gnn_loop_set_adjoint_solver(self._h, C.c_int(code), C.c_int(int(window)), C.byref(used)))
        return used.value

    def adjoint_solver_info(self) -> dict:
        """gnn_loop_adjoint_solver_info: dict(solver, window, restarts) - the solver and window set, the window restarts of the last backward pass."""
        sv, wd, rs = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().gnn_loop_adjoint_solver_info(self._h, C.byref(sv), C.byref(wd), C.byref(rs)))
        return dict(solver=SOLVER_NAMES[int(sv.value)], window=int(wd.value), restarts=int(rs.value))

    def adjoint_z(self) -> np.ndarray:
        """gnn_loop_adjoint_z (test entry point): z_final [n_rows, Ds] of the last backward pass in a fixed-point mode."""
        z = np.zeros((self.n_rows, self.Ds), np.float32)
        _check(lib().gnn_loop_adjoint_z(self._h, _fp(z)))
        return z

    def contraction_estimate(self, net_state: 'Mlp', iterations: int = 32, v0=None, seed: int = 0, src_csr=None, dropout_state=None, bn_state=None) -> dict:
        """gnn_loop_contraction_estimate: power iteration on J^T at the state the inference Loop finds, J = d body / d state of net_state there
        (BatchNormalization on its moving statistics).  growth[t] = |J^T v_t| for the unit vectors v_t the iteration runs through, from v0 [n_rows, Ds]
        or (None) normal draws keyed on ``seed``.  Returns dict(growth (the first ``done`` entries), done (< iterations: the vector became 0 or not
        finite there), k (bodies of the inference Loop), last (growth[done - 1], 0.0 without one), rho = exp(mean(log(growth[done // 2 : done])))
        - the estimate of the spectral radius; 0.0 when a growth entry is 0 -, contractive = rho < 1).  Works in every gradient mode and leaves it;
        ends the life of a pending train_forward()."""
        iterations = int(iterations)
        sip, sdst, sw = (np.ascontiguousarray(src_csr[0], np.int32), np.ascontiguousarray(src_csr[1], np.int32), _f32(src_csr[2])) if src_csr is not None else (None, None, None)
        ds_ = _f32(dropout_state if dropout_state is not None else np.zeros(net_state.n + 1))
        bs = _f32(bn_state) if bn_state is not None else None
        if v0 is not None: v0 = _f32(v0, (self.n_rows, self.Ds))
        growth = np.zeros(max(iterations, 1), np.float32)
        done, k = C.c_int(0), C.c_float(0.0)
        _check(lib().gnn_loop_contraction_estimate(self._h, _ip(sip), _ip(sdst), _fp(sw), _fp(ds_), _fp(bs), C.c_int(iterations), _fp(v0), C.c_uint64(seed),
                                                   _fp(growth), C.byref(done), C.byref(k)))
        return contraction_summary(growth, int(done.value), float(k.value))

    def contraction_vector(self) -> np.ndarray:
        """gnn_loop_contraction_vector (test entry point): the last vector w_done [n_rows, Ds] of the last contraction_estimate()."""
        w = np.zeros((self.n_rows, self.Ds), np.float32)
        _check(lib().gnn_loop_contraction_vector(self._h, _fp(w)))
        return w

    def train_arena_bytes(self) -> int:
        """gnn_loop_train_arena_bytes (test entry point): bytes of device scratch the last training forward / backward of this loop used."""
        b = C.c_int64(0)
        _check(lib().gnn_loop_train_arena_bytes(self._h, C.byref(b)))
        return int(b.value)

    def train_info(self) -> dict:
        """gnn_loop_train_info: dict(persistent: the last train_forward() / train_step() ran its bodies in the persistent launch;
        workgroups, barriers_per_body of that launch (0 otherwise); timeouts: how often a persistent forward of this loop gave up at a
        barrier and was repeated launch by launch)."""
        out = np.zeros(4, np.int32)
        _check(lib().gnn_loop_train_info(self._h, _ip(out)))
        return dict(persistent=bool(out[0]), workgroups=int(out[1]), barriers_per_body=int(out[2]), timeouts=int(out[3]))

    def set_tile_form(self, form: int) -> int:
        """gnn_loop_set_tile_form: 1 = one wave per 32-node tile, 2 = a wave pair per tile, 0 = the library's choice; returns the form the
        next run takes (0: the fused path does not cover this loop)."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_tile_form(self._h, C.c_int(int(form)), C.byref(used)))
        return used.value

    def body_kernel(self) -> int:
        """gnn_loop_body_kernel: the per-body kernel of the next run - 0 = not fused, 1 = k_fused_generic, 2 = k_fused_full, 3 = k_fused_pair."""
        kernel = C.c_int(0)
        _check(lib().gnn_loop_body_kernel(self._h, C.byref(kernel)))
        return kernel.value

    def set_gather_form(self, form: int) -> int:
        """gnn_loop_set_gather_form: how the full-tile kernel finds a tile's neighbour rows - 1 = it walks the CSR, 2 = it reads the graph's
        gather program (built on first demand), 0 = the library's choice; returns the form the next run takes (0: the fused path does not
        cover this loop).  Results are identical bit for bit."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_gather_form(self._h, C.c_int(int(form)), C.byref(used)))
        return used.value

    def set_tile_schedule(self, kind: int) -> int:
        """gnn_loop_set_tile_schedule: the order in which a launch of the program kernel works through its tiles - 1 = ascending, 2 = balanced
        by gather load (built per graph on first demand), 0 = the library's choice; returns the order the next run takes (0: its launches
        read no program).  Results are identical bit for bit."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_tile_schedule(self._h, C.c_int(int(kind)), C.byref(used)))
        return used.value

    def set_label_projection(self, mode) -> bool:
        """gnn_loop_set_label_projection: the fused Loop for wide labels - the label terms of net_state's first layer computed once per
        Loop, every body's first layer over [state | aggregated state] only.  'off' / 0 (default), 'auto' / 1 (where the fused path does
        not cover the net as it stands), 'always' / 2 (wherever applicable).  Returns whether the next run takes the seeded kernels
        (impl 2 with one launch per body only)."""
        used = C.c_int(0)
        _check(lib().gnn_loop_set_label_projection(self._h, C.c_int(label_projection_mode(mode)), C.byref(used)))
        return bool(used.value)

    def set_wide_state(self, mode) -> bool:
        """gnn_loop_set_wide_state: the one-launch-per-body Loop for state widths 68 .. 128 - k_fused_generic on a workgroup of 4 to 7
        waves, as many 32-node tiles as fit its LDS.  mode 'off' | 'auto' (where it was measured faster than one kernel per op) | 'always'
        (wherever it is covered and the eight-wave path is not), or 0 | 1 | 2.  Returns whether the next run takes the form."""
        used = C.c_int()
        _check(lib().gnn_loop_set_wide_state(self._h, C.c_int(wide_state_mode(mode)), C.byref(used)))
        return bool(used.value)

    def body_launch(self) -> tuple:
        """gnn_loop_body_launch (test hook): (waves per workgroup, workgroups) of the launch per body of the last form decision; (0, 0): none."""
        out = np.zeros(2, np.int32)
        _check(lib().gnn_loop_body_launch(self._h, _ip(out)))
        return int(out[0]), int(out[1])

    def set_grid_limit(self, n) -> int:
        """gnn_loop_set_grid_limit (test hook): at most n workgroups per k_fused_generic launch, 0 = the library's choice.  Returns the
        grid of the next run's launch per body."""
        if isinstance(n, bool) or int(n) != n or int(n) < 0: raise ValueError('param <n> must be an integer >= 0')
        used = C.c_int()
        _check(lib().gnn_loop_set_grid_limit(self._h, C.c_int(int(n)), C.byref(used)))
        return int(used.value)

    def set_wide_loader(self, loader) -> bool:
        """gnn_loop_set_wide_loader (test hook): the tile loader of the wide-state form's full tiles, 'wide' (load_tile_wide, the default)
        or 'generic' (load_tile_generic); same bits.  Returns whether the next run's launches use load_tile_wide."""
        if loader not in ('wide', 'generic'): raise ValueError("param <loader> not in ['wide', 'generic']")
        used = C.c_int()
        _check(lib().gnn_loop_set_wide_loader(self._h, C.c_int(0 if loader == 'wide' else 1), C.byref(used)))
        return bool(used.value)

    def label_projection(self) -> np.ndarray:
        """gnn_loop_get_label_projection (test hook): the projection the last run used, [owned rows, width of net_state's first layer]."""
        out = np.zeros((self.n_rows, int(self._keep[1].dims[1])), np.float32)
        _check(lib().gnn_loop_get_label_projection(self._h, _fp(out)))
        return out

    def counters(self) -> dict:
        """gnn_counters_get: algorithmic bytes / FLOPs of one iteration on the owned rows, and the last run's iteration count and times."""
        b, f, it, tot, avg = C.c_double(), C.c_double(), C.c_int(), C.c_float(), C.c_float()
        _check(lib().gnn_counters_get(self._h, C.byref(b), C.byref(f), C.byref(it), C.byref(tot), C.byref(avg)))
        return dict(bytes_per_iteration=b.value, flops_per_iteration=f.value, iterations=it.value, total_ms=tot.value, avg_iteration_ms=avg.value)

    @staticmethod
    def lgnn_run(loops, graphs, get_state: bool, get_output: bool) -> list:
        """gnn_lgnn_run: LGNN.Loop of a whole stack in one call (loops[i] created on graphs[i], graphs[0] the original graph)."""
        n = len(loops)
        ks = (C.c_float * n)()
        _check(lib().gnn_lgnn_run((C.c_void_p * n)(*[x._h for x in loops]), (C.c_void_p * n)(*[x._h for x in graphs]), C.c_int(n),
                                  C.c_int(bool(get_state)), C.c_int(bool(get_output)), ks))
        return [float(k) for k in ks]

    def drop_cached_aggregates(self):
        _check(lib().gnn_loop_drop_cached_aggregates(self._h))

    def set_profiling(self, on: bool):
        _check(lib().gnn_loop_set_profiling(self._h, C.c_int(bool(on))))

    def run(self, training: bool = False) -> float:
        k = C.c_float(0)
        _check(lib().gnn_loop_run(self._h, C.c_int(bool(training)), C.byref(k)))
        return float(k.value)

    @staticmethod
    def run_many(loops) -> list:
        """gnn_loop_run_many: independent loops (batches of a dataset) in one call; small graphs run side by side.  Returns [k per loop]."""
        n = len(loops)
        hs = (C.c_void_p * n)(*[l._h for l in loops])
        ks = (C.c_float * n)()
        _check(lib().gnn_loop_run_many(hs, C.c_int(n), ks))
        return [float(x) for x in ks]

    @staticmethod
    def run_group(loops) -> float:
        """gnn_loop_run_group: one Loop on all ranks of a loopback group (rank order)."""
        n = len(loops)
        hs = (C.c_void_p * n)(*[l._h for l in loops])
        k = C.c_float(0)
        _check(lib().gnn_loop_run_group(hs, C.c_int(n), C.byref(k)))
        return float(k.value)

    @staticmethod
    def readout_group(loops, ng_indptr, ng_node, ng_w) -> np.ndarray:
        n = len(loops)
        hs = (C.c_void_p * n)(*[l._h for l in loops])
        ng_indptr = np.ascontiguousarray(ng_indptr, dtype=np.int32)
        ng_node = np.ascontiguousarray(ng_node, dtype=np.int32)
        ng_w = _f32(ng_w)
        g = len(ng_indptr) - 1
        out = np.empty((g, loops[0].T), dtype=np.float32)
        _check(lib().gnn_loop_readout_group(hs, C.c_int(n), C.c_int(g), _ip(ng_indptr), _ip(ng_node), _fp(ng_w), _fp(out)))
        return out

    def timing(self):
        tot, avg, n = C.c_float(), C.c_float(), C.c_int()
        _check(lib().gnn_loop_get_timing(self._h, C.byref(tot), C.byref(avg), C.byref(n)))
        gap = C.c_float()
        _check(lib().gnn_loop_get_exchange_timing(self._h, C.byref(gap)))
        return dict(total_ms=tot.value, avg_iter_ms=avg.value, n_iter_timed=n.value, avg_between_bodies_ms=gap.value)

    def state(self) -> np.ndarray:
        out = np.empty((self.n_rows, self.Ds), dtype=np.float32)
        _check(lib().gnn_loop_get_state(self._h, _fp(out)))
        return out

    def output(self) -> np.ndarray:
        out = np.empty((self.n_masked, self.T), dtype=np.float32)
        m = C.c_int64(0)
        _check(lib().gnn_loop_get_output(self._h, _fp(out), C.byref(m)))
        return out

    def readout(self, ng_indptr, ng_node, ng_w) -> np.ndarray:
        ng_indptr = np.ascontiguousarray(ng_indptr, dtype=np.int32)
        ng_node = np.ascontiguousarray(ng_node, dtype=np.int32)
        ng_w = _f32(ng_w)
        g = len(ng_indptr) - 1
        out = np.empty((g, self.T), dtype=np.float32)
        _check(lib().gnn_loop_readout(self._h, C.c_int(g), _ip(ng_indptr), _ip(ng_node), _fp(ng_w), _fp(out)))
        return out

    def close(self):
        if self._h:
            lib().gnn_loop_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
