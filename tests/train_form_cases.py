"""The nets of tests/test_gpu_train_forms.py with the kernels each of them is meant to launch, shared with tests/test_train_forms_host.py (which
checks the expectations on the CPU through gnn_train_forms).  Inputs only, no reference code.

A case is one net_state on one row count.  `fwd` / `bwd` / `wg` give the expected form of every Dense layer in one letter:
    fwd   P k_dense_fwd      M all layers in k_mlp_fwd     W k_gemm_split          C inside k_fwd3_split
    bwd   P k_layer_bwd      W k_gemm_split on W^T         C inside k_bwd3_split
    wg    P k_layer_bwd      B k_wgrad_bf                  F k_wgrad_f32
The concat is K0 = AL + 2 (Ds + NL) wide (Ds = the last width): `al` and `nl` are chosen to hit dims[0]."""
from collections import namedtuple

Case = namedtuple('Case', 'name dims act bn drop1 n al nl fwd bwd wg seed')

LETTER = {'per_op': 'P', 'mlp_fwd': 'M', 'wide': 'W', 'chain3': 'C', 'wgrad_bf': 'B', 'wgrad_f32': 'F'}

MIN_ROWS = 4096                     # the matrix-core forms start here (asserted on both sides by test_train_forms_host.py)
N_SMALL = 4113                      # 128 full 32-row tiles + 17 rows


def n_second_sweep(sweep_rows):
    """Rows with which 25 waves of the persistent kernels take a second tile, the last of them a partial one (66,321 for a sweep of 65,536)."""
    return sweep_rows + 8 * 32 * 3 + 17


def _c(name, dims, act, fwd, bwd, wg, n=N_SMALL, bn=False, drop1=0.0, seed=1):
    ds = dims[-1]
    rest = dims[0] - 2 * ds
    al = 1 + (rest + 1) % 2
    nl = (rest - al) // 2
    assert nl >= 1 and al + 2 * (ds + nl) == dims[0] and len(fwd) == len(bwd) == len(wg) == len(dims) - 1
    return Case(name, tuple(dims), act, bn, drop1, n, al, nl, fwd, bwd, wg, seed)


WIDE3 = (135, 128, 128, 64)

# C1: every form at the smallest size.  (The issue's two-layer row 64 -> 65 -> 64 cannot be a net_state: a 64-wide concat leaves Ds + NL <= 31.
# A 16-wide third layer carries the state instead; the two wide layers in front of it are the row's.)  The two last rows complete the
# weight-gradient instantiations: k_wgrad_bf<3,4>, <4,2> and k_wgrad_f32<3,2> on five column tiles, <4,2> on three and on five.
C1 = [
    _c('chain_linear', WIDE3, 'linear', 'CCC', 'CCC', 'BBB'),
    _c('chain_sigmoid', WIDE3, 'sigmoid', 'CCC', 'CCC', 'BBB'),
    _c('chain_relu_k144', (144, 128, 128, 64), 'relu', 'CCC', 'CCC', 'BBB'),
    _c('chain_elu_narrow', (135, 68, 72, 36), 'elu', 'CCC', 'WWP', 'FFP'),
    _c('two_wide_k64', (64, 65, 64, 16), 'sigmoid', 'WWP', 'WWP', 'FBP'),
    _c('five_tiles', (135, 144, 64), 'tanh', 'WW', 'WW', 'FB'),
    _c('one_layer_bn', (135, 64), 'tanh', 'W', 'W', 'B', bn=True),
    _c('four_layers', (135, 128, 96, 128, 64), 'tanh', 'WWWW', 'WWWW', 'BFBB'),
    _c('mixed_wide_input', (145, 128, 64), 'tanh', 'PW', 'WW', 'BB'),
    _c('mixed_narrow_middle', (135, 128, 32, 64), 'tanh', 'WWP', 'WPP', 'BPP'),
    _c('wgrad_tiles_a', (135, 80, 140, 100, 96, 64), 'tanh', 'WWWWW', 'WWWWW', 'FFBFB'),
    _c('wgrad_tiles_b', (135, 100, 140, 80, 128, 64), 'tanh', 'WWWWW', 'WWWWW', 'BFFBB'),
    _c('rows_4095', WIDE3, 'linear', 'MMM', 'PPP', 'PPP', n=MIN_ROWS - 1),
    _c('rows_4096', WIDE3, 'linear', 'CCC', 'CCC', 'BBB', n=MIN_ROWS),
]
# C4: the kinked activations (chain_relu_k144 above is the other one); seeds chosen on the CPU so that the rows silenced next to a kink stay few
C4 = [_c('chain_selu', WIDE3, 'selu', 'CCC', 'CCC', 'BBB')]


def c2(sweep_rows):
    """C2: a second tile per wave."""
    n = n_second_sweep(sweep_rows)
    return [
        _c('sweep_chain', WIDE3, 'tanh', 'CCC', 'CCC', 'BBB', n=n),
        _c('sweep_dropout', WIDE3, 'tanh', 'WWW', 'WWW', 'BBB', n=n, drop1=0.1),
        _c('sweep_five_tiles', (135, 144, 64), 'tanh', 'WW', 'WW', 'FB', n=n),
    ]


def all_cases(sweep_rows):
    return C1 + C4 + c2(sweep_rows)


def rates(case):
    """Dropout rate in front of every Dense layer and of BatchNormalization."""
    r = [0.0] * len(case.dims)
    r[1] = case.drop1
    return r


def passes(width):
    """Column passes of a matrix-core product with `width` output columns: 32-column tiles taken four, two or one at a time (launch_gemm_f32)."""
    out, left = [], (width + 31) // 32
    while left > 0:
        no = 4 if left >= 4 else 2 if left >= 2 else 1
        out.append(no)
        left -= no
    return out


def kernels(dims, act, forms):
    """The kernel instantiations behind a form report (train_forms() of GNN/_engine.py): the template arguments follow from the widths as in
    the launchers - k_gemm_split<NO> per pass, k_wgrad_bf<mt, nt> / k_wgrad_f32<mt, 2> on nt column tiles with mt = tiles of [H | 1]."""
    out = set()
    for l, (f, b, w) in enumerate(zip(forms['forward'], forms['backward'], forms['wgrad'])):
        ni, no = dims[l], dims[l + 1]
        mt, nt = (ni + 1 + 31) // 32, (no + 31) // 32
        out.add({'per_op': 'k_dense_fwd', 'mlp_fwd': 'k_mlp_fwd', 'chain3': f'k_fwd3_split<{act}>', 'wide': f'k_gemm_split fwd {passes(no)}'}[f])
        out.add({'per_op': 'k_layer_bwd', 'chain3': 'k_bwd3_split', 'wide': f'k_gemm_split bwd {passes(ni)}'}[b])
        out.add({'per_op': 'k_layer_bwd', 'wgrad_bf': f'k_wgrad_bf<{mt},{nt}>', 'wgrad_f32': f'k_wgrad_f32<{mt},2> nt={nt}'}[w])
    return out


# Every instantiation the predicates can select with layer widths up to 160 (the largest width a predicate names), derived by enumeration in
# tests/test_train_forms_host.py; the table above launches each of them (last test of tests/test_gpu_train_forms.py).
# k_wgrad_bf<M,1> and k_wgrad_f32<M,1> are compiled but unreachable: a matrix-core weight gradient needs the backward product of its layer on
# the matrix cores as well, whose K = n_out must be at least 64 - two column tiles.
REACHABLE = (
    {'k_dense_fwd', 'k_mlp_fwd', 'k_layer_bwd', 'k_bwd3_split'}
    | {f'k_fwd3_split<{a}>' for a in ('linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid')}
    | {f'k_gemm_split fwd {p}' for p in ([1], [2], [2, 1], [4], [4, 1])}
    | {f'k_gemm_split bwd {p}' for p in ([2], [2, 1], [4], [4, 1])}
    | {f'k_wgrad_bf<{mt},{nt}>' for mt in (3, 4, 5) for nt in (2, 4)}
    | {f'k_wgrad_f32<{mt},2> nt={nt}' for mt in (3, 4, 5) for nt in (3, 5)})


def letters(forms):
    return tuple(''.join(LETTER[x] for x in forms[k]) for k in ('forward', 'backward', 'wgrad'))
