"""gnn_train_forms (host code, no device): which kernels the training step picks for a net, asserted on both neighbours of every limit of the
form predicates (gnn_train_wide.hip: tg_many_rows, tg_wide, tg_wgrad_covers, tg_wgrad_bf, fwd3_covers, bwd3_covers; gnn_train_net.hip:
net_decide_form), and for every net of tests/train_form_cases.py - the table tests/test_gpu_train_forms.py runs on the device."""
import os
import subprocess

import pytest

import train_form_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T.MIN_ROWS


@pytest.fixture(scope='module')
def e():
    from GNN import _engine
    if not os.path.exists(_engine.LIB_PATH):          # fresh checkout: cross-compile for gfx950 (no GPU needed), exactly what build() does
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'gnn_tf_2.x_amd', 'csrc'), '-j8'], stdout=subprocess.DEVNULL)
    return _engine


def forms(e, dims, act='tanh', n=N, rates=None, state=True):
    acts = list(act) if isinstance(act, (list, tuple)) else [act] * (len(dims) - 1)
    return T.letters(e.train_forms(dims, acts, rates, n, state))


def test_row_threshold(e):
    below, at = e.train_forms(T.WIDE3, ['linear'] * 3, None, N - 1), e.train_forms(T.WIDE3, ['linear'] * 3, None, N)
    assert T.letters(below) == ('MMM', 'PPP', 'PPP') and below['build_input']
    assert T.letters(at) == ('CCC', 'CCC', 'BBB') and not at['build_input']
    assert not e.train_forms(T.WIDE3, ['linear'] * 3, None, N - 1, False)['build_input']         # net_output: its rows are gathered by the caller
    assert forms(e, (135, 64), n=N - 1) == ('P', 'P', 'P') and forms(e, (135, 64), n=N) == ('W', 'W', 'B')
    assert forms(e, (135, 64), n=0) == ('P', 'P', 'P')
    # one sweep of the persistent kernels: 32 rows per wave, 8 waves per block, 256 blocks
    assert at['sweep_rows'] == 32 * 8 * 256 and T.n_second_sweep(at['sweep_rows']) == 66321


@pytest.mark.parametrize('n_in,want', [(63, 'PPP'), (64, 'WWB'), (144, 'WWB'), (145, 'PWB'), (159, 'PWB'), (160, 'PPP')])
def test_input_width_limits(e, n_in, want):
    """Forward product: 64 <= n_in <= 144 (tg_wide).  Backward: the weight gradient's tiles of [H | 1], mt = 3 .. 5, i.e. n_in 64 .. 159
    (tg_wgrad_covers) - a layer too wide for the forward product still has both backward products on the matrix cores."""
    assert forms(e, (n_in, 64)) == tuple(want)


@pytest.mark.parametrize('n_out,want', [(31, 'PPP'), (32, 'WPP'), (63, 'WPP'), (64, 'WWB'), (65, 'WWF'), (96, 'WWF'), (97, 'WWB'), (128, 'WWB'), (129, 'WWF'),
                                        (144, 'WWF'), (145, 'WPP'), (160, 'WPP')])
def test_output_width_limits(e, n_out, want):
    """Forward: n_out >= 32.  Backward: n_out is the K of d h_in = d z . W^T, 64 .. 144; the weight gradient takes k_wgrad_bf on two or four
    column tiles and k_wgrad_f32 on three or five."""
    assert forms(e, (64, n_out)) == tuple(want)


def test_narrow_input_of_a_backward_product(e):
    # n_in is the output width of the backward product (>= 32), but mt >= 3 asks for n_in >= 64 first
    assert forms(e, (31, 64)) == ('P', 'P', 'P') and forms(e, (32, 64)) == ('P', 'P', 'P')


def test_softmax_is_not_an_epilogue(e):
    assert forms(e, (135, 64), 'softmax') == ('P', 'W', 'B')
    assert forms(e, (135, 128, 64), ['softmax', 'tanh']) == ('PW', 'WP', 'BP')      # (the way back through a softmax needs whole rows)


@pytest.mark.parametrize('dims,chain', [((63, 128, 128, 64), False), ((64, 128, 128, 64), True), ((144, 128, 128, 64), True), ((145, 128, 128, 64), False),
                                        ((135, 64, 128, 64), False), ((135, 65, 128, 64), True), ((135, 128, 64, 64), False), ((135, 128, 65, 64), True),
                                        ((135, 128, 128, 64), True), ((135, 129, 128, 64), False), ((135, 128, 129, 64), False),
                                        ((135, 128, 128, 32), False), ((135, 128, 128, 33), True), ((135, 128, 128, 65), False)])
def test_fwd3_width_limits(e, dims, chain):
    f = forms(e, dims)[0]
    assert (f == 'CCC') == chain and 'C' not in f.replace('CCC', '')


def test_fwd3_needs_three_layers_of_one_elementwise_activation(e):
    assert forms(e, (135, 128, 64))[0] == 'WW' and forms(e, (135, 128, 128, 128, 64))[0] == 'WWWW'
    for a in ('linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid'):
        assert forms(e, T.WIDE3, a) == ('CCC', 'CCC', 'BBB')
    assert forms(e, T.WIDE3, ['tanh', 'tanh', 'sigmoid']) == ('WWW', 'WWW', 'BBB')
    assert forms(e, T.WIDE3, ['relu', 'tanh', 'tanh']) == ('WWW', 'WWW', 'BBB')
    assert forms(e, T.WIDE3, 'softmax') == ('PPP', 'WPP', 'BPP')


def test_bwd3_limits(e):
    """Widths of whole 16-byte pieces; every layer's two backward products on the matrix cores.  (bwd3_covers also names dims[0] <= 160: the
    forward chain's 144 comes first, so that limit never decides.)"""
    assert forms(e, (135, 128, 128, 64)) == ('CCC', 'CCC', 'BBB')
    assert forms(e, (135, 126, 128, 64)) == ('CCC', 'WWW', 'BBB') and forms(e, (135, 128, 126, 64)) == ('CCC', 'WWW', 'BBB')
    assert forms(e, (135, 128, 128, 62)) == ('CCC', 'WWP', 'BBP')          # (a 62-wide d z is too narrow a K as well)
    assert forms(e, (135, 68, 72, 36)) == ('CCC', 'WWP', 'FFP')            # last layer's backward product: K = 36 < 64
    assert forms(e, (144, 128, 128, 64))[1] == 'CCC'
    for k0 in (145, 160, 161):
        assert 'C' not in ''.join(forms(e, (k0, 128, 128, 64)))


@pytest.mark.parametrize('pos,state,fwd,bwd', [(0, True, 'CCC', 'WWW'), (0, False, 'WWW', 'WWW'), (1, True, 'WWW', 'WWW'), (2, True, 'WWW', 'WWW'), (3, True, 'CCC', 'CCC')])
def test_dropout_positions(e, pos, state, fwd, bwd):
    """Dropout in front of the first layer rides on net_state's concat kernel (the forward chain stays; not so for net_output), between the
    layers it switches both chains off, in front of BatchNormalization neither."""
    r = [0.0] * 4
    r[pos] = 0.1
    assert forms(e, T.WIDE3, rates=r, state=state) == (fwd, bwd, 'BBB')


def test_weight_gradient_tiles(e):
    """mt = tiles of [H | 1] = (n_in + 32) // 32: 2 | 3 at n_in 63 | 64, 5 | 6 at 159 | 160; nt = column tiles of d z: 2, 4 -> k_wgrad_bf, 3, 5 -> k_wgrad_f32."""
    for n_in, n_out, want in [(63, 64, None), (64, 64, 'k_wgrad_bf<3,2>'), (95, 128, 'k_wgrad_bf<3,4>'), (96, 128, 'k_wgrad_bf<4,4>'), (127, 64, 'k_wgrad_bf<4,2>'),
                              (128, 64, 'k_wgrad_bf<5,2>'), (159, 128, 'k_wgrad_bf<5,4>'), (160, 128, None),
                              (64, 96, 'k_wgrad_f32<3,2> nt=3'), (127, 144, 'k_wgrad_f32<4,2> nt=5'), (159, 65, 'k_wgrad_f32<5,2> nt=3')]:
        ks = T.kernels((n_in, n_out), 'tanh', e.train_forms((n_in, n_out), ['tanh'], None, N))
        got = [k for k in ks if k.startswith('k_wgrad')]
        assert got == ([want] if want else []), (n_in, n_out, got)


def test_the_device_table_is_what_the_predicates_say(e):
    sweep = e.train_forms((135, 64), ['tanh'], None, N)['sweep_rows']
    cases = T.all_cases(sweep)
    assert len({c.name for c in cases}) == len(cases)
    seen = set()
    for c in cases:
        f = e.train_forms(c.dims, [c.act] * (len(c.dims) - 1), T.rates(c), c.n, True)
        assert T.letters(f) == (c.fwd, c.bwd, c.wg), c.name
        assert f['build_input'] == (c.n < N), c.name
        seen |= T.kernels(c.dims, c.act, f)
    assert seen == T.REACHABLE, (sorted(seen - T.REACHABLE), sorted(T.REACHABLE - seen))
    # net_output of every case: one softmax layer on Ds + NL <= 95 columns - always the per-op kernels
    assert forms(e, (67, 2), 'softmax', n=sweep, state=False) == ('P', 'P', 'P')


def test_reachable_instantiations_by_enumeration(e):
    """Every one-layer net with widths up to 160 on 4,096 rows, and the three-layer chain with each activation: the instantiations the
    predicates can select are exactly train_form_cases.REACHABLE."""
    seen = set()
    for n_in in range(1, 161):
        for n_out in range(1, 161):
            seen |= T.kernels((n_in, n_out), 'tanh', e.train_forms((n_in, n_out), ['tanh'], None, N))
    for a in ('linear', 'relu', 'selu', 'elu', 'tanh', 'sigmoid'):
        seen |= T.kernels(T.WIDE3, a, e.train_forms(T.WIDE3, [a] * 3, None, N))
    seen |= T.kernels(T.WIDE3, 'tanh', e.train_forms(T.WIDE3, ['tanh'] * 3, None, N - 1))
    assert seen == T.REACHABLE, (sorted(seen - T.REACHABLE), sorted(T.REACHABLE - seen))


def test_bad_descriptions_are_refused(e):
    with pytest.raises(ValueError):
        e.train_forms((135, 0), ['tanh'], None, N)
    with pytest.raises(ValueError):
        e.train_forms((135, 64), ['tanh'], None, -1)
