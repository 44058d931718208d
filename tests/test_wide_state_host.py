"""The wide-state form's decision from shapes alone (gnn_wide_state_form: host code, no device), the cases of tests/wide_state_cases.py
against what they were chosen for, and the argument checks of the Python setters."""
import numpy as np
import pytest

import wide_state_cases as wc

LDS_LIMIT = 160 * 1024


def _engine():
    from GNN import _engine
    return _engine


def lds_bytes(concat, waves):
    """LDS of a workgroup of `waves` waves on a net_state of `concat` input columns and a state width other than 64: per
    wave a tile [32][KP] of floats, KP = max(2 kk0, concat rounded up to 16) + 1 with kk0 = K-steps of 2 rounded up to groups of 12, and
    36 row-pointer words; 128 bytes of slack, five staged vectors of 128 floats, 16 bytes."""
    kk0 = ((concat + 1) // 2 + 11) // 12 * 12
    kp = max(2 * kk0, (concat + 15) // 16 * 16) + 1
    return waves * 32 * kp * 4 + 128 + waves * 36 * 4 + 5 * 32 * 4 * 4 + 16


def expected_waves(concat):
    fit = [w for w in range(1, 9) if lds_bytes(concat, w) <= LDS_LIMIT]
    return max(fit) if fit else 0


@pytest.mark.parametrize('i', range(len(wc.CASES)))
def test_cases_are_what_they_were_chosen_for(i):
    ref_err, margin = wc.check_case(i)
    print(f'case {i}: |C oracle - float64| {ref_err:.2e}, mover margin {margin:.0f} x band')


@pytest.mark.parametrize('i', range(len(wc.CASES)))
def test_form_of_the_cases(i):
    e = _engine()
    c = wc.CASES[i]
    dims, acts, d, nl, al, n = wc.net_description(i)
    assert dims[0] == 2 * d + 2 * nl + al
    assert e.wide_state_form(dims, acts, d, nl, al, n, 'off') == dict(taken=False, kernel=0, waves=0, seeded=False)
    assert expected_waves(dims[0]) < 8, 'the eight-wave path covers the case'
    for mode in ('auto', 'always'):
        plain = e.wide_state_form(dims, acts, d, nl, al, n, mode)
        both = e.wide_state_form(dims, acts, d, nl, al, n, mode, 'auto')
        if c.get('seeded'):
            assert expected_waves(dims[0]) < 4 and plain == dict(taken=False, kernel=0, waves=0, seeded=False)
            assert expected_waves(2 * d) == c['waves']                   # the net over [state | aggregated state]
            assert both == dict(taken=True, kernel=1, waves=c['waves'], seeded=True)
        else:
            assert expected_waves(dims[0]) == c['waves'] >= 4
            assert plain == dict(taken=True, kernel=1, waves=c['waves'], seeded=False)
            assert both == plain                                         # projection 'auto': the net as it stands has a form of its own
            forced = e.wide_state_form(dims, acts, d, nl, al, n, mode, 'always')
            assert forced == dict(taken=True, kernel=1, waves=expected_waves(2 * d), seeded=True)
    assert (c['waves'] == 4) == (d == 128) and (i not in (2, 4) or c['waves'] > 4)


def _form(d, hidden, acts, nl=3, al=2, n=333, mode='always', projection='off'):
    dims = [2 * d + 2 * nl + al] + list(hidden) + [d]
    return _engine().wide_state_form(dims, acts, d, nl, al, n, mode, projection)


NOT_TAKEN = dict(taken=False, kernel=0, waves=0, seeded=False)


@pytest.mark.parametrize('mode', ['auto', 'always'])
def test_refusals(mode):
    assert _form(128, (128, 128), ['tanh'] * 3, mode=mode)['taken']                       # the shape the others differ from
    assert _form(66, (128, 128), ['tanh'] * 3, nl=8, mode=mode) == NOT_TAKEN              # state width no multiple of 4
    assert _form(132, (128, 128), ['tanh'] * 3, mode=mode) == NOT_TAKEN                   # state wider than 128
    assert _form(128, (200, 128), ['tanh'] * 3, mode=mode) == NOT_TAKEN                   # a hidden layer wider than 128
    assert _form(128, (128,), ['tanh', 'softmax'], mode=mode) == NOT_TAKEN                # softmax
    assert _form(128, (128, 128), ['tanh', 'relu', 'tanh'], mode=mode) == NOT_TAKEN       # two hidden activations
    assert _form(128, (128, 128), ['tanh'] * 3, mode='off') == NOT_TAKEN
    assert _form(128, (128, 128), ['tanh'] * 3, n=0, mode=mode) == NOT_TAKEN
    assert _form(128, (128, 128), ['tanh'] * 3, nl=40, mode=mode) == NOT_TAKEN            # no four-wave tile without the projection
    assert _form(32, (64,), ['tanh'] * 2, nl=150, mode=mode) == NOT_TAKEN                 # a narrow state under wide labels: the projection's ground


@pytest.mark.parametrize('mode', ['auto', 'always'])
@pytest.mark.parametrize('projection', ['off', 'auto', 'always'])
def test_nets_the_eight_wave_path_covers_are_left_alone(mode, projection):
    for d, nl in ((64, 3), (68, 1), (32, 3), (20, 3)):
        concat = 2 * d + 2 * nl + 2
        assert d == 64 or expected_waves(concat) == 8
        assert _form(d, (128, 128), ['tanh'] * 3, nl=nl, mode=mode, projection=projection) == NOT_TAKEN, d
    # width 64 under wide labels is the full-tile kernel's, seeded or not: eight waves
    assert _form(64, (128, 128), ['tanh'] * 3, nl=40, al=3, mode=mode, projection=projection) == NOT_TAKEN


def test_wave_counts_follow_the_lds_formula():
    e = _engine()
    seen = set()
    for d in range(68, 129, 4):
        for nl in (0, 1, 3, 7, 12, 20, 40):
            for al in (0, 2):
                concat = 2 * d + 2 * nl + al
                want = expected_waves(concat)
                got = e.wide_state_form([concat, 128, d], ['selu', 'selu'], d, nl, al, 1000, 'always')
                if 4 <= want < 8: assert got == dict(taken=True, kernel=1, waves=want, seeded=False), (d, nl, al, want, got)
                else: assert got == NOT_TAKEN, (d, nl, al, want, got)
                seen.add(want if 4 <= want < 8 else 0)
    assert seen == {0, 4, 5, 6, 7}
    assert lds_bytes(2 * 128 + 2 * 3 + 2, 4) <= LDS_LIMIT < lds_bytes(2 * 128 + 2 * 3 + 2, 5)


def test_setter_arguments():
    from GNN.GNN import GNNnodeBased
    from GNN.LGNN import LGNN
    e = _engine()
    assert e.wide_state_mode('off') == 0 and e.wide_state_mode('auto') == 1 and e.wide_state_mode('always') == 2 and e.wide_state_mode(2) == 2
    for bad in ('on', 3, -1, True, 1.5, None):
        with pytest.raises((ValueError, TypeError)): e.wide_state_mode(bad)
        with pytest.raises((ValueError, TypeError)): GNNnodeBased.set_wide_state(object.__new__(GNNnodeBased), bad)
    with pytest.raises(ValueError): e.wide_state_form([10, 4], ['tanh', 'tanh'], 4, 1, 0, 10, 'always')
    with pytest.raises(ValueError): e.wide_state_form([264, 128], ['tanh'], 128, 3, 2, 10, 'sometimes')
    with pytest.raises(ValueError): e.wide_state_form([264, 128], ['tanh'], 128, 3, 2, 10, 'always', 'sometimes')
    with pytest.raises(ValueError): e.wide_state_form([264, 128], ["tanh"], 0, 3, 2, 10, "always")          # (the library's own argument check)
    model = object.__new__(GNNnodeBased)
    for mode, name in ((0, 'off'), ('auto', 'auto'), (2, 'always')):
        model.set_wide_state(mode)
        assert model.wide_state == name
    assert callable(LGNN.set_wide_state)
    for name in ('set_wide_state', 'body_launch', 'set_grid_limit', 'set_wide_loader'): assert callable(getattr(e.Loop, name))
