"""tests/fp16_form_cases.py on the CPU: every row of the table answers the form it names through the host-only form queries, and the inputs of
tests/test_gpu_fp16_forms.py - not the kernel - decide each verdict: emulated in numpy, no operand of a case that expects no repeat reaches
4,094 at any cut (every aggregated column and every hidden unit included), and exactly one operand of a case that expects one does, at the
intended cut."""
import numpy as np
import pytest

import fp16_form_cases as fc
from test_fp16_edges import UNDER, cut, cut_pieces

IDS = [r['id'] for r in fc.FORMS]


def _engine():
    from GNN import _engine
    return _engine


def _verdict(case):
    """The case's inputs decide what it expects; returns the largest operand over all cuts."""
    state, ops = fc.emulate(case)
    want = {case['trip']: (case['count'], 1)} if case['trip'] else {}      # one operand, or one unit's on every row
    assert fc.reaching(ops) == want, (case['row']['id'], fc.reaching(ops), want)
    if case['want'] is not None: assert np.array_equal(state, case['want'])
    return max(float(v.max()) for v in ops.values())


@pytest.mark.parametrize('name', IDS)
def test_form_of_every_row(name):
    e = _engine()
    r = fc.BY_ID[name]
    ds, nl, al, acts = r['ds'], r['nl'], r['al'], r['acts']
    dims = fc.dims_of(r)
    assert dims[0] == 2 * ds + 2 * nl + al and fc.N % 32 and fc.N >= 3 * 32
    # the instantiation: of the net as it stands, or of the shadow net over [state | aggregated state] that a seeded launch runs
    f = e.fused_net_form(fc.dims_of(r, shadow=True), acts, 0) if r['seeded'] else e.fused_net_form(dims, acts, nl)
    assert f['covered'] and (f['NT'], f['NTL']) == r['tiles'] and f['mixed'] == (r['kind'] == 'M')
    assert f['hidden'] == acts[0] and f['last'] == acts[-1]
    # the persistent small-graph loop (exact arithmetic) would take the 32-wide nets on these rows: the GPU tests forbid it on every loop
    assert e.small_form(dims, acts, fc.N, nl)['persistent'] == (r['id'].startswith('G11'))
    proj = e.label_projection_form(dims, acts, ds, nl, al, fc.N, r['proj'])
    wide = e.wide_state_form(dims, acts, ds, nl, al, fc.N, r['wide'], r['proj'])
    if r['wide'] == 'always':
        assert 68 <= ds <= 128 and wide == dict(taken=True, kernel=1, waves=r['waves'], seeded=r['seeded']) and 4 <= r['waves'] <= 7
        assert r['kernel'] == 1 and not proj['seeded']                  # (the projection alone has no eight-wave tile for a state this wide)
    else:
        assert wide == dict(taken=False, kernel=0, waves=0, seeded=False) and r['waves'] == 8
        assert proj['seeded'] == r['seeded'] and r['kernel'] == (2 if ds == 64 else 1)
        if r['seeded']: assert proj['kernel'] == r['kernel'] and proj['iw'] == 2 * nl + al and proj['tiles'] == r['tiles'][0]
    if r['seeded'] and nl > 1:                                          # wide labels: seeded because nothing else covers the net
        assert r['proj'] == 'auto' and not e.label_projection_form(dims, acts, ds, nl, al, fc.N, 'off')['seeded']
    if r['seeded'] and nl == 1:                                         # narrow labels: covered as it stands, seeded on request
        assert r['proj'] == 'always' and not e.label_projection_form(dims, acts, ds, nl, al, fc.N, 'auto')['seeded']


def test_the_table_holds_the_listed_forms():
    kinds = [r['kind'] for r in fc.FORMS]
    assert kinds.count('G') == 7 and kinds.count('W') == 4 and kinds.count('S') == 7 and kinds.count('M') == 4 and len(set(IDS)) == len(IDS)
    assert {r['tiles'] for r in fc.FORMS if r['kind'] == 'G'} == {(1, 1), (2, 2), (4, 2)}
    assert sorted(r['waves'] for r in fc.FORMS if r['kind'] == 'W') == [4, 5, 5, 7]
    assert fc.hidden_units(fc.BY_ID['G22-40-h48']) == [(1, 5), (1, 40)]                       # unit 40: the padded second tile
    assert fc.hidden_units(fc.BY_ID['W5-96-h128-128']) == [(l, u) for l in (1, 2) for u in (5, 40, 70, 100)]
    for name in fc.ACTIVATION_FORMS: assert len(fc.BY_ID[name]['hidden']) == 2
    assert {fc.BY_ID[n]['kind'] for n in fc.BOOKKEEPING_FORMS} == {'W', 'S'} and fc.BY_ID[fc.SHARDED_FORM]['ds'] == 128


@pytest.mark.parametrize('name', IDS)
def test_probe_set_of_every_form(name):
    """The chain's inputs: the probe set fits the rows, stays below the limit at every cut of both routes, and still holds ties in p0, ties in
    p1 and more than 500 values whose p1 is an fp16 subnormal (as test_emulated_cut_matches_host_packer asks of the whole set)."""
    r = fc.BY_ID[name]
    for route in ('own', 'agg'):
        case = fc.chain_case(r, route)
        assert _verdict(case) < 4094.0
        x = case['x'] if not r['seeded'] else np.delete(case['x'], [r['ds'] - 2, r['ds'] - 1], axis=1)
        s = x.astype(np.float32) * np.float32(16.0)
        p0, p1 = cut_pieces(x)
        half_ulp = lambda p: 0.5 * np.spacing(np.abs(p).astype(np.float32).clip(max=65000.0).astype(np.float16)).astype(np.float32)
        rem = s - p0.astype(np.float32)
        sub = (p1 != 0) & (np.abs(p1.astype(np.float32)) < 2.0 ** -14)
        tie0 = np.isfinite(s) & (rem != 0) & (np.abs(rem) == half_ulp(p0))
        rem1 = rem - p1.astype(np.float32)
        tie1 = (rem1 != 0) & (np.abs(rem1) == half_ulp(p1))
        assert sub.sum() >= 500 and tie0.sum() >= 100 and tie1.sum() >= 100, (route, int(sub.sum()), int(tie0.sum()), int(tie1.sum()))
        assert np.any(x == UNDER) and np.all(np.isfinite(p0))
        if r['kind'] == 'M': assert case['s0'].min() >= 0.0             # every activation of the net is the identity there
        else: assert np.any(x == -UNDER)
        if r['seeded']:                                                  # the label terms are not cut at layer 0: one cut fewer
            L = len(r['hidden']) + 1
            for j in (r['ds'] - 2, r['ds'] - 1): assert np.array_equal(case['want'][:, j], cut(case['x'][:, j], L - 1))


@pytest.mark.parametrize('name', IDS)
def test_layer0_inputs_decide(name):
    r = fc.BY_ID[name]
    for where in fc.WHERES:
        for pos in fc.ROWS:
            for at_limit in (True, False):
                case = fc.layer0_case(r, where, pos, at_limit)
                cut_here = not (r['seeded'] and where in ('label', 'agg_label', 'agg_arc'))
                assert (case['trip'] == 'b0.layer0') == (at_limit and cut_here), (where, pos, at_limit)
                _verdict(case)
                big = fc.concat(case['g'], case['s0'])[fc.ROWS[pos], fc.block_start(r, where) + fc.COL[where]]
                assert big == (fc.LIMIT if at_limit else UNDER), (where, pos, at_limit, big)      # 2,047 + 2,047 and UNDER/2 + UNDER/2 are exact
    assert fc.ROWS['full'] // 32 < fc.N // 32 and fc.ROWS['partial'] // 32 == fc.N // 32 and fc.ROWS['partial'] == fc.N - 1


@pytest.mark.parametrize('name', [r['id'] for r in fc.FORMS if r['hidden']])
def test_hidden_inputs_decide(name):
    r = fc.BY_ID[name]
    units = fc.hidden_units(r)
    assert {(l, u // 32) for l, u in units} == {(l, t) for l, w in enumerate(r['hidden'], 1) for t in range((w + 31) // 32)}
    for layer, unit in units:
        for at_limit in (True, False):
            case = fc.hidden_case(r, layer, unit, at_limit)
            assert case['trip'] == (f'b0.hidden{layer}' if at_limit else None)
            _verdict(case)
            if not at_limit:
                L = len(r['hidden']) + 1
                later = cut(np.float32(0.5) * cut(UNDER)) if layer < L - 1 else cut(UNDER)
                assert np.all(case['want'][:, unit % r['ds']] == later)


@pytest.mark.parametrize('name', fc.ACTIVATION_FORMS)
def test_activation_inputs_decide(name):
    r = fc.BY_ID[name]
    for act, v, trips in fc.ACTIVATIONS:
        case = fc.activation_case(r, act, v, trips)
        _verdict(case)
        assert (case['want'] is not None) == (not trips and act != 'selu')
    # selu: the guard reads log2(e) v - 3,000 reaches the limit, 2,600 (and what the next layer makes of it) does not
    assert 3000.0 * fc.LOG2E >= 4094.0 > 2600.0 * fc.LOG2E and 16 * 3000.0 < 65504.0


@pytest.mark.parametrize('name', [r['id'] for r in fc.FORMS if r['seeded']])
def test_seeded_inputs_decide(name):
    r = fc.BY_ID[name]
    L = len(r['hidden']) + 1
    for value in (5000.0, 1e5):
        case = fc.zeroed_label_case(r, value, True)
        _verdict(case)
        assert np.array_equal(case['want'], fc.zeroed_label_case(r, None, True)['want'])
        if r['nl'] == 1: _verdict(fc.zeroed_label_case(r, value, False, arc=False))
    if L > 1:
        for pos in fc.ROWS:
            _verdict(fc.unit_weight_case(r, fc.LIMIT, True, 'b0.hidden1', pos))
            case = fc.unit_weight_case(r, UNDER, True, None, pos)
            _verdict(case)
            assert np.array_equal(case['want'][:, fc.LABEL_UNIT], fc.behind_label_unit(case['x'][:, fc.LABEL_UNIT], L))
            if r['nl'] == 1:
                off = fc.unit_weight_case(r, UNDER, False, None, pos)
                _verdict(off)
                # the cut is idempotent (p0 + p1 is its own cut), so behind a hidden layer both expectations are the same bits: the two
                # differ only where nothing is cut behind the label - the one-layer form below
                assert np.array_equal(off['want'], case['want'])
    else:
        one = fc.unit_weight_case(r, 1e5, True, None)
        _verdict(one)
        assert one['want'][fc.ROWS['partial'], fc.LABEL_UNIT] == np.float32(1e5)
        _verdict(fc.unit_weight_case(r, 1e5, True, 'b1.layer0', bodies=2))
        _verdict(fc.unit_weight_case(r, 1e5, False, 'b0.layer0'))           # unseeded, layer 0 cuts the label itself
        seeded, off = fc.unit_weight_case(r, UNDER, True, None), fc.unit_weight_case(r, UNDER, False, None)
        _verdict(seeded); _verdict(off)
        col = seeded['g']['nodes'][:, 0]
        assert np.array_equal(seeded['want'][:, fc.LABEL_UNIT], col) and np.array_equal(off['want'][:, fc.LABEL_UNIT], cut(col))
        assert np.sum(seeded['want'] != off['want']) > 100                  # the two expectations really differ


def test_bookkeeping_and_sharded_inputs_decide():
    e = _engine()
    for name in fc.BOOKKEEPING_FORMS:
        case, small = fc.bookkeeping_case(fc.BY_ID[name])
        _verdict(case)
        again = dict(case, s0=small, trip=None, want=None)
        assert _verdict(again) <= 400.0 and not np.array_equal(fc.emulate(again)[0], small)
    case = fc.sharded_case()
    _verdict(case)
    rb, nr = e.shard_range(fc.N, 1, 2)
    x = fc.concat(case['g'], case['s0'])
    rows = np.flatnonzero((np.abs(x) >= 4094.0).any(1))
    assert list(rows) == [fc.N - 1] and rb <= fc.N - 1 < rb + nr and rb > 0
