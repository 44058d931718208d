"""The launch form of a Loop is decided once per run (gnn_loop_decide_form, csrc/gnn_fused.hip) from settings that may change between
runs.  One handle is taken through a sequence of setter calls; after every step its run must be the run of a FRESH handle that had those
settings from the start: the same `used` answer of every setter, the same k, and states and outputs equal bit for bit (both handles launch
the same kernels with the same arguments, so there is no tolerance to choose)."""
import numpy as np
import pytest

from util import make_mlp

pytestmark = pytest.mark.gpu

DEFAULTS = dict(impl=2, pieces=2, tile_form=0, gather_form=0, persistent=True, profiling=False)


def _engine():
    from GNN import _engine
    return _engine


def _used(lp, cfg):
    """Every setter's `used` for the handle's current settings (each setter is called again with the value it already has).  A fresh handle
    gets its settings this way; the handle under test is only asked after it has run."""
    return dict(impl=lp.set_impl(cfg['impl']), pieces=lp.set_pieces(cfg['pieces']), tile_form=lp.set_tile_form(cfg['tile_form']),
                gather_form=lp.set_gather_form(cfg['gather_form']), persistent=lp.set_persistent(cfg['persistent']))


class Case:
    """A graph on the device, the nets' weights on the host, and a way to make loops on them."""

    def __init__(self, n, ds, hidden, seed):
        from GNN import GNN_utils as utils
        self.e = _engine()
        s = utils.syntheticGraph(n, 10.0 if n > 1000 else 3.0, 3, 1, 2, seed=seed)
        assert s['n_nodes'] == n
        rng = np.random.default_rng(seed)
        self.n, self.ds = n, ds
        self.st = make_mlp(rng, 1 + 2 * (3 + ds), list(hidden) + [ds], 'selu', gain=1.0, bn_random=True)
        self.st_new = make_mlp(rng, 1 + 2 * (3 + ds), list(hidden) + [ds], 'selu', gain=0.25, bn_random=True)      # other values AND another fp16 weight scale
        self.ou = make_mlp(rng, 3 + ds, [2], 'softmax', bn_random=True)
        self.s0 = (0.1 * rng.standard_normal((n, ds))).astype(np.float32)
        self.graph = self.e.Graph(n, s['indptr'], s['adj_src'], s['adj_w'], s['arc_w'], s['arc_labels_csr'], s['nodes'], np.ones(n, np.uint8))

    def loop(self, st):
        e = self.e
        mst, mou = e.Mlp(st['weights'], st['activations'], True), e.Mlp(self.ou['weights'], self.ou['activations'], True)
        lp = e.Loop(self.graph, mst, mou, self.ds, 6, 0.0)
        lp.set_state0(self.s0)
        return lp, mst

    def fresh_run(self, st, cfg):
        """(used, k, state, output) of a new handle, on new MLP handles, that gets the settings `cfg` before its first run."""
        lp, _ = self.loop(st)
        lp.set_profiling(cfg['profiling'])
        used = _used(lp, cfg)
        k = lp.run()
        res = (used, k, lp.state(), lp.output())
        lp.close()
        return res

    def check(self, lp, st, cfg, step):
        """The handle has had the step's own setter and nothing else since its last run: it runs on the form its loop_prepare decides.  The
        setters' answers are read AFTER the run (asking them decides the form again, which would hide a stale one)."""
        k = lp.run()
        state, out = lp.state(), lp.output()
        used = _used(lp, cfg)
        used_f, k_f, state_f, out_f = self.fresh_run(st, cfg)
        print(f'{step}: used {used}, k {k}; fresh handle: used {used_f}, k {k_f}, {int(np.sum(state != state_f))} of {state.size} state values differ')
        assert used == used_f, step
        assert k == k_f, step
        assert not np.isnan(state_f).any(), step
        assert np.array_equal(state, state_f) and np.array_equal(out, out_f), step
        self.last_k = k
        return used


def test_form_follows_every_setter_on_one_handle():
    """A net the wave pair covers (state 64, 135 -> 128 -> 128 -> 64) on 4,113 rows: 129 tiles, the last one partial."""
    c = Case(4113, 64, (128, 128), seed=4113)
    lp, mst = c.loop(c.st)
    cfg = dict(DEFAULTS)
    used = c.check(lp, c.st, cfg, '1 defaults')
    assert (used['impl'], used['tile_form'], used['gather_form'], used['persistent']) == (2, 2, 1, False)      # wave pair
    cfg['tile_form'] = 1
    assert lp.set_tile_form(1) == 1
    used = c.check(lp, c.st, cfg, '2 set_tile_form(1)')
    assert (used['tile_form'], used['gather_form']) == (1, 2)                          # full-tile kernel, gathering from the program
    cfg['gather_form'] = 1
    assert lp.set_gather_form(1) == 1
    used = c.check(lp, c.st, cfg, '3 set_gather_form(1)')
    assert (used['tile_form'], used['gather_form']) == (1, 1)                          # ... walking the CSR
    cfg['pieces'] = 3
    assert lp.set_pieces(3) == 3
    c.check(lp, c.st, cfg, '4 set_pieces(3)')
    cfg['impl'] = 1
    assert lp.set_impl(1) == 1
    c.check(lp, c.st, cfg, '5 set_impl(1)')
    cfg['impl'] = 0
    assert lp.set_impl(0) == 0
    used = c.check(lp, c.st, cfg, '6 set_impl(0)')
    assert (used['tile_form'], used['gather_form']) == (0, 0)
    cfg.update(impl=2, pieces=2, tile_form=0, gather_form=0)
    assert lp.set_impl(2) == 2 and lp.set_pieces(2) == 2 and lp.set_tile_form(0) == 2 and lp.set_gather_form(0) == 1
    c.check(lp, c.st, cfg, '7 set_impl(2), forms back to 0')
    mst.set_weights(c.st_new['weights'])
    c.check(lp, c.st_new, cfg, '8 set_weights')
    cfg['profiling'] = True
    lp.set_profiling(True)
    c.check(lp, c.st_new, cfg, '9 set_profiling(1)')
    lp.close()
    c.graph.close()


def test_persistent_form_follows_its_setters_on_one_handle():
    """100 rows, state width 8, one hidden layer of 16: the persistent small-graph loop on 16-node tiles."""
    c = Case(100, 8, (16,), seed=100)
    lp, _ = c.loop(c.st)
    cfg = dict(DEFAULTS)
    assert c.check(lp, c.st, cfg, 'defaults')['persistent'] is True
    cfg['persistent'] = False
    assert lp.set_persistent(False) is False
    assert c.check(lp, c.st, cfg, 'set_persistent(False)')['persistent'] is False
    cfg['persistent'] = True
    assert lp.set_persistent(True) is True
    assert c.check(lp, c.st, cfg, 'set_persistent(True)')['persistent'] is True
    cfg['profiling'] = True
    lp.set_profiling(True)
    assert c.check(lp, c.st, cfg, 'set_profiling(1)')['persistent'] is False           # a profiled run is one launch per body
    assert lp.timing()['n_iter_timed'] == c.last_k > 0                                  # (its bodies were timed one by one)
    lp.close()
    c.graph.close()


@pytest.mark.parametrize('hidden', [(), (48,), (128,), (128, 128)])
def test_state_width_64_never_takes_the_generic_kernel(hidden):
    """k_fused_generic has none of the width-64 paths (csrc/gnn_fused_kernel.h; its launcher refuses the width): a loop with state width
    64 reports k_fused_full or k_fused_pair in every mode the setters allow - impl 1 or 2, every tile form, the feature-sliced exchange on
    and off (two ranks over the loopback transport), every gather form - and on one GPU with and without the persistent path."""
    from test_gpu_sharded import _case, _csr_parts, _sharded_loops
    e = _engine()
    n, d = 333, 64
    g, st, ou, s0 = _case(64 + len(hidden), n, d, hidden=hidden)
    indptr, adj_src, adj_w, _, _ = _csr_parts(g)
    comms, graphs, loops, _ = _sharded_loops(e, g, st, ou, d, 5, 0.01, s0, 2, 1)
    for gr in graphs: gr.set_full_adjacency(n, indptr, adj_src, adj_w)
    seen = set()
    for lp in loops:
        for sliced in (False, True):
            lp.set_slice_exchange(sliced)
            for impl in (1, 2):
                assert lp.set_impl(impl) == impl
                for tile_form in (0, 1, 2):
                    lp.set_tile_form(tile_form)
                    for gather_form in (0, 1, 2):
                        lp.set_gather_form(gather_form)
                        kernel = lp.body_kernel()
                        assert kernel in (2, 3), (sliced, impl, tile_form, gather_form, kernel)
                        seen.add(kernel)
    for lp in loops: lp.close()
    for c in comms: c.close()
    case = Case(333, 64, hidden, 11)
    lp, _ = case.loop(case.st)
    for impl in (1, 2):
        assert lp.set_impl(impl) == impl
        for persistent in (True, False):
            lp.set_persistent(persistent)
            for tile_form in (0, 1, 2):
                lp.set_tile_form(tile_form)
                for gather_form in (0, 1, 2):
                    lp.set_gather_form(gather_form)
                    kernel = lp.body_kernel()
                    assert kernel in (2, 3), (impl, persistent, tile_form, gather_form, kernel)
                    seen.add(kernel)
    lp.close()
    assert 2 in seen and (3 in seen) == (hidden in ((128,), (128, 128)))      # the pair covers 128-wide hidden layers only
