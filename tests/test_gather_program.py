"""The gather program's builder (gnn_gather_program_build, host code): from the program alone every row's (source, weight) sequence is
the CSR's, padding lies behind its group's last row end, the four row ranges of a tile are contiguous and cover it, and the largest
group is as small as any contiguous split allows."""
import itertools

import numpy as np
import pytest

ROW_END, NOROW = 32, 0xfffffe00


def _engine():
    from GNN import _engine
    return _engine


def csr_from_degrees(rng, deg, n_src):
    """Rows with the given entry counts, sources drawn without repetition per row, the weights of a row all distinct."""
    deg = np.asarray(deg, np.int64)
    indptr = np.zeros(deg.size + 1, np.int32)
    np.cumsum(deg, out=indptr[1:])
    src = np.concatenate([np.sort(rng.choice(n_src, d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    w = 0.25 + rng.permutation(src.size) / (4.0 * max(1, src.size))
    w = (w / np.repeat(deg, deg)).astype(np.float32)          # (a row's weights sum to less than 1)
    assert all(np.unique(w[a:b]).size == b - a for a, b in zip(indptr[:-1], indptr[1:]))
    return indptr, src, w


def hand_built_degrees():
    """The tiles of the issue's list, 32 rows each (group = the 8 consecutive rows a lane group of the CSR-walking loader owns)."""
    tiles = []
    for p in range(8):                                   # an empty row at each position of a group, first and last included
        t = np.full(32, 3)
        t[[p, 8 + p, 16 + p, 24 + p]] = 0
        tiles.append(t)
    t = np.full(32, 5); t[8:16] = 0; tiles.append(t)     # a whole group of empty rows
    tiles.append(np.zeros(32, np.int64))                 # a whole empty tile
    t = np.full(32, 2); t[13] = 200; tiles.append(t)     # one hub row longer than several batches beside short rows
    tiles.append(np.array([2] * 7 + [1] + [2] * 8 + [2] * 7 + [3] + [4] * 8))      # group totals of exactly 15, 16, 17 and 32 entries
    t = np.ones(32, np.int64); t[0] = 40; tiles.append(t)                           # the balanced split gives one group a single row
    t = np.ones(32, np.int64); t[31] = 40; tiles.append(t)                          # ... the last one
    tiles.append(np.full(32, 2))                                                     # balanced groups of exactly 16 slots: one full batch
    tiles.append(np.array([2] * 7 + [3] + [2] * 16 + [3] + [2] * 7))                 # balanced groups of 17, 16, 16, 17: one slot into the second batch
    return np.concatenate(tiles)


def decode(hdr, ent):
    """Per tile: (rows of every group in order of appearance, {row: [(source, weight bits)]}, slots of the longest group, slots in
    use per group); checks the layout rules on the way."""
    out = []
    for t in range(hdr.shape[0]):
        first, nb = int(hdr[t, 0]), int(hdr[t, 1])
        assert nb >= 1 and (t == 0 or first == hdr[t - 1, 0] + hdr[t - 1, 1])
        rows_of, seqs, used = [], {}, []
        for g in range(4):
            stream = ent[first:first + nb, 16 * g:16 * g + 16].reshape(-1, 2)
            words, wbits = stream[:, 0], stream[:, 1]
            ends = np.flatnonzero(words & ROW_END)
            last = int(ends[-1]) if ends.size else -1
            # padding: behind the group's last row end, no source, no row end, weight +0
            assert np.all(words[last + 1:] == NOROW) and np.all(wbits[last + 1:] == 0)
            rows, cur, cur_row = [], [], None
            for word, wb in zip(words[:last + 1], wbits[:last + 1]):
                r = int(word & 31)
                assert cur_row in (None, r)              # every entry carries the tile-local row it belongs to
                cur_row = None if word & ROW_END else r
                if (word & NOROW) == NOROW:              # the single entry of an empty row
                    assert word & ROW_END and not cur and wb == 0
                else:
                    cur.append((int(word >> 8), int(wb)))
                if word & ROW_END:
                    assert r not in seqs
                    seqs[r] = cur
                    rows.append(r)
                    cur = []
            assert not cur
            rows_of.append(rows)
            used.append(last + 1)
        assert 16 * (nb - 1) < max(used) <= 16 * nb     # no batch more than the longest group needs
        out.append((rows_of, seqs, max(used), used))
    return out


def best_split(slots):
    """Smallest largest-group sum over all splits of the 32 rows into four contiguous (possibly empty) ranges."""
    c = np.concatenate([[0], np.cumsum(slots)])
    return min(max(c[a] - c[0], c[b] - c[a], c[d] - c[b], c[32] - c[d])
               for a, b, d in itertools.combinations_with_replacement(range(33), 3))


@pytest.mark.parametrize('kind', ['hand', 'random', 'skewed'])
def test_program_is_the_csr_in_consumption_order(kind):
    e = _engine()
    rng = np.random.default_rng({'hand': 1, 'random': 2, 'skewed': 3}[kind])
    if kind == 'hand': deg = hand_built_degrees()
    elif kind == 'random': deg = rng.poisson(10.0, 32 * 9 + 7)                   # 7 rows of a partial last tile: not in the program
    else: deg = np.minimum(400, (rng.pareto(1.2, 32 * 12) * 3).astype(np.int64))
    indptr, src, w = csr_from_degrees(rng, deg, 512)
    hdr, ent = e.gather_program(indptr, src, w)
    tiles = deg.size // 32
    assert hdr.shape == (tiles, 2) and ent.shape == (int(hdr[:, 1].sum()), 64, 2)
    wbits = w.view(np.uint32)
    decoded = decode(hdr, ent)
    if kind == 'hand':      # the last two hand-built tiles sit on the batch boundary of the loader that reads the program
        assert decoded[-2][3] == [16, 16, 16, 16] and hdr[-2, 1] == 1 and decoded[-1][3] == [17, 16, 16, 17] and hdr[-1, 1] == 2
    for t, (rows_of, seqs, longest, _) in enumerate(decoded):
        # group ranges are contiguous, in order, and cover the 32 rows
        assert [r for rows in rows_of for r in rows] == list(range(32))
        for r in range(32):
            lo, hi = indptr[32 * t + r], indptr[32 * t + r + 1]
            assert seqs[r] == list(zip(src[lo:hi].tolist(), wbits[lo:hi].tolist())), (t, r)
        slots = np.maximum(1, deg[32 * t:32 * t + 32])
        assert longest == best_split(slots), (t, longest)


def test_program_rejects_what_it_cannot_encode():
    e = _engine()
    indptr = np.arange(33, dtype=np.int32)
    w = np.ones(32, np.float32)
    src = np.zeros(32, np.int32)
    src[5] = 1 << 23                                     # (source << 8) would leave the 2 GiB a replica may have
    with pytest.raises(NotImplementedError):
        e.gather_program(indptr, src, w)
    src[5] = (1 << 23) - 1
    hdr, ent = e.gather_program(indptr, src, w)
    assert hdr.tolist() == [[0, 1]] and int(ent[0, 5, 0]) == (((1 << 23) - 1) << 8 | ROW_END | 5)
    hdr, ent = e.gather_program(np.zeros(20, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))      # no full tile: an empty program
    assert hdr.shape == (0, 2) and ent.shape == (0, 64, 2)
