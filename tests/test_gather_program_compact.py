"""The gather program's compact format (gnn_gather_program_compact, host code): 4-byte entries - the source words of the 8-byte program,
unchanged - and one weight per tile-local row.  From words and row weights alone every row's (source, weight bits) sequence is the CSR's;
an empty row carries +0; a row whose entries differ in their weights' bit patterns makes the program not compactable."""
import numpy as np
import pytest

from test_gather_program import csr_from_degrees, hand_built_degrees

ROW_END, NOROW = 32, 0xfffffe00


def _engine():
    from GNN import _engine
    return _engine


def uniform_csr(rng, deg, n_src):
    """csr_from_degrees with 'average'-style weights: 1 / degree on every entry of a row."""
    indptr, src, _ = csr_from_degrees(rng, deg, n_src)
    d = np.asarray(deg, np.int64)
    w = (1.0 / np.repeat(d, d)).astype(np.float32)
    return indptr, src, w


def rows_from_compact(hdr, words, roww):
    """{(tile, row): [(source, weight bits)]} rebuilt from the compact program; an empty row maps to []."""
    wbits = roww.view(np.uint32)
    seqs = {}
    for t in range(hdr.shape[0]):
        first, nb = int(hdr[t, 0]), int(hdr[t, 1])
        for g in range(4):
            stream = words[first:first + nb, 16 * g:16 * g + 16].reshape(-1)
            cur = []
            for word in stream:
                word = int(word)
                if word == NOROW: continue                       # padding
                r = word & 31
                if (word & NOROW) != NOROW: cur.append((word >> 8, int(wbits[t, r])))
                if word & ROW_END:
                    assert (t, r) not in seqs
                    seqs[(t, r)] = cur
                    cur = []
            assert not cur
    return seqs


@pytest.mark.parametrize('kind', ['hand', 'skewed'])
def test_compact_program_is_the_csr(kind):
    e = _engine()
    rng = np.random.default_rng({'hand': 1, 'skewed': 3}[kind])
    deg = hand_built_degrees() if kind == 'hand' else np.minimum(400, (rng.pareto(1.2, 32 * 12) * 3).astype(np.int64))
    indptr, src, w = uniform_csr(rng, deg, 512)
    hdr, ent = e.gather_program(indptr, src, w)
    words, roww = e.gather_program_compact(hdr, ent)
    tiles = deg.size // 32
    assert words.shape == ent.shape[:2] and words.dtype == np.uint32 and roww.shape == (tiles, 32) and roww.dtype == np.float32
    assert np.array_equal(words, ent[:, :, 0])                  # every source word unchanged: row ends, rows, empty rows' entries, padding
    assert np.any(words == NOROW)                               # (the case has padding)
    wb = w.view(np.uint32)
    seqs = rows_from_compact(hdr, words, roww)
    assert len(seqs) == 32 * tiles
    for t in range(tiles):
        for r in range(32):
            lo, hi = indptr[32 * t + r], indptr[32 * t + r + 1]
            assert seqs[(t, r)] == list(zip(src[lo:hi].tolist(), wb[lo:hi].tolist())), (t, r)
            if lo == hi: assert roww.view(np.uint32)[t, r] == 0                     # an empty row: +0, sign bit included
    assert np.any(deg[:32 * tiles] == 0)


def test_one_row_with_two_weights_is_refused():
    e = _engine()
    rng = np.random.default_rng(5)
    deg = rng.integers(1, 9, 96)
    deg[40] = 4
    indptr, src, w = uniform_csr(rng, deg, 512)
    hdr, ent = e.gather_program(indptr, src, w)
    e.gather_program_compact(hdr, ent)                           # uniform: compactable
    w2 = w.copy()
    w2[indptr[40] + 2] = np.nextafter(w2[indptr[40] + 2], np.float32(1.0))      # one entry of one row, one ulp
    hdr, ent = e.gather_program(indptr, src, w2)
    with pytest.raises(NotImplementedError):
        e.gather_program_compact(hdr, ent)


def test_positive_and_negative_zero_in_one_row_are_refused():
    e = _engine()
    rng = np.random.default_rng(6)
    deg = np.full(32, 3)
    indptr, src, w = uniform_csr(rng, deg, 64)
    w[indptr[7]:indptr[8]] = 0.0
    hdr, ent = e.gather_program(indptr, src, w)
    words, roww = e.gather_program_compact(hdr, ent)             # a row of +0 weights is uniform
    assert roww.view(np.uint32)[0, 7] == 0
    w[indptr[7] + 1] = -0.0
    hdr, ent = e.gather_program(indptr, src, w)
    with pytest.raises(NotImplementedError):
        e.gather_program_compact(hdr, ent)
    w[indptr[7]:indptr[8]] = -0.0                                # all -0: uniform again, and kept as -0
    hdr, ent = e.gather_program(indptr, src, w)
    words, roww = e.gather_program_compact(hdr, ent)
    assert roww.view(np.uint32)[0, 7] == 0x80000000


def test_empty_program_compacts_to_empty_arrays():
    e = _engine()
    hdr, ent = e.gather_program(np.zeros(20, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))      # no full tile
    words, roww = e.gather_program_compact(hdr, ent)
    assert words.shape == (0, 64) and roww.shape == (0, 32)
