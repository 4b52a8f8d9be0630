"""tests/hood_reference.py on hand-worked units, what its cases hold, and ``api._neighbor_lists`` - the host half of
``ResidentPredictor.smooth`` - on both forms of a neighbour graph.  No GPU."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from scdeepsort_amd import api

import hood_reference as H


def _f32(x):
    return np.float32(x)


def test_hand_worked_units():
    # three cells over five genes: cell 0 holds genes 1 and 3, cell 1 genes 3 and 4 (unsorted), cell 2 nothing
    rowptr = np.array([0, 2, 4, 4])
    col = np.array([1, 3, 4, 3], np.int32)
    cnt = np.array([2, 5, 1, 3], np.float32)
    lib = np.array([10, 4, 0], np.int64)               # cell 0 has 3 reads outside the bundle
    ptr, members = H.lists([[], [0], [0, 1], [1, 0], [0, 0], [2]])
    out = H.hood_rows(rowptr, col, cnt, lib, ptr, members, 0.0)
    assert out.rowptr.tolist() == [0, 0, 2, 5, 8, 10, 10] and out.total.tolist() == [0, 10, 14, 14, 20, 0]
    assert out.col.tolist() == [1, 3, 1, 3, 4, 1, 3, 4, 1, 3] and out.cnt.tolist() == [2, 5, 2, 8, 1, 2, 8, 1, 4, 10]
    v = lambda c, total: _f32(math.log1p(c / total * 1e4))
    want = [v(2, 10), v(5, 10), v(2, 14), v(8, 14), v(1, 14), v(2, 14), v(8, 14), v(1, 14), v(4, 20), v(10, 20)]
    assert out.val.dtype == np.float32 and out.val.tolist() == want
    assert out.val[8] == out.val[0] and out.val[9] == out.val[1]       # a cell pooled with itself: the same shares
    # the threshold is strict and compares the float32 value
    edge = float(v(2, 14))
    assert H.hood_rows(rowptr, col, cnt, lib, ptr, members, edge).col.tolist() == [1, 3, 3, 3, 1, 3]      # v(2, 14) itself is dropped
    # a pooled count above 2^24 enters the logarithm as it is, not through a float32
    big = H.hood_rows(np.array([0, 1, 2]), np.array([0, 0], np.int32), np.array([2.0 ** 23, 1.0], np.float32),
                      np.array([2 ** 40, 0], np.int64), *H.lists([[0, 0, 1]]), 0.0)
    assert big.cnt.tolist() == [2 ** 24 + 1] and big.total.tolist() == [2 ** 41]
    assert np.float32(2 ** 24 + 1) == 2 ** 24 and big.v64[0] == math.log1p((2 ** 24 + 1) / 2 ** 41 * 1e4)
    assert big.v64[0] != math.log1p(2 ** 24 / 2 ** 41 * 1e4)


def test_the_cases_hold_what_they_name_and_no_value_is_fragile():
    m = H.batch()
    assert m.B == 40 and m.G == 300 and len(m.lib) == 40 and m.col.max() == 299
    lens = np.diff(m.rowptr)
    assert lens[H.ROW_EMPTY] == lens[H.ROW_EMPTY_READS] == 0 and m.lib[H.ROW_EMPTY] == 0 and m.lib[H.ROW_EMPTY_READS] == 7
    assert lens[H.ROW_ONE] == 1 and lens[H.ROW_ALL] == 300 and lens[H.ROW_65] == 65 and (m.rest > 0).sum() > 5
    assert all((np.diff(m.col[m.rowptr[r]:m.rowptr[r + 1]]) > 0).all() for r in range(m.B))          # strictly ascending rows
    assert m.cnt.min() >= 1 and m.cnt.max() == 2.0 ** 23 and (m.cnt == np.round(m.cnt)).all()
    units = H.units()
    sizes = [len(u) for u in units]
    assert sizes[H.UNIT_NONE] == 0 and sizes[H.UNIT_ONE] == 1 and sizes[H.UNIT_PAIR] == 2 and sizes[H.UNIT_ALL] == 40
    assert sizes[H.UNIT_256] == sizes[H.UNIT_255_AND_ONE] == 256 == H.MAX_MEMBERS
    ragged = sizes[H.UNIT_RAGGED:]
    assert len(ragged) == H.N_RAGGED and min(ragged) == 0 and max(ragged) == 9 and len(set(ragged)) > 4
    assert len(set(units[H.UNIT_TWICE])) < len(units[H.UNIT_TWICE])
    for thr in H.THRESHOLDS:
        c = H.case(thr)
        ref = c.ref
        kept = np.diff(ref.rowptr)
        assert kept[H.UNIT_NONE] == kept[H.UNIT_EMPTY_ROWS] == kept[H.UNIT_FOREIGN_ONLY] == 0
        assert ref.total[H.UNIT_NONE] == 0 and ref.total[H.UNIT_EMPTY_ROWS] == 7 and ref.total[H.UNIT_FOREIGN_ONLY] == 7
        row = lambda q: slice(ref.rowptr[q], ref.rowptr[q + 1])
        at = lambda q: ref.cnt[row(q)][list(ref.col[row(q)]).index(H.BIG_GENE)]
        assert at(H.UNIT_256) == 2 ** 31 and at(H.UNIT_255_AND_ONE) == 255 * 2 ** 23 + 1 > 2 ** 24          # the counter's limit
        assert np.float32(at(H.UNIT_255_AND_ONE)) != at(H.UNIT_255_AND_ONE)
        assert not H.fragile(ref.v64).any()            # so a comparison of the float32 bits with this file is decided
        assert (ref.val > np.float32(thr)).all()
    loose, strict = H.case(0.0).ref, H.case(1.5).ref
    assert 0 < strict.rowptr[-1] < loose.rowptr[-1]                    # the positive threshold drops entries, and keeps some
    assert loose.rowptr[H.UNIT_ALL + 1] - loose.rowptr[H.UNIT_ALL] == 300
    assert loose.col[-1] == 299 and units[-1][-1] == H.ROW_LAST_GENE   # the last unit fills the last slot of the output
    assert all(len(set(u)) == len(u) for u in units[H.UNIT_RAGGED:])
    # every slab of 128 genes holds kept entries of the ragged units: the sweep's slots carry over from slab to slab
    for lo in (0, 128, 256):
        seg = loose.col[loose.rowptr[H.UNIT_RAGGED + 1]:loose.rowptr[H.UNIT_RAGGED + 2]]
        assert ((seg >= lo) & (seg < lo + 128)).any()


def test_neighbor_lists_from_an_index_array():
    nb = np.array([[1, 2, -1], [-1, -1, -1], [2, 0, 3], [-1, 1, -1]])
    ptr, members = api._neighbor_lists(nb, 4, include_self=True)
    assert ptr.dtype == np.int64 and members.dtype == np.int32
    assert ptr.tolist() == [0, 3, 4, 7, 9] and members.tolist() == [0, 1, 2, 1, 2, 0, 3, 3, 1]       # the cell first, its own entry dropped
    ptr, members = api._neighbor_lists(nb, 4, include_self=False)
    assert ptr.tolist() == [0, 2, 2, 4, 5] and members.tolist() == [1, 2, 0, 3, 1]                    # cell 1: the empty unit
    for form in (torch.from_numpy(nb), nb.astype(np.int32), nb.tolist()):
        again = api._neighbor_lists(form, 4, include_self=False)
        assert again[0].tolist() == ptr.tolist() and again[1].tolist() == members.tolist()
    none = api._neighbor_lists(np.zeros((3, 0), np.int64), 3, True)
    assert none[0].tolist() == [0, 1, 2, 3] and none[1].tolist() == [0, 1, 2]
    assert api._neighbor_lists(np.zeros((0, 4), np.int64), 0, True)[0].tolist() == [0]
    with pytest.raises(ValueError, match="cell 2 lists the neighbour 0 twice"):
        api._neighbor_lists(np.array([[1, 2], [0, 2], [0, 0]]), 3)
    with pytest.raises(ValueError, match="cell 1 lists the index 3, outside"):
        api._neighbor_lists(np.array([[1, 2], [3, 2], [0, 1]]), 3)
    with pytest.raises(ValueError, match="cell 0 lists the index -2"):
        api._neighbor_lists(np.array([[-2, 2], [0, 2], [0, 1]]), 3)
    for bad in (np.zeros((3, 2)), np.zeros(3, np.int64), np.zeros((4, 2), np.int64)):          # floats, a vector, another B
        with pytest.raises(ValueError, match="neighbors"):
            api._neighbor_lists(bad, 3)
    # 255 neighbours are a unit of 256 with the cell itself; 256 are too many, with or without it
    wide = np.tile(np.arange(1, 257), (300, 1))
    wide[1:] = -1
    ptr, members = api._neighbor_lists(wide[:, :255], 300)
    assert ptr[1] == 256 and members[:256].tolist() == list(range(256))
    for include_self in (True, False):
        with pytest.raises(ValueError, match="cell 0 lists 256 neighbours"):
            api._neighbor_lists(wide, 300, include_self)
    wide[0, 0] = 0                                                     # ... unless one of them is the cell itself
    assert api._neighbor_lists(wide, 300)[0][1] == 256


def test_neighbor_lists_from_a_sparse_matrix():
    dense = np.array([[0.7, 0.2, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 1.0, 0.1], [0.0, -3.0, 0.0, 0.0]])
    want_self = ([0, 2, 3, 6, 8], [0, 1, 1, 2, 0, 3, 3, 1])
    want_none = ([0, 1, 1, 3, 4], [1, 0, 3, 1])
    for form in (sp.csr_matrix(dense), sp.coo_matrix(dense), sp.csc_matrix(dense), sp.lil_matrix(dense)):
        for include_self, want in ((True, want_self), (False, want_none)):
            ptr, members = api._neighbor_lists(form, 4, include_self)
            assert ptr.tolist() == want[0] and members.tolist() == want[1] and members.dtype == np.int32
    stored = sp.csr_matrix(dense)
    stored.data[1] = 0.0                                               # a stored zero is no neighbour
    assert api._neighbor_lists(stored, 4, False)[1].tolist() == [0, 3, 1]
    assert stored.nnz == 6                                             # the caller's matrix is left as it was
    twice = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))          # COO duplicates are one entry
    assert api._neighbor_lists(twice, 2, False)[1].tolist() == [1, 0]
    with pytest.raises(ValueError, match="the batch holds 5 cells"):
        api._neighbor_lists(sp.csr_matrix(dense), 5)
    with pytest.raises(ValueError, match="cell 0 lists 256 neighbours"):
        api._neighbor_lists(sp.csr_matrix(np.ones((257, 257))), 257)
    # the two forms of one graph agree
    rng = np.random.default_rng(0)
    nb = np.full((30, 6), -1)
    for i in range(30):
        k = int(rng.integers(0, 7))
        nb[i, :k] = np.sort(rng.choice(30, size=k, replace=False))
    a = sp.lil_matrix((30, 30))
    for i in range(30):
        for j in nb[i][nb[i] >= 0]:
            a[i, j] = 1.0
    for include_self in (True, False):
        x, y = api._neighbor_lists(nb, 30, include_self), api._neighbor_lists(a.tocsr(), 30, include_self)
        assert x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist()
