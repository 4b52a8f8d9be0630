"""The numpy restatement of log-normalising alignment (tests/lognorm_reference.py) against hand-derived vectors, and the argument
checks of the Python layers that need no GPU."""
import math

import numpy as np
import pytest
import torch

import scdeepsort_amd as sda
from scdeepsort_amd import api, ops

import lognorm_reference as L
from align_reference import bits


def f32(*v):
    return np.asarray(v, np.float64).astype(np.float32)


def test_hand_vector():
    # total 10, scale 10: v = log1p(x) = ln 2, ln 4, -, ln 7
    rowptr, col, v = L.lognorm_dense([[1, 3, 0, 6]], [5, 2, 7, 0], 0.0, scale=10)
    assert rowptr.tolist() == [0, 3] and col.tolist() == [5, 2, 0]
    np.testing.assert_array_equal(bits(v), bits(f32(math.log(2), math.log(4), math.log(7))))
    # a threshold between ln 2 and ln 4
    rowptr, col, v = L.lognorm_dense([[1, 3, 0, 6]], [5, 2, 7, 0], 1.0, scale=10)
    assert rowptr.tolist() == [0, 2] and col.tolist() == [2, 0]
    # Seurat's defaults: 2 of 8 counts -> log1p(2500)
    _, _, v = L.lognorm_dense([[2, 6]], [0, 1], 0.0)
    np.testing.assert_array_equal(bits(v), bits(f32(math.log1p(2500.0), math.log1p(7500.0))))


def test_foreign_column_counts_in_the_total_only():
    # the 10 of the foreign column doubles the total: v = log1p(x / 20 * 10)
    rowptr, col, v = L.lognorm_dense([[1, 3, 10, 6]], [5, 2, -1, 0], 0.0, scale=10)
    assert col.tolist() == [5, 2, 0]
    np.testing.assert_array_equal(bits(v), bits(f32(math.log1p(0.5), math.log1p(1.5), math.log1p(3.0))))
    # aligning first and normalising second is another result
    _, _, other = L.lognorm_dense([[1, 3, 6]], [5, 2, 0], 0.0, scale=10)
    assert not np.array_equal(v, other)


def test_zero_rows_and_zero_entries():
    rowptr, col, v = L.lognorm_dense([[0, 0, 0], [0, 4, 0], [0, 0, 5]], [1, -1, 0], 0.0)
    assert rowptr.tolist() == [0, 0, 0, 1] and col.tolist() == [0]            # all-zero row; foreign-only row; one entry
    np.testing.assert_array_equal(bits(v), bits(f32(math.log1p(1e4))))
    rowptr, _, _ = L.lognorm_dense([[-0.0, 2.0]], [0, 1], 0.0)                 # a -0.0 is a zero: not kept, not an error
    assert rowptr.tolist() == [0, 1]
    _, _, v = L.lognorm_dense([[0.5, 1.5]], [0, 1], 0.0, scale=2)              # counts need not be integers
    np.testing.assert_array_equal(bits(v), bits(f32(math.log1p(0.5), math.log1p(1.5))))


def test_library_size_overrides_the_total():
    x = [[1, 3, 0, 6], [0, 0, 0, 0]]
    _, col, v = L.lognorm_dense(x, [5, 2, 7, 0], 0.0, scale=10, library_size=[20.0, 0.0])     # row 1 holds nothing: its size is not read
    assert col.tolist() == [5, 2, 0]
    np.testing.assert_array_equal(bits(v), bits(f32(math.log1p(0.5), math.log1p(1.5), math.log1p(3.0))))
    np.testing.assert_array_equal(L.totals(x), [10.0, 0.0])
    same = L.lognorm_dense(x, [5, 2, 7, 0], 0.0, scale=10, library_size=L.totals(x))
    for a, b in zip(same, L.lognorm_dense(x, [5, 2, 7, 0], 0.0, scale=10)):
        np.testing.assert_array_equal(a, b)
    for size in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="library size"):
            L.lognorm_dense(x, [5, 2, 7, 0], 0.0, library_size=[size, 1.0])


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_counts_are_errors_on_any_column(bad):
    for j in (0, 1):                                                           # mapped, foreign
        x = np.array([[1, 1, 1]], np.float32); x[0, j] = bad
        with pytest.raises(ValueError, match="bad count"):
            L.lognorm_dense(x, [0, -1, 1], 0.0)
        with pytest.raises(ValueError, match="bad count"):
            L.lognorm_csr(*L.to_csr(x), [0, -1, 1], 0.0)


@pytest.mark.parametrize("thr", [0.0, 0.5])
def test_dense_and_csr_forms_agree(thr):
    c = L.count_case(7, 12, 130, 100, thr)
    cs = L.corners(c)
    assert cs.zero_row and cs.foreign_only_row and cs.one_big_among_ones and cs.total_beyond_2_24_odd and cs.neg_zero \
        and cs.fractions and cs.foreign_counts
    dense = L.lognorm_dense(c.x, c.gene_map, thr, fp64=True)
    sparse = L.lognorm_csr(*L.to_csr(c.x), c.gene_map, thr, fp64=True)
    for a, b in zip(dense, sparse):
        np.testing.assert_array_equal(a, b)
    assert dense[0][-1] > 100 and (np.diff(dense[0])[[L.ROW_ZERO, L.ROW_FOREIGN_ONLY]] == 0).all()


def test_fragile_marks_float32_midpoints_only():
    f = np.float32(1.2345)
    up = np.nextafter(f, np.float32(2))
    mid = (float(f) + float(up)) / 2
    ulp = np.spacing(mid)
    v = np.array([float(f), mid, mid + 10 * ulp, mid - 16 * ulp, mid + 40 * ulp, float(up)])
    assert L.fragile(v).tolist() == [False, True, True, True, False, False]


def test_argument_checks_need_no_gpu():
    x, gmap = torch.zeros((2, 3)), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="threshold = -0.5 must be >= 0"):
        ops.align_rows(x, gmap, 5, threshold=-0.5, normalize="lognorm")
    with pytest.raises(ValueError, match="threshold"):
        ops.align_rows(x, gmap, 5, threshold=float("nan"), normalize="lognorm")
    with pytest.raises(ValueError, match="normalize = 'log'"):
        ops.align_rows(x, gmap, 5, normalize="log")
    with pytest.raises(ValueError, match="scale"):
        ops.align_rows(x, gmap, 5, normalize="lognorm", scale=0.0)
    with pytest.raises(ValueError, match="library_size belongs"):
        ops.align_rows(x, gmap, 5, library_size=[1.0, 1.0])
    with pytest.raises(sda.WgnnError, match="GPU only"):                       # the unnormalised call still ends where it did
        ops.align_rows(x, gmap, 5)
    assert api._normalize_spec(None) is None
    assert api._normalize_spec("lognorm") == sda.LogNormalize() == sda.LogNormalize(scale_factor=1e4, library_size=None)
    spec = sda.LogNormalize(scale_factor=1e6)
    assert api._normalize_spec(spec) is spec
    for bad in ("cpm", True, 1e4):
        with pytest.raises(ValueError, match="normalize ="):
            api._normalize_spec(bad)
    assert ops._ALIGN_STATUS[-1][0] == 8
