"""CPU side of vocabulary coverage: the numpy restatement of tests/coverage_reference.py against hand-written cases and its own
invariants, the C ABI of ``wgnn_coverage_rows`` without a GPU, and the host methods of ``api.Coverage`` on a hand-built one."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from scdeepsort_amd import _lib, api

import coverage_reference as V

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = np.float32(np.nan), np.float32(np.inf)


# ------------------------------------------------------------------------------------------------
# 1. the restatement
# ------------------------------------------------------------------------------------------------
# columns:            0      1 (foreign)  2      3      4
GENE_MAP = np.array([2, -1, 0, 4, 1], np.int32)
X = np.array([[1.5, 2.0, -0.0, 0.0, 4.0],          # one foreign count; a -0.0 is a zero
              [NAN, 3.0, -1.0, INF, 0.25],         # a NaN, a negative and an inf: bad, in nothing else
              [0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
WANT = dict(n_expressed=[3, 2, 0], n_mapped=[2, 1, 0], n_bad=[0, 3, 0], total=[7.5, 3.25, 0.0], total_mapped=[5.5, 0.25, 0.0],
            col_cells=[1, 2, 0, 0, 2])


def _check_hand_case(out):
    for f, want in WANT.items():
        got = getattr(out, f)
        assert got.dtype == (np.float64 if f.startswith("total") else np.int32), f
        np.testing.assert_array_equal(got, np.asarray(want), err_msg=f)


def test_reference_on_the_hand_written_dense_case():
    assert np.signbit(X[0, 2]) and GENE_MAP[1] == -1
    _check_hand_case(V.coverage_dense(X, GENE_MAP))


def test_reference_on_the_hand_written_csr_case():
    rowptr, col, val = V.to_csr(X)                               # stores the -0.0, the NaN, the negative and the inf
    assert rowptr.tolist() == [0, 4, 9, 9] and np.isnan(val).any() and np.isinf(val).any() and (val < 0).any()
    assert any(v == 0 and np.signbit(v) for v in val)
    _check_hand_case(V.coverage_csr(rowptr, col, val, GENE_MAP))


def test_reference_bad_value_on_a_foreign_column():
    x = np.array([[2.0, -3.0, 1.0], [0.0, INF, 0.0], [1.0, NAN, 1.0]], np.float32)
    out = V.coverage_dense(x, np.array([0, -1, 1], np.int32))
    assert out.n_bad.tolist() == [1, 1, 1] and out.n_expressed.tolist() == [2, 0, 2] and out.n_mapped.tolist() == [2, 0, 2]
    assert out.total.tolist() == [3.0, 0.0, 2.0] and out.total_mapped.tolist() == [3.0, 0.0, 2.0]
    assert out.col_cells.tolist() == [2, 0, 2]


def test_reference_invariants_on_a_random_case():
    c = V.count_case(11, 37, 130, 100, 0.0)
    mapped = c.gene_map >= 0
    for out in (V.coverage_dense(c.x, c.gene_map), V.coverage_csr(*V.to_csr(c.x), c.gene_map)):
        assert out.col_cells.sum() == out.n_expressed.sum() > 0
        assert out.col_cells[mapped].sum() == out.n_mapped.sum() > 0
        assert (out.total_mapped <= out.total).all() and (out.n_mapped <= out.n_expressed).all()
        assert (out.total_mapped < out.total).any()                                        # foreign columns hold counts
        np.testing.assert_array_equal(out.n_expressed, (c.x > 0).sum(1))
        np.testing.assert_array_equal(out.total, np.where(c.x > 0, c.x, 0).astype(np.float64).sum(1))
        np.testing.assert_array_equal(out.col_cells, (c.x > 0).sum(0))
    a, b = V.coverage_dense(c.x, c.gene_map), V.coverage_csr(*V.to_csr(c.x), c.gene_map)
    for g, w in zip(V.as_tuple(a), V.as_tuple(b)):
        np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------------------------------------
# 2. the ABI
# ------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    assert re.search(r"\bwgnn_coverage_rows\s*\(", text), "wgnn_coverage_rows is not declared in wgnn.h"
    assert hasattr(lib, "wgnn_coverage_rows") and "wgnn_coverage_rows" in _lib.SIGNATURES
    assert lib.wgnn_version() == 206
    from scdeepsort_amd import build
    assert "wgnn_coverage.hip" in {p.name for p in build.SRC}
    import scdeepsort_amd as sda
    assert sda.Coverage is api.Coverage and callable(sda.coverage_rows)


def test_bad_arguments_return_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)          # fake, aligned, never dereferenced: validation happens first
    BAD_ARG, ALIGNMENT = -1, -2

    def run(x=one, ld=8, rowptr=None, col=None, val=None, B=4, n_cols=8, gmap=one, G=5, n_expressed=one, n_mapped=one, n_bad=one,
            total=one, total_mapped=one, col_cells=one, status=one, flags=0):
        return lib.wgnn_coverage_rows(x, ld, rowptr, col, val, B, n_cols, gmap, G, n_expressed, n_mapped, n_bad, total,
                                      total_mapped, col_cells, status, flags, None)

    def detail(rc):
        return lib.wgnn_last_error_string(rc).decode()

    assert run(status=None) == BAD_ARG and "wgnn_coverage_rows: status is required" in detail(BAD_ARG)
    assert "wgnn_coverage_rows" not in detail(BAD_ARG)                                     # the detail is handed out once
    assert run(rowptr=one) == BAD_ARG and "either x (dense) or rowptr" in detail(BAD_ARG)  # both forms
    assert run(x=None) == BAD_ARG and "either x (dense) or rowptr" in detail(BAD_ARG)      # neither, with columns
    assert run(ld=7) == BAD_ARG and "ld must be >= n_cols" in detail(BAD_ARG)
    assert run(flags=_lib.FLAG_ROWPTR_I64) == BAD_ARG and "CSR form" in detail(BAD_ARG)    # dense with the CSR flag
    assert run(flags=1) == BAD_ARG and "WGNN_FLAG_ROWPTR_I64" in detail(BAD_ARG)
    assert run(total=C.c_void_p(20)) == ALIGNMENT and "8-byte" in detail(ALIGNMENT)
    assert run(total_mapped=C.c_void_p(20)) == ALIGNMENT and "8-byte" in detail(ALIGNMENT)
    assert run(B=-1) == BAD_ARG and "n_rows" in detail(BAD_ARG)
    assert run(B=2 ** 31) == BAD_ARG and "n_rows" in detail(BAD_ARG)
    assert run(n_cols=-1) == BAD_ARG and "n_cols" in detail(BAD_ARG)
    assert run(G=0) == BAD_ARG and "n_genes" in detail(BAD_ARG)
    assert run(gmap=None) == BAD_ARG and "gene_map" in detail(BAD_ARG)
    for missing in ("n_expressed", "n_mapped", "n_bad", "total", "total_mapped"):
        assert run(**{missing: None}) == BAD_ARG and "are required" in detail(BAD_ARG), missing
    assert run(col_cells=None) == BAD_ARG and "col_cells" in detail(BAD_ARG)
    assert run(x=C.c_void_p(18)) == ALIGNMENT and "4-byte" in detail(ALIGNMENT)
    assert run(n_mapped=C.c_void_p(18)) == ALIGNMENT and "4-byte" in detail(ALIGNMENT)
    # an empty batch without columns is valid and touches nothing
    assert run(B=0, n_cols=0, x=None, gmap=None, ld=0, col_cells=None) == 0
    assert run(B=0, n_cols=0, x=None, rowptr=one, gmap=None, ld=0, col_cells=None, flags=_lib.FLAG_ROWPTR_I64) == 0


# ------------------------------------------------------------------------------------------------
# 3. Coverage's host methods
# ------------------------------------------------------------------------------------------------
def _hand_built():
    #  columns   A(bundle 0)  x   B(bundle 2)  y   z   w       cells c0..c3
    return api.Coverage(
        n_columns=6, n_matched=2, n_bundle_genes=5, n_bundle_absent=3,
        n_expressed=np.array([4, 0, 2, 3], np.int32), n_mapped=np.array([2, 0, 0, 1], np.int32),
        n_bad=np.array([0, 2, 0, 1], np.int32), total=np.array([10.0, 0.0, 4.0, 8.0]), total_mapped=np.array([7.5, 0.0, 0.0, 2.0]),
        col_cells=torch.tensor([2, 3, 1, 1, 3, 0], dtype=torch.int32), index=pd.Index(["c0", "c1", "c2", "c3"]),
        columns=["A", "x", "B", "y", "z", "w"], matched=np.array([True, False, True, False, False, False]),
        absent_ids=np.array([1, 3, 4]), absent_support_cells=np.array([5, 9, 9]), absent_names=["G1", "G3", "G4"],
        n_support_cells=10)


def test_fractions_with_zero_rows():
    cov = _hand_built()
    np.testing.assert_array_equal(cov.fraction_counts(), [0.75, 0.0, 0.0, 0.25])           # c1: total 0 -> 0, no warning, no NaN
    np.testing.assert_array_equal(cov.fraction_genes(), [0.5, 0.0, 0.0, 1 / 3])
    f = cov.frame()
    assert list(f.index) == ["c0", "c1", "c2", "c3"]
    assert list(f.columns) == ["n_expressed", "n_mapped", "n_bad", "total", "total_mapped", "fraction_counts", "fraction_genes"]
    np.testing.assert_array_equal(f["fraction_counts"].to_numpy(), cov.fraction_counts())
    np.testing.assert_array_equal(f["n_bad"].to_numpy(), [0, 2, 0, 1])


def test_unmatched_orders_by_cells_then_position():
    cov = _hand_built()
    u = cov.unmatched()
    assert list(u.columns) == ["position", "gene", "cells", "fraction_of_cells"]
    assert u["position"].tolist() == [1, 4, 3, 5] and u["gene"].tolist() == ["x", "z", "y", "w"]      # 3, 3 (tie: lower first), 1, 0
    assert u["cells"].tolist() == [3, 3, 1, 0] and u["fraction_of_cells"].tolist() == [0.75, 0.75, 0.25, 0.0]
    assert cov.unmatched(k=2)["gene"].tolist() == ["x", "z"]
    cov.columns = None                                                                     # a gene map was passed: no names
    assert list(cov.unmatched().columns) == ["position", "cells", "fraction_of_cells"]


def test_absent_orders_by_support_cells_then_gene_id():
    a = _hand_built().absent()
    assert a["gene_id"].tolist() == [3, 4, 1] and a["gene"].tolist() == ["G3", "G4", "G1"]
    assert a["support_cells"].tolist() == [9, 9, 5] and a["fraction_of_support"].tolist() == [0.9, 0.9, 0.5]
    assert _hand_built().absent(k=1)["gene"].tolist() == ["G3"]


def test_below():
    cov = _hand_built()
    assert cov.below().tolist() == [False, True, True, True]                               # fraction_counts < 0.5
    assert cov.below(min_counts=0.2).tolist() == [False, True, True, False]
    assert cov.below(min_counts=0.0).tolist() == [False, False, False, False]
    assert cov.below(min_counts=0.0, min_genes=2).tolist() == [False, True, True, True]   # n_mapped < 2
    assert cov.below(min_counts=0.8, min_genes=0).tolist() == [True, True, True, True]


def test_summary():
    s = _hand_built().summary()
    assert isinstance(s, dict)
    assert (s["n_columns"], s["n_matched"], s["n_bundle_genes"], s["n_bundle_absent"], s["n_cells"]) == (6, 2, 5, 3, 4)
    assert s["median_fraction_counts"] == 0.125 and s["min_fraction_counts"] == 0.0
    assert s["median_fraction_genes"] == 1 / 6 and s["min_fraction_genes"] == 0.0
    assert s["n_cells_below"] == 3 and s["n_bad"] == 3
    text = str(s)
    assert 2 <= len(text.splitlines()) <= 3
    assert "2 of 6 columns" in text and "3 of its 5 genes are absent" in text and "3 cells below" in text and "3 values" in text
    cov = _hand_built()
    cov.n_bad[:] = 0
    assert len(str(cov.summary()).splitlines()) == 2
