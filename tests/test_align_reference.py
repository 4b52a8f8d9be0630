"""CPU side of batch alignment: the C ABI of ``wgnn_align_count`` / ``wgnn_align_fill`` without a GPU, the numpy restatement of
tests/align_reference.py against ``api._read_test_csr`` on a file in the reference's layout, the corners the GPU suite's cases
claim to hold, and the host logic behind ``ResidentPredictor.gene_map``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from scdeepsort_amd import _lib, api

import align_reference as A

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------
# 1. the ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wgnn.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for s in ("wgnn_align_count", "wgnn_align_fill"):
        assert re.search(rf"\b{s}\s*\(", text), f"{s} is not declared in wgnn.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    for name, value in (("BAD_COL", _lib.ALIGN_BAD_COL), ("BAD_MAP", _lib.ALIGN_BAD_MAP), ("BAD_ROWPTR", _lib.ALIGN_BAD_ROWPTR)):
        assert int(re.search(rf"#define\s+WGNN_ALIGN_{name}\s+(\d+)", text).group(1)) == value
    assert lib.wgnn_version() == 206
    from scdeepsort_amd import build
    assert "wgnn_align.hip" in {p.name for p in build.SRC}


def test_bad_arguments_return_error_codes_without_gpu():
    lib = _lib.lib()
    one = C.c_void_p(16)          # fake, aligned, never dereferenced: validation happens first
    BAD_ARG, ALIGNMENT = -1, -2

    def count(x=one, ld=8, rowptr=None, col=None, val=None, B=4, n_cols=8, gmap=one, G=5, counts=one, status=one, flags=0):
        return lib.wgnn_align_count(x, ld, rowptr, col, val, B, n_cols, gmap, G, 0.0, counts, status, flags, None)

    def fill(x=one, ld=8, rowptr=None, B=4, n_cols=8, gmap=one, G=5, out_rowptr=one, status=one, flags=0):
        return lib.wgnn_align_fill(x, ld, rowptr, one, one, B, n_cols, gmap, G, 0.0, out_rowptr, one, one, status, flags, None)

    def detail(rc):
        return lib.wgnn_last_error_string(rc).decode()

    assert count(status=None) == BAD_ARG and "wgnn_align_count: status is required" in detail(BAD_ARG)
    assert "wgnn_align" not in detail(BAD_ARG)                                               # the detail is handed out once
    assert count(B=-1) == BAD_ARG and "n_rows" in detail(BAD_ARG)
    assert count(B=2 ** 31) == BAD_ARG and "n_rows" in detail(BAD_ARG)
    assert count(n_cols=-1) == BAD_ARG and "n_cols" in detail(BAD_ARG)
    assert count(G=0) == BAD_ARG and "n_genes" in detail(BAD_ARG)
    assert count(flags=1) == BAD_ARG and "WGNN_FLAG_ROWPTR_I64" in detail(BAD_ARG)
    assert count(flags=_lib.FLAG_ROWPTR_I64) == BAD_ARG and "CSR form" in detail(BAD_ARG)     # dense with the CSR flag
    assert count(rowptr=one) == BAD_ARG and "either x (dense) or rowptr" in detail(BAD_ARG)   # both forms
    assert count(x=None) == BAD_ARG and "either x (dense) or rowptr" in detail(BAD_ARG)       # neither, with columns
    assert count(ld=7) == BAD_ARG and "ld must be >= n_cols" in detail(BAD_ARG)
    assert count(gmap=None) == BAD_ARG and "gene_map" in detail(BAD_ARG)
    assert count(counts=None) == BAD_ARG and "row_count" in detail(BAD_ARG)
    assert count(x=C.c_void_p(18)) == ALIGNMENT and "4-byte" in detail(ALIGNMENT)
    assert fill(out_rowptr=None) == BAD_ARG and "wgnn_align_fill: out_rowptr is required" in detail(BAD_ARG)
    assert fill(out_rowptr=C.c_void_p(20)) == ALIGNMENT and "8-byte" in detail(ALIGNMENT)
    assert fill(status=None) == BAD_ARG
    # an empty batch is valid and launches nothing, in both forms, also without columns
    assert count(B=0) == 0 and fill(B=0) == 0
    assert count(B=0, x=None, rowptr=one, flags=_lib.FLAG_ROWPTR_I64) == 0
    assert count(B=0, n_cols=0, x=None, gmap=None, ld=0) == 0


# ------------------------------------------------------------------------------------------------
# 2. the restatement against api._read_test_csr on a file in the reference's layout
# ------------------------------------------------------------------------------------------------
def _write_csv(path, x, names):
    """(genes x cells) as pre-process.R writes it: gene names down the first column, one column per cell."""
    pd.DataFrame(x.T, index=list(names), columns=[f"C{i}" for i in range(x.shape[0])]).to_csv(path)


def _file_case(rng, G=40, n_foreign=12, B=23):
    bundle = [f"Gene{i}" for i in range(G)]
    gene2id = {g: i for i, g in enumerate(bundle)}
    present = sorted(rng.choice(G, size=G - 7, replace=False).tolist())            # the file lacks 7 bundle genes
    names = [bundle[i] for i in present]
    for k in range(n_foreign):                                                     # foreign genes in between
        names.insert(int(rng.integers(len(names) + 1)), f"Other{k}")
    x = np.where(rng.random((B, len(names))) < 0.4, rng.uniform(0.1, 6.0, (B, len(names))), 0.0).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.float32(-1.25)                               # below every threshold
    x[3] = 0                                                                        # a cell with nothing
    x[rng.random(x.shape) < 0.05] = np.float32(0.5)                                 # exactly AT the threshold 0.5
    x[3] = 0
    return gene2id, names, x


@pytest.mark.parametrize("threshold", [0, 0.5])
def test_restatement_equals_read_test_csr(tmp_path, threshold):
    rng = np.random.default_rng(5)
    gene2id, names, x = _file_case(rng)
    f = tmp_path / "mouse_Test1_data.csv"
    _write_csv(f, x, names)
    want, index = api._read_test_csr(f, "csv", gene2id, threshold)
    gmap = api._gene_map_ids(names, gene2id)
    assert (gmap == -1).sum() == 12 and (np.diff(gmap[gmap >= 0]) > 0).all()       # bundle genes in the bundle's order
    rowptr, col, raw = A.align_dense(x, gmap, threshold)
    # exactly: indptr, indices in stored order, data
    np.testing.assert_array_equal(rowptr, want.indptr)
    np.testing.assert_array_equal(col, want.indices)
    np.testing.assert_array_equal(A.bits(raw), A.bits(want.data))
    assert want.shape == (x.shape[0], len(gene2id)) and list(index) == [f"C{i}" for i in range(x.shape[0])]
    assert rowptr[4] == rowptr[3] and (x[:, gmap < 0] > threshold).any() and (x == np.float32(0.5)).any() and (x < 0).any()
    # the CSR form over the caller's columns says the same
    got = A.align_csr(*A.dense_to_csr(x), gmap, threshold)
    for g, w in zip(got, (rowptr, col, raw)):
        np.testing.assert_array_equal(g, w)


def test_read_test_csr_orders_a_row_by_bundle_id_the_restatement_by_input(tmp_path):
    """With the file's genes in another order than the bundle's, ``_read_test_csr`` still lists a cell's genes by ascending
    bundle id (scipy's COO -> CSR), alignment in the caller's order: the same entries, row by row, in two orders."""
    rng = np.random.default_rng(6)
    gene2id, names, x = _file_case(rng)
    perm = rng.permutation(len(names))
    names, x = [names[i] for i in perm], np.ascontiguousarray(x[:, perm])
    f = tmp_path / "mouse_Test2_data.csv"
    _write_csv(f, x, names)
    want, _ = api._read_test_csr(f, "csv", gene2id, 0)
    rowptr, col, raw = A.align_dense(x, api._gene_map_ids(names, gene2id), 0)
    np.testing.assert_array_equal(rowptr, want.indptr)
    assert not np.array_equal(col, want.indices)
    for r in range(x.shape[0]):
        s = slice(rowptr[r], rowptr[r + 1])
        order = np.argsort(col[s], kind="stable")
        np.testing.assert_array_equal(col[s][order], want.indices[s])
        np.testing.assert_array_equal(A.bits(raw[s][order]), A.bits(want.data[s]))


def test_restatement_by_boolean_mask():
    """The loop against the one-line boolean-mask selection, on every dense case of the GPU suite."""
    for B, n_cols, G in A.SHAPES:
        for thr in A.THRESHOLDS:
            c = A.dense_case(n_cols, B, n_cols, G, thr)
            keep = (c.gene_map >= 0)[None, :] & (c.x > np.float32(thr))
            rowptr, col, raw = A.align_dense(c.x, c.gene_map, thr)
            np.testing.assert_array_equal(np.diff(rowptr), keep.sum(1))
            np.testing.assert_array_equal(col, np.broadcast_to(c.gene_map, c.x.shape)[keep])
            np.testing.assert_array_equal(A.bits(raw), A.bits(c.x[keep]))
            got = A.align_csr(*A.dense_to_csr(c.x), c.gene_map, thr)
            for g, w in zip(got, (rowptr, col, raw)):
                np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------------------------------------
# 3. the cases hold the corners they claim
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", A.THRESHOLDS)
@pytest.mark.parametrize("B,n_cols,G", A.SHAPES)
def test_cases_hold_their_corners(B, n_cols, G, thr):
    c = A.dense_case(n_cols, B, n_cols, G, thr)
    k = A.corners(c)
    assert c.x.shape == (B, n_cols) and c.gene_map.shape == (n_cols,)
    hit = c.gene_map[c.gene_map >= 0]
    assert hit.size >= 1 and len(set(hit.tolist())) == hit.size and hit.max() < G          # a gene at most once
    assert k.kept[0] == 0 and k.has_empty_row                                              # a row with nothing kept
    assert k.kept[1] == k.n_mapped and k.has_full_row                                      # a row with everything kept
    assert k.at_threshold                                                                  # a value exactly at the threshold
    if n_cols >= 63:
        assert (c.gene_map < 0).any() and k.foreign_value_above                            # foreign columns that hold values
        assert k.nan and k.neg_zero and k.negative
        assert not np.array_equal(hit, np.sort(hit))                                       # the map permutes
    if n_cols == 1000:
        assert k.longest > 64 * 4 and k.n_mapped > 512                                     # many steps, of every form
    if n_cols == 130:
        assert k.longest > 64 and n_cols % 4                                               # a second step, a ragged quad
    assert bool(np.isnan(A.dense_to_csr(c.x)[2]).any()) == k.nan                          # the CSR form stores the NaN explicitly


def test_grid_stride_case_and_leading_dims():
    B, n_cols, G = A.GRID_STRIDE_SHAPE
    assert B > 1024 * 8                                              # kAMaxBlocks * kAWaves of csrc/wgnn_align.hip
    text = (ROOT / "scdeepsort_amd" / "csrc" / "wgnn_align.hip").read_text()
    assert int(re.search(r"kAMaxBlocks = (\d+);", text).group(1)) * int(re.search(r"kAWaves = (\d+);", text).group(1)) == 8192
    for _, n, _ in A.SHAPES:
        ld = A.leading_dims(n)
        assert ld["packed"] == n and ld["padded"] % 4 == 0 and ld["padded"] > n and ld["odd"] % 4 and ld["odd"] > n


# ------------------------------------------------------------------------------------------------
# 4. gene_map's host logic
# ------------------------------------------------------------------------------------------------
def test_gene_map_ids():
    gene2id = {"A": 0, "B": 1, "7": 2, "D": 3}
    ids = api._gene_map_ids(["D", "zzz", 7, "A"], gene2id)                                 # names are compared as str
    assert ids.dtype == np.int32 and ids.tolist() == [3, -1, 2, 0]
    assert api._gene_map_ids(np.array(["B", "B2"]), gene2id).tolist() == [1, -1]
    assert api._gene_map_ids(pd.Index(["A", "D"]), gene2id).tolist() == [0, 3]
    with pytest.raises(ValueError, match="positions 1 and 3 .* both name bundle gene 2"):
        api._gene_map_ids(["A", "7", "x", 7], gene2id)
    with pytest.raises(ValueError, match="none of the 2 gene names"):
        api._gene_map_ids(["x", "y"], gene2id)
    with pytest.raises(ValueError, match="none of the 0 gene names"):
        api._gene_map_ids([], gene2id)
