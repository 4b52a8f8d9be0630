"""numpy restatement of vocabulary coverage (``wgnn_coverage_rows`` / ``ResidentPredictor.coverage``), written from the contract
in ``include/wgnn.h`` - a helper for the CPU and GPU tests, not a test module.

    an entry COUNTS       iff  its value is finite and > 0          (0, -0.0, NaN, negative and infinite values do not)
    a column j is MAPPED  iff  gene_map[j] >= 0
    n_expressed[r]  = counting entries of row r over all columns         total[r]        = their fp64 sum
    n_mapped[r]     = those on mapped columns                            total_mapped[r] = their fp64 sum
    n_bad[r]        = entries of row r that are negative, NaN or infinite (in no other output)
    col_cells[j]    = rows in which column j counts

Plain loops, fp64 sums in column (CSR: stored) order.  The kernel folds a row in another fixed order; on the count cases of
``lognorm_reference`` every partial sum is exact in fp64 (its docstring), so the sums are compared with ``array_equal``.
"""
import math
from types import SimpleNamespace

import numpy as np

from align_reference import dense_to_csr, leading_dims, random_gene_map      # noqa: F401  (re-exported for the tests)
from lognorm_reference import count_case, to_csr                              # noqa: F401


def counts(v):
    v = float(v)
    return v > 0 and not math.isinf(v)


def is_bad(v):
    v = float(v)
    return math.isnan(v) or v < 0 or math.isinf(v)


def _empty(B, n_cols):
    return SimpleNamespace(n_expressed=np.zeros(B, np.int32), n_mapped=np.zeros(B, np.int32), n_bad=np.zeros(B, np.int32),
                           total=np.zeros(B, np.float64), total_mapped=np.zeros(B, np.float64),
                           col_cells=np.zeros(n_cols, np.int32))


def _entry(out, r, j, v, gene_map):
    if is_bad(v):
        out.n_bad[r] += 1
    elif counts(v):
        out.n_expressed[r] += 1
        out.total[r] += float(v)
        out.col_cells[j] += 1
        if gene_map[j] >= 0:
            out.n_mapped[r] += 1
            out.total_mapped[r] += float(v)


def coverage_dense(x, gene_map):
    """The six outputs of a dense [B, n_cols] matrix."""
    x = np.asarray(x, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    out = _empty(x.shape[0], x.shape[1])
    for r in range(x.shape[0]):
        for j in range(x.shape[1]):
            _entry(out, r, j, x[r, j], gene_map)
    return out


def coverage_csr(rowptr, col, val, gene_map):
    """The same for a CSR over the caller's columns (stored order)."""
    rowptr = np.asarray(rowptr, np.int64)
    val = np.asarray(val, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    out = _empty(len(rowptr) - 1, len(gene_map))
    for r in range(len(rowptr) - 1):
        for k in range(rowptr[r], rowptr[r + 1]):
            _entry(out, r, int(col[k]), val[k], gene_map)
    return out


FIELDS = ("n_expressed", "n_mapped", "n_bad", "total", "total_mapped", "col_cells")


def as_tuple(out):
    return tuple(getattr(out, f) for f in FIELDS)
