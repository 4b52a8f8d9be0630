"""numpy restatement of batch alignment (``wgnn_align_count`` / ``wgnn_align_fill`` / ``ResidentPredictor.align``), written from
the contract in ``include/wgnn.h`` - a helper for the CPU and GPU tests, not a test module.

    entry (r, j) with value v is kept  iff  gene_map[j] >= 0  and  v > threshold       (a NaN fails the comparison)
    kept entries of a row leave in input order as (gene_map[j], v), v's bits untouched

Everything is selection and copy, so every comparison against this file is ``array_equal`` on the raw bits: no tolerance.
It also generates the cases of the GPU suite (``dense_case``) and says which corners each one holds (``corners``).
"""
from types import SimpleNamespace

import numpy as np


def align_dense(x, gene_map, threshold):
    """(rowptr int64 [B+1], col int32, raw f32) of a dense [B, n_cols] matrix: a plain loop over rows and columns."""
    x = np.asarray(x, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    thr = np.float32(threshold)
    rowptr, col, raw = [0], [], []
    for r in range(x.shape[0]):
        for j in range(x.shape[1]):
            if gene_map[j] >= 0 and x[r, j] > thr:
                col.append(gene_map[j]); raw.append(x[r, j])
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(raw, np.float32)


def align_csr(rowptr, col, val, gene_map, threshold):
    """The same for a CSR over the caller's columns (stored order, nothing merged or sorted)."""
    rowptr = np.asarray(rowptr, np.int64)
    val = np.asarray(val, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    thr = np.float32(threshold)
    out_ptr, out_col, out_raw = [0], [], []
    for r in range(len(rowptr) - 1):
        for k in range(rowptr[r], rowptr[r + 1]):
            g = gene_map[col[k]]
            if g >= 0 and val[k] > thr:
                out_col.append(g); out_raw.append(val[k])
        out_ptr.append(len(out_col))
    return np.asarray(out_ptr, np.int64), np.asarray(out_col, np.int32), np.asarray(out_raw, np.float32)


def dense_to_csr(x, keep=None):
    """A CSR over the caller's columns holding the entries of ``x`` where ``keep`` (default: x != 0 or NaN, so that explicit
    sub-threshold and NaN entries stay stored), columns ascending."""
    x = np.asarray(x, np.float32)
    keep = ((x != 0) | np.isnan(x)) if keep is None else keep
    rows, cols = np.nonzero(keep)
    rowptr = np.zeros(x.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=x.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), x[rows, cols]


def bits(a):
    """float32 values as their bit patterns: ``array_equal`` on these tells -0.0 from 0.0 and compares NaNs."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_gene_map(rng, n_cols, n_genes, foreign=0.25):
    """A permutation-like map: distinct bundle ids in random order, about ``foreign`` of the columns -1."""
    ids = rng.permutation(max(n_genes, n_cols))[:n_cols].astype(np.int32)
    ids[ids >= n_genes] = -1
    ids[rng.random(n_cols) < foreign] = -1
    return ids


def dense_case(seed, B, n_cols, n_genes, threshold, density=0.35, special=True):
    """A dense batch with the corners the kernel can get wrong.  Values are small positive floats at ``density``, else 0;
    with ``special`` (and room for it): row 0 keeps nothing, row 1 keeps every mapped column, row 2 holds values exactly at
    the threshold, a -0.0, a NaN and a negative value on mapped columns."""
    rng = np.random.default_rng(seed)
    gene_map = random_gene_map(rng, n_cols, n_genes)
    if n_cols and not (gene_map >= 0).any():
        gene_map[rng.integers(n_cols)] = 0
    x = np.where(rng.random((B, n_cols)) < density, rng.uniform(0.6, 6.0, (B, n_cols)), 0.0).astype(np.float32)
    if special and B >= 3 and n_cols:
        x[0] = np.float32(threshold)                                   # nothing kept: every value AT the threshold
        x[1] = rng.uniform(1.0, 5.0, n_cols).astype(np.float32)       # everything mapped is kept
        on = np.flatnonzero(gene_map >= 0)
        picks = on[:: max(1, len(on) // 4)][:4]
        for j, v in zip(picks, (np.float32(threshold), np.float32(-0.0), np.float32(np.nan), np.float32(-1.5))):
            x[2, j] = v
    return SimpleNamespace(x=x, gene_map=gene_map, n_genes=n_genes, threshold=threshold, B=B, n_cols=n_cols)


def corners(case):
    """What a dense case really holds, for the tests to assert: per-row kept counts and which special values sit on mapped columns."""
    rowptr, col, raw = align_dense(case.x, case.gene_map, case.threshold)
    kept = np.diff(rowptr)
    mapped = case.gene_map >= 0
    xm = case.x[:, mapped] if case.n_cols else np.zeros((case.B, 0), np.float32)
    return SimpleNamespace(
        kept=kept, n_mapped=int(mapped.sum()),
        has_empty_row=bool((kept == 0).any()), has_full_row=bool(mapped.any() and (kept == mapped.sum()).any()),
        longest=int(kept.max()) if kept.size else 0,
        at_threshold=bool((xm == np.float32(case.threshold)).any()), nan=bool(np.isnan(xm).any()),
        neg_zero=bool(((xm == 0) & np.signbit(xm)).any()), negative=bool((xm < 0).any()),
        foreign_value_above=bool(case.n_cols and (case.x[:, ~mapped] > case.threshold).any()))


# the dense shapes of the GPU suite: (B, n_cols, n_genes).  n_cols 1 / 63 / 64 / 65 sit on the edges of the 64-lane mask, 130 needs
# a second 64-entry step and ends inside a 4-column quad, 1000 takes many steps (and a second 512-column step of the 16-byte form).
SHAPES = [(37, 1, 5), (37, 63, 50), (37, 64, 50), (37, 65, 50), (37, 130, 100), (37, 1000, 700)]
THRESHOLDS = (0.0, 0.5)
GRID_STRIDE_SHAPE = (8300, 8, 6)      # more rows than the grid holds waves (1024 workgroups x 8)


def leading_dims(n_cols):
    """Row strides that reach each dense form: packed, padded to 16-byte rows (the 4-columns-per-lane form, with a ragged last
    quad when n_cols % 4), and a stride that is no multiple of 4 (the one-column-per-lane form)."""
    padded = -(-n_cols // 4) * 4 + 4
    odd = n_cols + 1 if (n_cols + 1) % 4 else n_cols + 2
    return {"packed": n_cols, "padded": padded, "odd": odd}
