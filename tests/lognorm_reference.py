"""numpy restatement of log-normalising alignment (``wgnn_align_count_ln`` / ``wgnn_align_fill_ln``,
``ResidentPredictor.align(..., normalize="lognorm")``), written from the contract in ``include/wgnn.h`` - a helper for the CPU
and GPU tests, not a test module.

    total[r] = sum over ALL j of float64(x[r, j])                       (columns outside the bundle included)
    v[r, j]  = float32(log1p(float64(x[r, j]) / total[r] * scale))      (fp64 throughout: divide, scale, log1p)
    entry (r, j) is kept  iff  gene_map[j] >= 0  and  x[r, j] > 0  and  v[r, j] > threshold
    kept entries of a row leave in input order as (gene_map[j], v[r, j]); a row whose total is 0 keeps nothing
    library_size[r], when given, replaces total[r]

Everything is fp64 and plain loops.  What a comparison against this file may ask:

* The total.  The kernel folds a row in another (fixed) order than the loop below.  The cases of this file make that order
  irrelevant: every count is a float32 that is a multiple of 2^-3 and below 2^20, and a row has at most 1000 of them, so every
  partial sum is a multiple of 2^-3 below 2^30 - 33 bits, exact in fp64 whatever the order.  Totals therefore agree bit for bit.
* The value.  The division and the product are correctly rounded (0.5 ulp each), log1p has condition number <= 1 on y >= 0,
  so they reach its result as at most 1 ulp; the device library's fp64 log1p is a few ulps at worst (the HIP math API lists 1).
  ``fragile`` marks the fp64 values that lie within 16 fp64 ulps - the margin over that sum - of the midpoint between two
  adjacent float32 values: only there may the rounding to float32 differ, by one float32 ulp.  Everywhere else the float32
  bits must be EQUAL.  (An all-float32 evaluation differs on about 7 % of the entries: it does not pass.)
"""
import math
from types import SimpleNamespace

import numpy as np

from align_reference import dense_to_csr, random_gene_map

FRAGILE_ULPS = 16


def _check_count(x):
    if not (x >= 0) or math.isinf(x):                                 # negative, NaN, infinite
        raise ValueError(f"bad count {x!r}")


def _row_total(values, library_size, r):
    total = 0.0
    for x in values:
        _check_count(x)
        total += float(x)
    if library_size is not None and total > 0:
        total = float(library_size[r])
        if not (total > 0) or math.isinf(total):
            raise ValueError(f"bad library size {total!r}")
    return total


def _value(x, total, scale):
    return math.log1p(float(x) / total * scale)


def lognorm_dense(x, gene_map, threshold, scale=1e4, library_size=None, fp64=False):
    """(rowptr int64 [B+1], col int32, v float32) of a dense [B, n_cols] count matrix; with ``fp64`` also the kept values before
    their rounding to float32."""
    x = np.asarray(x, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    thr = np.float32(threshold)
    rowptr, col, v64 = [0], [], []
    for r in range(x.shape[0]):
        total = _row_total(x[r], library_size, r)
        for j in range(x.shape[1]):
            if total > 0 and gene_map[j] >= 0 and x[r, j] > 0:
                v = _value(x[r, j], total, scale)
                if np.float32(v) > thr:
                    col.append(gene_map[j]); v64.append(v)
        rowptr.append(len(col))
    out = (np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(v64, np.float64).astype(np.float32))
    return out + (np.asarray(v64, np.float64),) if fp64 else out


def lognorm_csr(rowptr, col, val, gene_map, threshold, scale=1e4, library_size=None, fp64=False):
    """The same for a CSR over the caller's columns (stored order; the total is the sum of the row's stored entries)."""
    rowptr = np.asarray(rowptr, np.int64)
    val = np.asarray(val, np.float32)
    gene_map = np.asarray(gene_map, np.int32)
    thr = np.float32(threshold)
    out_ptr, out_col, v64 = [0], [], []
    for r in range(len(rowptr) - 1):
        total = _row_total(val[rowptr[r]: rowptr[r + 1]], library_size, r)
        for k in range(rowptr[r], rowptr[r + 1]):
            g = gene_map[col[k]]
            if total > 0 and g >= 0 and val[k] > 0:
                v = _value(val[k], total, scale)
                if np.float32(v) > thr:
                    out_col.append(g); v64.append(v)
        out_ptr.append(len(out_col))
    out = (np.asarray(out_ptr, np.int64), np.asarray(out_col, np.int32), np.asarray(v64, np.float64).astype(np.float32))
    return out + (np.asarray(v64, np.float64),) if fp64 else out


def totals(x):
    """The fp64 row totals of a dense count matrix (the loop of ``_row_total``)."""
    return np.asarray([_row_total(row, None, r) for r, row in enumerate(np.asarray(x, np.float32))], np.float64)


def fragile(v64):
    """True where an fp64 value lies within ``FRAGILE_ULPS`` fp64 ulps of the midpoint between two adjacent float32 values, i.e.
    where an evaluation that is off by that much may round to the other float32."""
    v64 = np.asarray(v64, np.float64)
    f = v64.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    down = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    dist = np.minimum(np.abs(v64 - (f + up) / 2), np.abs(v64 - (f + down) / 2))
    return dist <= FRAGILE_ULPS * np.spacing(np.abs(v64))


# rows of a count case that hold the corners, when the case has room for them (B >= 6, n_cols >= 63)
ROW_ZERO, ROW_FOREIGN_ONLY, ROW_ONE_BIG, ROW_BEYOND_2_24, ROW_NEG_ZERO, ROW_FRACTIONS = range(6)


def count_case(seed, B, n_cols, n_genes, threshold, density=0.3, special=True):
    """A dense batch of raw counts: Poisson draws with about ``density`` of the entries positive.  With ``special`` and room for
    them, rows 0..5 hold the corners named by the ROW_* constants."""
    rng = np.random.default_rng(seed)
    gene_map = random_gene_map(rng, n_cols, n_genes)
    if n_cols and not (gene_map >= 0).any():
        gene_map[rng.integers(n_cols)] = 0
    x = rng.poisson(-math.log1p(-density), (B, n_cols)).astype(np.float32)
    if special and B >= 6 and n_cols >= 63:
        if not (gene_map < 0).any():
            gene_map[n_cols // 2] = -1
        on, off = np.flatnonzero(gene_map >= 0), np.flatnonzero(gene_map < 0)
        x[ROW_ZERO] = 0
        x[ROW_FOREIGN_ONLY] = 0
        x[ROW_FOREIGN_ONLY, off] = rng.integers(1, 9, len(off))          # positive total, nothing kept
        x[ROW_ONE_BIG] = 1
        x[ROW_ONE_BIG, on[len(on) // 2]] = 60000
        # a total beyond 2^24 by an odd amount: a float32 total cannot hold it
        big, n_big = (70000, 300) if n_cols >= 303 else (700000, n_cols - 3)
        x[ROW_BEYOND_2_24] = 0
        x[ROW_BEYOND_2_24, :n_big] = big
        x[ROW_BEYOND_2_24, n_big: n_big + 3] = 1
        x[ROW_NEG_ZERO, on[0]] = np.float32(-0.0)
        frac = rng.random(n_cols) < density
        x[ROW_FRACTIONS] = np.where(frac, rng.integers(1, 64, n_cols) / 8.0, 0.0)      # multiples of 1/8: see the module docstring
    return SimpleNamespace(x=x, gene_map=gene_map, n_genes=n_genes, threshold=threshold, B=B, n_cols=n_cols)


def corners(case, scale=1e4):
    """What a count case really holds, for the tests to assert."""
    rowptr, col, raw = lognorm_dense(case.x, case.gene_map, case.threshold, scale)
    kept = np.diff(rowptr)
    mapped = case.gene_map >= 0
    t = totals(case.x)
    xm = case.x[:, mapped]
    return SimpleNamespace(
        kept=kept, totals=t,
        zero_row=bool(((case.x == 0).all(axis=1)).any()),
        foreign_only_row=bool(((t > 0) & ((xm > 0).sum(axis=1) == 0)).any()),
        one_big_among_ones=bool(((xm == 60000).sum(axis=1) == 1).any() and ((case.x == 1).sum(axis=1) >= case.n_cols - 1).any()),
        total_beyond_2_24_odd=bool(((t > 2 ** 24) & (t % 2 == 1)).any()),
        neg_zero=bool(((xm == 0) & np.signbit(xm)).any()),
        fractions=bool((case.x != np.round(case.x)).any()),
        foreign_counts=bool((case.x[:, ~mapped] > 0).any()))


def to_csr(x):
    """The stored form of a count matrix: every non-zero entry and every -0.0 (an explicit zero), columns ascending."""
    x = np.asarray(x, np.float32)
    return dense_to_csr(x, keep=(x != 0) | np.signbit(x) | np.isnan(x))
