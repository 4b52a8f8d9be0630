"""numpy restatement of ``wgnn_pair_rows_count`` / ``wgnn_pair_rows_fill`` (``ops.pair_rows``) and of the partner rule of
``ResidentPredictor.doublets``, written from the contract in ``include/wgnn.h`` and the method's docstring, and the cases the
CPU and GPU tests share - a helper, not a test module.  Nothing here imports torch or the package.

    total = float64(lib[a] + lib[b]);  c(g) = cnt_a(g) + cnt_b(g) over the union of the two rows;
    v = float32(log1p(float64(c) / total * scale))  - ``lognorm_reference._value``, imported, not copied;
    (g, v) leaves iff c > 0 and v > threshold, in ascending g.

What a comparison may ask is what tests/lognorm_reference.py says of a value: the float32 bits are EQUAL wherever the fp64 value
is not ``fragile`` (within 16 fp64 ulps of a float32 rounding boundary), one float32 ulp apart at most there.  The totals and
the summed counts are integers far below 2^53, exact in any order."""
import functools
from types import SimpleNamespace

import numpy as np

import stability_reference as R
from lognorm_reference import _value, fragile          # noqa: F401  (fragile is re-exported for the tests)
from thin_reference import mix64_np

GOLDEN = 0x9E3779B97F4A7C15
SCALE = 1e4


# ------------------------------------------------------------------------------------------------
# the merge
# ------------------------------------------------------------------------------------------------
def pair_rows(rowptr, col, cnt, lib, a, b, threshold, scale=SCALE):
    """``(rowptr int64 [n_pairs + 1], col int32, val float32, v64 float64)`` of the pairs ``(a[q], b[q])``; ``v64`` holds the
    kept values before their rounding to float32."""
    rowptr = np.asarray(rowptr, np.int64)
    thr = np.float32(threshold)
    out_ptr, out_col, v64 = [0], [], []
    for ra, rb in zip(a, b):
        total = float(int(lib[ra]) + int(lib[rb]))
        summed = {}
        for r in (ra, rb):
            for k in range(rowptr[r], rowptr[r + 1]):
                summed[int(col[k])] = summed.get(int(col[k]), 0.0) + float(cnt[k])
        for g in sorted(summed):
            c = summed[g]
            if total > 0 and c > 0:
                v = _value(np.float32(c), total, scale)
                if np.float32(v) > thr:
                    out_col.append(g); v64.append(v)
        out_ptr.append(len(out_col))
    v64 = np.asarray(v64, np.float64)
    return np.asarray(out_ptr, np.int64), np.asarray(out_col, np.int32), v64.astype(np.float32), v64


def summed_dense(rowptr, col, cnt, lib, a, b, n_genes):
    """The pairs' summed counts as a dense float32 ``[n_pairs, n_genes + 1]`` matrix - the last column holds the two cells' reads
    outside the bundle - and the int32 gene map ``[n_genes + 1]`` that sends column ``g`` to gene ``g`` and the last one to -1:
    what ``align_rows(..., normalize="lognorm")`` takes."""
    rowptr = np.asarray(rowptr, np.int64)
    dense = np.zeros((len(rowptr) - 1, n_genes + 1), np.float64)
    for r in range(len(rowptr) - 1):
        dense[r, col[rowptr[r]:rowptr[r + 1]]] = cnt[rowptr[r]:rowptr[r + 1]]
        dense[r, n_genes] = int(lib[r]) - dense[r, :n_genes].sum()
    x = (dense[np.asarray(a)] + dense[np.asarray(b)]).astype(np.float32)
    return x, np.concatenate([np.arange(n_genes), [-1]]).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# the partner rule
# ------------------------------------------------------------------------------------------------
def partner_u(seed, cell, draw) -> np.ndarray:
    """uint64 ``mix64(key(seed, cell, draw) + GOLDEN)`` with the dropout block's key; arrays broadcast."""
    cell, draw = np.asarray(cell).astype(np.uint64), np.asarray(draw).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = np.uint64(seed & R.M64) ^ (cell * np.uint64(R.K_CELL)) ^ (draw * np.uint64(R.K_DRAW))
        return mix64_np(key + np.uint64(GOLDEN))


def partners(label, n_partners, seed, across, draw0=0) -> np.ndarray:
    """int32 ``[B, n_partners]``: the partner of every (cell, draw) by the rule of ``ResidentPredictor.doublets``, one pair at a
    time in Python integers."""
    label = np.asarray(label, np.int64)
    B = len(label)
    order = np.argsort(label, kind="stable")                          # by (full call, index)
    out = np.zeros((B, n_partners), np.int32)
    for c in range(B):
        group = np.flatnonzero(label[order] == label[c])              # the cell's own group: a run of the order
        for d in range(n_partners):
            u = int(partner_u(seed, c, draw0 + d))
            if across == "any":
                k = u % (B - 1)
                out[c, d] = k + (k >= c)
            else:
                k = u % (B - len(group))
                out[c, d] = order[k if k < group[0] else k + len(group)]
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
G_CASE = 300
THRESHOLDS = (0.0, 1.5)
ROW_EMPTY, ROW_ONE, ROW_63, ROW_64, ROW_65, ROW_130, ROW_ALL, ROW_EVEN, ROW_ODD, ROW_LOW, ROW_HIGH, ROW_130_TWIN = range(12)
ROW_EMPTY_READS, ROW_LONG, ROW_BEFORE, ROW_INSIDE, ROW_AFTER, ROW_GAP, ROW_EDGE_A, ROW_EDGE_B = range(12, 20)
N_RANDOM = 8
CASE_SEED = 0


@functools.lru_cache(maxsize=None)
def batch(seed: int = CASE_SEED):
    """The count batch of the pair tests over ``G_CASE`` genes, rows strictly ascending: an empty row without and one with reads
    outside the bundle, rows of 1, 63, 64, 65, 130 and 300 genes, the even and the odd genes, two disjoint rows, two rows on one
    gene set, a long row (genes 100..199 without 151) and single genes before (50), inside and held (150), inside and not held
    (151) and after it (250), two rows whose common gene 100 falls on the merged positions 63 | 64, and ``N_RANDOM`` random rows.
    ``lib`` = the row's sum plus, on every third row, reads outside the bundle."""
    rng = np.random.default_rng(52_000 + seed)
    pick = lambda n: np.sort(rng.choice(G_CASE, size=n, replace=False))
    g130 = pick(130)
    rows = [np.zeros(0, int), np.array([5]), pick(63), pick(64), pick(65), g130, np.arange(G_CASE), np.arange(0, G_CASE, 2),
            np.arange(1, G_CASE, 2), np.arange(0, 100), np.arange(200, 300), g130.copy(), np.zeros(0, int),
            np.array([g for g in range(100, 200) if g != 151]), np.array([50]), np.array([150]), np.array([250]), np.array([151]),
            np.concatenate([np.arange(0, 64, 2), [100, 110, 112]]), np.concatenate([np.arange(1, 62, 2), [100, 111]])]
    rows += [pick(int(n)) for n in rng.integers(2, 200, N_RANDOM)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    cnt = rng.geometric(0.4, col.shape[0]).astype(np.float32)
    cnt[rowptr[ROW_ALL]] = 2.0 ** 23                                   # the largest count the operand check admits
    rest = np.where(np.arange(len(rows)) % 3 == 0, rng.integers(1, 4000, len(rows)), 0)
    rest[ROW_EMPTY], rest[ROW_EMPTY_READS] = 0, 7
    lib = np.asarray([cnt[rowptr[r]:rowptr[r + 1]].sum() for r in range(len(rows))], np.int64) + rest
    return SimpleNamespace(rowptr=rowptr, col=col, cnt=cnt, lib=lib, rest=rest, B=len(rows), G=G_CASE)


def pair_list(B):
    """Every ordered pair of rows, the self pairs included."""
    a, b = np.divmod(np.arange(B * B), B)
    return a.astype(np.int32), b.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(threshold: float, seed: int = CASE_SEED):
    """The batch, all its ordered pairs and the reference's merged rows at ``threshold``."""
    m = batch(seed)
    a, b = pair_list(m.B)
    rowptr, col, val, v64 = pair_rows(m.rowptr, m.col, m.cnt, m.lib, a, b, threshold)
    return SimpleNamespace(m=m, a=a, b=b, rowptr=rowptr, col=col, val=val, v64=v64, threshold=threshold)
