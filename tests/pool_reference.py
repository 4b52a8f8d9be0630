"""numpy restatement of ``wgnn_pool_rows_accumulate`` / ``wgnn_pool_rows_count`` / ``wgnn_pool_rows_fill`` (``ops.pool_rows``),
written from the contract in ``include/wgnn.h``, and the cases the CPU and GPU tests share - a helper, not a test module.  Nothing
here imports torch or the package.

    total[k] = sum of lib over the group's cells;   c(k, g) = sum of the cells' counts of gene g      (Python integers)
    v = float32(log1p(float64(c) / float64(total[k]) * scale))  - ``lognorm_reference._value`` on the fp64 count, NOT through
                                                                   ``np.float32(c)``: a pooled count may exceed 2^24
    (g, v) leaves iff c > 0 and v > threshold, in ascending g;  total[k] == 0 gives the empty row.

What a comparison may ask is what tests/lognorm_reference.py says of a value: the float32 bits are EQUAL wherever the fp64 value
is not ``fragile``, one float32 ulp apart at most there.  Counts, totals and cell numbers are integers: equal."""
import functools
from types import SimpleNamespace

import numpy as np

import pairs_reference as P
from lognorm_reference import _value, fragile          # noqa: F401  (fragile is re-exported for the tests)

SCALE = P.SCALE
THRESHOLDS = P.THRESHOLDS
FRAGILE_CAP = 0.01


def pool_rows(rowptr, col, cnt, lib, group, n_groups, threshold, scale=SCALE, seed=None):
    """The pooled rows of ``group`` (int [B], -1 = skip) as a namespace: ``rowptr`` int64 [K + 1], ``col`` int32, ``val`` float32,
    ``v64`` (the kept values before their rounding), ``cnt`` int64, ``total`` int64 [K], ``n_cells`` int64 [K].  ``seed``: an
    earlier namespace over the same groups, pooled on top of."""
    rowptr = np.asarray(rowptr, np.int64)
    thr = np.float32(threshold)
    summed = [dict() for _ in range(n_groups)]
    total, n_cells = [0] * n_groups, [0] * n_groups
    if seed is not None:
        for k in range(n_groups):
            total[k], n_cells[k] = int(seed.total[k]), int(seed.n_cells[k])
            for e in range(seed.rowptr[k], seed.rowptr[k + 1]):
                summed[k][int(seed.col[e])] = int(seed.cnt[e])
    for r, k in enumerate(group):
        if k < 0:
            continue
        total[k] += int(lib[r])
        n_cells[k] += 1
        for e in range(rowptr[r], rowptr[r + 1]):
            summed[k][int(col[e])] = summed[k].get(int(col[e]), 0) + int(cnt[e])
    out_ptr, out_col, out_cnt, v64 = [0], [], [], []
    for k in range(n_groups):
        for g in sorted(summed[k]):
            c = summed[k][g]
            if total[k] > 0 and c > 0:
                v = _value(float(c), float(total[k]), scale)
                if np.float32(v) > thr:
                    out_col.append(g); out_cnt.append(c); v64.append(v)
        out_ptr.append(len(out_col))
    v64 = np.asarray(v64, np.float64)
    return SimpleNamespace(rowptr=np.asarray(out_ptr, np.int64), col=np.asarray(out_col, np.int32), val=v64.astype(np.float32),
                           v64=v64, cnt=np.asarray(out_cnt, np.int64), total=np.asarray(total, np.int64),
                           n_cells=np.asarray(n_cells, np.int64))


def summed_dense(m, group, n_groups):
    """The groups' summed counts as a dense float32 ``[K, G + 1]`` matrix - the last column holds the cells' reads outside the
    bundle - and the int32 gene map that sends column ``g`` to gene ``g`` and the last one to -1: what
    ``align_rows(..., normalize="lognorm")`` takes.  Exact wherever every sum is <= 2^24 (``small_groups``)."""
    dense = np.zeros((n_groups, m.G + 1), np.float64)
    for r, k in enumerate(group):
        if k < 0:
            continue
        sl = slice(m.rowptr[r], m.rowptr[r + 1])
        np.add.at(dense[k], m.col[sl], m.cnt[sl].astype(np.float64))
        dense[k, m.G] += int(m.lib[r]) - float(m.cnt[sl].astype(np.float64).sum())
    return dense.astype(np.float32), np.concatenate([np.arange(m.G), [-1]]).astype(np.int32)


def small_groups(m, group, n_groups):
    """bool [K]: the groups all of whose sums - every gene's, and the reads outside the bundle - are <= 2^24, so that a float32
    holds them."""
    exact = pool_rows(m.rowptr, m.col, m.cnt, m.lib, group, n_groups, 0.0)
    big = np.zeros(n_groups, bool)
    for k in range(n_groups):
        c = exact.cnt[exact.rowptr[k]:exact.rowptr[k + 1]]
        rest = int(exact.total[k]) - int(c.sum())
        big[k] = (c > 2 ** 24).any() or rest > 2 ** 24
    return ~big


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
BIG_GENE = 17
BIG_COUNT = 2 ** 24 + 1            # 2^23 + 2^23 + 1: what float32 cannot hold


def _differs(total):
    """Whether the value of BIG_COUNT against ``total`` has other float32 bits than that of float32(BIG_COUNT) = 2^24, and is
    not fragile."""
    exact = _value(float(BIG_COUNT), float(total), SCALE)
    through_f32 = _value(float(np.float32(BIG_COUNT)), float(total), SCALE)
    return np.float32(exact) != np.float32(through_f32) and not fragile([exact])[0] and not fragile([through_f32])[0]


@functools.lru_cache(maxsize=None)
def big_total():
    """The first total from 10^11 on at which the exact pooled count and its float32 rounding give different float32 values."""
    total = 10 ** 11
    while not _differs(total):
        total += 1
    return total


@functools.lru_cache(maxsize=None)
def batch():
    """``pairs_reference.batch()`` and, after its rows: ``ROW_EMPTY_2`` (a second row without entries or reads), ``ROW_UNSORTED``
    (descending genes), ``ROW_TWICE`` (gene 7 listed twice, gene 299 three times - they add), and ``ROW_BIG_A / _B / _C``, which
    hold 2^23, 2^23 and 1 of ``BIG_GENE`` (and a few other genes) and whose library sizes add up to ``big_total()``."""
    m = P.batch()
    rng = np.random.default_rng(77)
    rows = [(np.zeros(0, int), np.zeros(0)),
            (np.arange(290, 10, -7), rng.geometric(0.4, len(np.arange(290, 10, -7)))),
            (np.array([7, 120, 7, 299, 299, 3, 299]), np.array([2, 5, 3, 1, 4, 9, 6])),
            (np.array([3, BIG_GENE, 200]), np.array([4, 2 ** 23, 1])),
            (np.array([BIG_GENE, 128, 299]), np.array([2 ** 23, 7, 2])),
            (np.array([0, BIG_GENE]), np.array([1, 1]))]
    first = m.B
    names = dict(ROW_EMPTY_2=first, ROW_UNSORTED=first + 1, ROW_TWICE=first + 2, ROW_BIG_A=first + 3, ROW_BIG_B=first + 4,
                 ROW_BIG_C=first + 5)
    rowptr = np.concatenate([m.rowptr, m.rowptr[-1] + np.cumsum([len(g) for g, _ in rows])]).astype(np.int64)
    col = np.concatenate([m.col] + [g for g, _ in rows]).astype(np.int32)
    cnt = np.concatenate([m.cnt] + [c for _, c in rows]).astype(np.float32)
    sums = [int(c.sum()) for _, c in rows]
    rest = [0, 11, 0, 5, 0, 0]
    rest[5] = big_total() - sum(sums[3:]) - rest[3] - rest[4]            # the big group's total is big_total()
    lib = np.concatenate([m.lib, np.asarray(sums, np.int64) + np.asarray(rest, np.int64)])
    return SimpleNamespace(rowptr=rowptr, col=col, cnt=cnt, lib=lib, B=len(lib), G=m.G, random=list(range(first - P.N_RANDOM, first)),
                           **names)


# the groups of the main case, by name
(GROUP_NO_CELLS, GROUP_EMPTY_ROWS, GROUP_FOREIGN_ONLY, GROUP_ONE, GROUP_TWINS, GROUP_EVEN_ODD, GROUP_FOUR, GROUP_FIVE, GROUP_NINE,
 GROUP_BIG) = range(10)
N_GROUPS = 10


@functools.lru_cache(maxsize=None)
def groups():
    """int32 [B]: the main case's groups - none, all-empty rows, a row with reads only outside the bundle, and groups of 1, 2, 2,
    4, 5, 9 and 3 cells; five random rows take no part (-1).  The cells of a group are scattered over the batch."""
    m = batch()
    g = np.full(m.B, -1, np.int32)
    g[[P.ROW_EMPTY, m.ROW_EMPTY_2]] = GROUP_EMPTY_ROWS
    g[P.ROW_EMPTY_READS] = GROUP_FOREIGN_ONLY
    g[P.ROW_65] = GROUP_ONE
    g[[P.ROW_130, P.ROW_130_TWIN]] = GROUP_TWINS
    g[[P.ROW_EVEN, P.ROW_ODD]] = GROUP_EVEN_ODD
    g[[P.ROW_63, P.ROW_64, P.ROW_LOW, P.ROW_HIGH]] = GROUP_FOUR
    g[[P.ROW_LONG, P.ROW_BEFORE, P.ROW_INSIDE, P.ROW_AFTER, P.ROW_GAP]] = GROUP_FIVE
    g[[P.ROW_ALL, P.ROW_ONE, P.ROW_EDGE_A, P.ROW_EDGE_B, m.ROW_UNSORTED, m.ROW_TWICE] + m.random[:3]] = GROUP_NINE
    g[[m.ROW_BIG_A, m.ROW_BIG_B, m.ROW_BIG_C]] = GROUP_BIG
    return g


@functools.lru_cache(maxsize=None)
def case(threshold: float, which: str = "groups"):
    """The batch, a grouping (``"groups"``: the main case; ``"all"``: one group of every cell but the three ``ROW_BIG``, whose
    10^11 reads would push every other value of the group under any threshold) and the reference's pooled rows."""
    m = batch()
    group, K = groups(), N_GROUPS
    if which == "all":
        group, K = np.zeros(m.B, np.int32), 1
        group[[m.ROW_BIG_A, m.ROW_BIG_B, m.ROW_BIG_C]] = -1
    return SimpleNamespace(m=m, group=group, K=K, threshold=threshold, ref=pool_rows(m.rowptr, m.col, m.cnt, m.lib, group, K, threshold))
