"""numpy restatement of ``wgnn_hood_rows_count`` / ``wgnn_hood_rows_fill`` (``ops.hood_rows``), written from the contract in
``include/wgnn.h``, and the cases the CPU and GPU tests share - a helper, not a test module.  Nothing here imports torch or the
package.

    unit q pools the rows members[hood_ptr[q] : hood_ptr[q + 1]] (a member listed twice adds twice)
    total = sum of lib over the members;   c(g) = sum of the members' counts of gene g                  (Python integers)
    v = float32(log1p(float64(c) / float64(total) * scale))  - ``lognorm_reference._value`` on the fp64 count, NOT through
                                                                ``np.float32(c)``: a pooled count may exceed 2^24
    (g, v) leaves iff c > 0 and v > threshold, in ascending g;  total == 0, or no member, gives the empty row.

Why the tests compare the VALUES bit for bit with this file, although the device's fp64 log1p and the host's may differ in the
last places: tests/lognorm_reference.py shows that the float32 bits can differ only where the fp64 value lies within 16 fp64
ulps of the midpoint between two adjacent float32 values (``fragile``).  tests/test_hood_reference.py asserts that NO value of
the cases below is fragile - a property of this file's data alone - so every float32 here is decided.  Counts, totals and row
lengths are integers: equal in any case."""
import functools
from types import SimpleNamespace

import numpy as np

from lognorm_reference import _value, fragile          # noqa: F401  (fragile is re-exported for the tests)

SCALE = 1e4
THRESHOLDS = (0.0, 1.5)
MAX_MEMBERS = 256


def hood_rows(rowptr, col, cnt, lib, hood_ptr, members, threshold, scale=SCALE):
    """The pooled rows of the units as a namespace: ``rowptr`` int64 [U + 1], ``col`` int32, ``val`` float32, ``v64`` (the kept
    values before their rounding), ``cnt`` int64, ``total`` int64 [U]."""
    rowptr = np.asarray(rowptr, np.int64)
    thr = np.float32(threshold)
    out_ptr, out_col, out_cnt, v64, totals = [0], [], [], [], []
    for q in range(len(hood_ptr) - 1):
        summed, total = {}, 0
        for r in members[hood_ptr[q]:hood_ptr[q + 1]]:
            total += int(lib[r])
            for e in range(rowptr[r], rowptr[r + 1]):
                summed[int(col[e])] = summed.get(int(col[e]), 0) + int(cnt[e])
        for g in sorted(summed):
            c = summed[g]
            if total > 0 and c > 0:
                v = _value(float(c), float(total), scale)
                if np.float32(v) > thr:
                    out_col.append(g); out_cnt.append(c); v64.append(v)
        out_ptr.append(len(out_col))
        totals.append(total)
    v64 = np.asarray(v64, np.float64)
    return SimpleNamespace(rowptr=np.asarray(out_ptr, np.int64), col=np.asarray(out_col, np.int32), val=v64.astype(np.float32),
                           v64=v64, cnt=np.asarray(out_cnt, np.int64), total=np.asarray(totals, np.int64))


def lists(units):
    """``(hood_ptr int64 [U + 1], members int32)`` of a list of member lists."""
    ptr = np.concatenate([[0], np.cumsum([len(u) for u in units])]).astype(np.int64)
    return ptr, np.asarray([r for u in units for r in u], np.int32)


def summed_dense(m, units):
    """The units' summed counts as a dense float32 ``[U, G + 1]`` matrix - the last column holds the members' reads outside the
    bundle - and the int32 gene map that sends column ``g`` to gene ``g`` and the last one to -1: what
    ``align_rows(..., normalize="lognorm")`` takes.  Exact wherever every sum is <= 2^24."""
    dense = np.zeros((len(units), m.G + 1), np.float64)
    for q, unit in enumerate(units):
        for r in unit:
            sl = slice(m.rowptr[r], m.rowptr[r + 1])
            np.add.at(dense[q], m.col[sl], m.cnt[sl].astype(np.float64))
            dense[q, m.G] += int(m.lib[r]) - float(m.cnt[sl].astype(np.float64).sum())
    assert dense.max(initial=0) <= 2 ** 24
    return dense.astype(np.float32), np.concatenate([np.arange(m.G), [-1]]).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
B_CASE, G_CASE = 40, 300
ROW_EMPTY, ROW_EMPTY_READS, ROW_ONE, ROW_ALL, ROW_BIG, ROW_BIG_ONE, ROW_65, ROW_LAST_GENE = range(8)
BIG_GENE = 17


@functools.lru_cache(maxsize=None)
def batch():
    """40 rows over 300 genes, every row strictly ascending (``pair_rows`` takes them): a row without entries or reads, one with
    reads outside the bundle only, a single gene, all 300 genes, ``ROW_BIG`` (2^23 of ``BIG_GENE`` and three other genes),
    ``ROW_BIG_ONE`` (1 of ``BIG_GENE``), a row of 65 genes, a row that holds the last gene of every slab of 128, and 32 random
    rows of 2 to 199 genes.  ``lib`` = the row's sum plus, on every third row, reads outside the bundle."""
    rng = np.random.default_rng(61_000)
    pick = lambda n: np.sort(rng.choice(G_CASE, size=n, replace=False))
    rows = [np.zeros(0, int), np.zeros(0, int), np.array([5]), np.arange(G_CASE), np.array([3, BIG_GENE, 128, 299]),
            np.array([BIG_GENE, 200]), pick(65), np.array([0, 127, 128, 255, 256, 299])]
    rows += [pick(int(n)) for n in rng.integers(2, 200, B_CASE - len(rows))]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    cnt = rng.geometric(0.4, col.shape[0]).astype(np.float32)
    cnt[rowptr[ROW_BIG] + 1] = 2.0 ** 23                               # the largest count the operand check admits
    cnt[rowptr[ROW_BIG_ONE]] = 1.0
    rest = np.where(np.arange(B_CASE) % 3 == 0, rng.integers(1, 4000, B_CASE), 0)
    rest[ROW_EMPTY], rest[ROW_EMPTY_READS] = 0, 7
    lib = np.asarray([cnt[rowptr[r]:rowptr[r + 1]].sum() for r in range(B_CASE)], np.int64) + rest
    return SimpleNamespace(rowptr=rowptr, col=col, cnt=cnt, lib=lib, rest=rest, B=B_CASE, G=G_CASE)


# the units of the main case, by name; UNIT_RAGGED is the first of N_RAGGED units of 0 to 9 random members
(UNIT_NONE, UNIT_ONE, UNIT_PAIR, UNIT_ALL, UNIT_EMPTY_ROWS, UNIT_FOREIGN_ONLY, UNIT_TWICE, UNIT_256, UNIT_255_AND_ONE,
 UNIT_RAGGED) = range(10)
N_RAGGED = 14


@functools.lru_cache(maxsize=None)
def units():
    """The member lists of the main case: no member, one, a pair, all 40 rows, two rows without entries, the row with reads
    outside the bundle only, a row listed twice next to another, ``ROW_BIG`` 256 times (the counter of ``BIG_GENE`` reaches
    256 x 2^23 = 2^31), ``ROW_BIG`` 255 times and ``ROW_BIG_ONE`` (255 x 2^23 + 1: odd and above 2^24, no float32 holds it), then
    ragged lists of 0 to 9 distinct members: the first two of 0 and of 9, the last of 3 (it ends on ``ROW_LAST_GENE``, so the
    last slot of the whole output is written)."""
    rng = np.random.default_rng(62_000)
    out = [[], [ROW_65], [ROW_ALL, 11], list(range(B_CASE)), [ROW_EMPTY, ROW_EMPTY_READS, ROW_EMPTY], [ROW_EMPTY_READS],
           [9, ROW_LAST_GENE, 9], [ROW_BIG] * MAX_MEMBERS, [ROW_BIG] * (MAX_MEMBERS - 1) + [ROW_BIG_ONE]]
    sizes = [0, 9] + [int(n) for n in rng.integers(0, 10, N_RAGGED - 3)]
    out += [[int(r) for r in rng.choice(B_CASE, size=n, replace=False)] for n in sizes] + [[20, 30, ROW_LAST_GENE]]
    return tuple(tuple(u) for u in out)


@functools.lru_cache(maxsize=None)
def case(threshold: float):
    """The batch, the units and the reference's pooled rows at ``threshold``."""
    m = batch()
    hood_ptr, members = lists(units())
    return SimpleNamespace(m=m, units=units(), hood_ptr=hood_ptr, members=members, threshold=threshold,
                           ref=hood_rows(m.rowptr, m.col, m.cnt, m.lib, hood_ptr, members, threshold))
