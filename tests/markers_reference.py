"""fp64 restatement of the per-group gene tables (``wgnn_group_gene_reduce`` / ``ResidentPredictor.markers``), written from
the contract in ``include/wgnn.h`` - a helper for the CPU and GPU tests, not a test module.

For a batch of B cells in CSR form with one f32 score per stored (cell, gene) entry and one group id per cell (-1 = out):

    sum[k, g]   = sum over the cells i with group[i] == k that list g of score[i, g]        (fp64)
    count[k, g] = number of those cells
    mag[k, g]   = sum of |score| over the same entries (what the error bound scales with)

Bound of a device sum against this one (derived, not tuned): the f32 terms are exact in fp64, a bin of n terms takes n - 1
additions in ANY order, each rounding its partial sum (|partial| <= mag) by at most 2^-53 relative:

    |got - want| <= (n - 1) 2^-53 mag                                                       (``bound``)

On LATTICE scores - integer multiples of 2^-8 in [-1024, 1024] - every partial sum of a bin is a multiple of 2^-8 below
2^53 * 2^-8 in magnitude (``exact_premise``), so it is exact in fp64 in any order and the device must match bit for bit.
"""
from types import SimpleNamespace

import numpy as np

U64 = 2.0 ** -53
UNIT = 2.0 ** -8


def reduce(rowptr, col, scores, group, n_groups, n_genes):
    """(sum f64 [K, G], count int32 [K, G], mag f64 [K, G]) by ``np.add.at`` over the stored entries."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    group = np.asarray(group, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    k = group[rows]
    on = k >= 0
    s = np.asarray(scores, np.float64)[on]
    total = np.zeros((n_groups, n_genes))
    mag = np.zeros((n_groups, n_genes))
    count = np.zeros((n_groups, n_genes), np.int32)
    np.add.at(total, (k[on], col[on]), s)
    np.add.at(mag, (k[on], col[on]), np.abs(s))
    np.add.at(count, (k[on], col[on]), 1)
    return total, count, mag


def bound(count, mag):
    return np.maximum(count.astype(np.float64) - 1.0, 0.0) * U64 * mag


def exact_premise(mag):
    """sum |terms| / unit < 2^53 in every bin: each partial sum of lattice terms is then an exact fp64 number."""
    return bool((mag / UNIT < 2.0 ** 53).all())


def group_stats(group, base, logit, n_groups):
    """(n_cells int64 [K], n_skipped, base_sum f64 [K], logit_sum f64 [K])."""
    group = np.asarray(group, np.int64)
    on = group >= 0
    return (np.bincount(group[on], minlength=n_groups).astype(np.int64), int((~on).sum()),
            np.bincount(group[on], weights=np.asarray(base, np.float64)[on], minlength=n_groups),
            np.bincount(group[on], weights=np.asarray(logit, np.float64)[on], minlength=n_groups))


def ranking(total, count, n_cells, min_fraction=0.0):
    """Per group the eligible genes (count > 0, count / n_cells >= min_fraction) ordered by float32(total / n_cells)
    descending, equal keys by the lower gene id: a list of (genes int64, keys f32) per group."""
    out = []
    for k in range(total.shape[0]):
        n = float(n_cells[k])
        if n == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.float32)))
            continue
        key = (total[k] / n).astype(np.float32)
        ok = np.nonzero((count[k] > 0) & (count[k] / n >= min_fraction))[0]
        order = ok[np.argsort(-key[ok], kind="stable")]
        out.append((order.astype(np.int64), key[order]))
    return out


def clear_pairs(ranked, k):
    """Boolean [K, k]: (group, rank) pairs that exist and whose key is more than one f32 ulp (2^-22 |key|) away from both
    neighbours in the reference order - the pairs a device ranking is compared on."""
    clear = np.zeros((len(ranked), k), bool)
    exists = np.zeros((len(ranked), k), bool)
    for g, (_, key) in enumerate(ranked):
        key = key.astype(np.float64)
        for r in range(min(k, len(key))):
            exists[g, r] = True
            ulp = 2.0 ** -22 * abs(key[r])
            up = r == 0 or key[r - 1] - key[r] > ulp
            down = r + 1 >= len(key) or key[r] - key[r + 1] > ulp
            clear[g, r] = up and down
    return clear, exists


# ------------------------------------------------------------------------------------------------
# the operands of the GPU tests (built here so that the CPU suite can assert their premises)
# ------------------------------------------------------------------------------------------------
GROUPS = (1, 2, 16, 40, 300, 1024)
GENES = (64, 6000, 32768, 40000)
CASES = [(K, G, i64) for K in GROUPS for G in GENES for i64 in (False, True)]
SPECIAL = ("one_group", "no_cells", "all_skipped")


def _ragged(rng, B, G):
    """B rows: two empty, one of min(5000, G) entries, the rest 1 .. min(300, G); sorted gene ids, each once per row."""
    lens = rng.integers(1, min(300, G) + 1, B)
    if B > 4:
        lens[1] = 0
        lens[B - 2] = 0
        lens[3] = min(5000, G)
    cols = [np.sort(rng.choice(G, size=int(n), replace=False)) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = (np.concatenate(cols) if B else np.zeros(0)).astype(np.int32)
    return rowptr, col


def lattice(rng, n):
    return (rng.integers(-1024 * 256, 1024 * 256 + 1, n) * UNIT).astype(np.float32)


def case(K, G, i64, B=77, seed=None):
    """One operand: B = 77 cells (a multiple of nothing convenient), ~15 % of them in group -1, group K // 2 without a
    cell (K >= 2), lattice scores ``lat`` and N(0, 1) scores ``flt`` over the same structure."""
    rng = np.random.default_rng(seed if seed is not None else 1000003 * K + 7 * G + int(i64))
    rowptr, col = _ragged(rng, B, G)
    group = rng.integers(0, K, B).astype(np.int32)
    group[rng.random(B) < 0.15] = -1
    if K >= 2:
        group[group == K // 2] = -1
    if B > 4:
        group[3] = 0 if K < 3 else K - 1                 # the long row takes part
    nnz = int(rowptr[-1])
    return SimpleNamespace(K=K, G=G, i64=i64, B=B, rowptr=rowptr, col=col, group=group, lat=lattice(rng, nnz),
                           flt=rng.standard_normal(nnz).astype(np.float32))


def special(name):
    if name == "one_group":                              # all cells in one group of 16
        c = case(16, 6000, False, seed=5)
        c.group[:] = 9
    elif name == "no_cells":                             # B = 0
        c = case(16, 6000, True, B=0, seed=6)
    elif name == "all_skipped":                          # every cell -1
        c = case(2, 6000, False, seed=8)
        c.group[:] = -1
    else:
        raise KeyError(name)
    return c


def ranking_case():
    """Continuous random scores, 16 groups, 6 000 genes, 400 cells of ~300 genes."""
    rng = np.random.default_rng(12)
    K, G, B = 16, 6000, 400
    lens = rng.integers(200, 400, B)
    cols = [np.sort(rng.choice(G, size=int(n), replace=False)) for n in lens]
    c = case(K, G, False, seed=12)
    c.B, c.rowptr, c.col = B, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(cols).astype(np.int32)
    c.group = rng.integers(-1, K, B).astype(np.int32)
    c.flt = rng.standard_normal(int(c.rowptr[-1])).astype(np.float32)
    return c
