"""A dense numpy / scipy reference of ``wgnn_rank_genes_groups`` (``include/wgnn.h``) and of the host step behind
``ResidentPredictor.rank_genes``, and the builders of the cases its tests share.

``tables``: per gene ``scipy.stats.rankdata(method="average")`` over the participating cells' values (a cell that does not list
the gene holds +0.0), doubled and rounded to int64 and added per group; the tie term from ``np.unique``'s counts.  Values are
compared through the kernel's order-preserving integer key of the f32 bits, which is the numeric order on finite values with
-0.0 below +0.0.  ``host_stats``: U, AUC, z and p in scalar Python floats, operation by operation as the header orders them -
written apart from ``api._rank_genes_stats``, which must give the same bits.

Against ``scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic")`` over every (group, gene) of the cases below with
both sides non-empty and not all values tied: U is equal, and the largest relative difference of p measured on the CPU is 0.0
(test_rank_genes_reference.py asserts 16 x that, no less than 4 ulp of fp64)."""
import math

import numpy as np
from scipy.special import ndtr
from scipy.stats import rankdata

P_REL_MEASURED = 0.0                # the largest |p - p_scipy| / p_scipy over this file's cases
KEY0 = 0x80000000                   # the key of +0.0f
GENE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 129, 511, 512, 513, 600)     # the wave, vector and owner-block edges


def rank_key(val) -> np.ndarray:
    """int64: the order-preserving key of f32 bit patterns (all bits flipped under a set sign bit, else the sign bit set)."""
    u = np.ascontiguousarray(val, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def tables(rowptr, col, val, group, n_groups: int, n_genes: int):
    """``(rank2_sum int64 [K, G], count int32 [K, G], tie_sum int64 [G], group_size int64 [K])`` of a cell-major batch."""
    rowptr, col, group = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(group, np.int64)
    B, K, G = len(rowptr) - 1, int(n_groups), int(n_genes)
    keys = np.full((B, G), KEY0, np.int64)
    stored = np.zeros((B, G), bool)
    rows = np.repeat(np.arange(B), np.diff(rowptr))
    keys[rows, col] = rank_key(val)
    stored[rows, col] = True
    part = (group >= 0) & (group < K)
    keys, stored, grp = keys[part], stored[part], group[part]
    rank2_sum, count, tie_sum = np.zeros((K, G), np.int64), np.zeros((K, G), np.int32), np.zeros(G, np.int64)
    for g in range(G):
        if len(grp):
            r2 = np.rint(2.0 * rankdata(keys[:, g], method="average")).astype(np.int64)
            np.add.at(rank2_sum[:, g], grp, r2)
            np.add.at(count[:, g], grp, stored[:, g].astype(np.int32))
            t = np.unique(keys[:, g], return_counts=True)[1].astype(np.int64)
            tie_sum[g] = int((t ** 3 - t).sum())
    return rank2_sum, count, tie_sum, np.bincount(grp, minlength=K).astype(np.int64)


def host_stats(rank2_sum, tie_sum, n_cells):
    """``(U, auc, z, p)`` f64 [K, G], every element on its own in Python floats."""
    K, G = np.asarray(rank2_sum).shape
    N = int(np.asarray(n_cells).sum())
    U, auc, z, p = (np.full((K, G), np.nan) for _ in range(4))
    for k in range(K):
        n1 = int(n_cells[k])
        n2 = N - n1
        for g in range(G):
            u = (int(rank2_sum[k, g]) - n1 * (n1 + 1)) / 2.0
            U[k, g] = u
            if n1 == 0 or n2 == 0:
                continue
            mu = (n1 * n2) / 2.0
            var = (n1 * n2) / 12.0 * ((N + 1) - int(tie_sum[g]) / (N * (N - 1.0)))
            if var == 0:
                z[k, g], p[k, g], auc[k, g] = 0.0, 1.0, 0.5
                continue
            z[k, g] = (u - mu) / math.sqrt(var)
            p[k, g] = 2 * float(ndtr(-abs(z[k, g])))
            auc[k, g] = u / (n1 * n2)
    return U, auc, z, p


def benjamini_hochberg(p):
    """One vector's Benjamini-Hochberg adjusted p-values, by the definition: min over j >= i (in ascending order) of p_j * m / j."""
    p = np.asarray(p, np.float64)
    order = np.argsort(p, kind="stable")
    m = len(p)
    out = np.empty(m)
    for pos, i in enumerate(order):
        out[i] = min(1.0, min(p[order[j]] * m / (j + 1) for j in range(pos, m)))
    return out


def csr_of(dense_mask, values):
    """A cell-major CSR (rowptr int64, col int32, val f32) of the entries ``dense_mask`` marks, a cell's genes ascending."""
    rows, cols = np.nonzero(dense_mask)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=dense_mask.shape[0]))]).astype(np.int64)
    return rowptr, cols.astype(np.int32), np.asarray(values, np.float32)[rows, cols]


def column_case(n_cells: int, lengths, n_genes: int, seed: int, tied_gene=None):
    """``n_cells`` cells x ``n_genes`` genes; gene ``g`` is stored by ``lengths[g % len(lengths)]`` random cells.  Tie-heavy
    values: ``log1p`` of small integers; ``tied_gene``: that gene's entries all hold one value."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((n_cells, n_genes), bool)
    for g in range(n_genes):
        mask[rng.choice(n_cells, size=lengths[g % len(lengths)], replace=False), g] = True
    values = np.log1p(rng.integers(1, 6, size=mask.shape)).astype(np.float32)
    if tied_gene is not None:
        values[:, tied_gene] = np.float32(np.log1p(3.0))
    return csr_of(mask, values)


def edge_case(seed: int = 0):
    """600 cells x 40 genes with the gene lengths ``GENE_LENGTHS`` (each at least three times)."""
    return column_case(600, GENE_LENGTHS, 40, seed)


def slab_case(seed: int = 1):
    """17 000 cells x 6 genes around the 16 384-key slab: 16 384, 16 385 and 17 000 stored entries, one gene (of 16 385) whose
    entries all tie, and two short ones."""
    return column_case(17000, (16384, 16385, 17000, 16385, 100, 0), 6, seed, tied_gene=3)


def groups_of(n_cells: int, n_groups: int, seed: int, skip: float = 0.1):
    """One group per cell in ``[0, K)`` with a share ``skip`` of the cells at -1; with three or more groups, group 1 is empty
    and group 2 holds exactly one cell."""
    rng = np.random.default_rng(seed)
    K = int(n_groups)
    group = rng.integers(0, K, size=n_cells).astype(np.int64)
    if K >= 3:
        group[(group == 1) | (group == 2)] = 0
        group[rng.integers(0, n_cells)] = 2
    group[rng.random(n_cells) < skip] = -1
    if K >= 3 and not (group == 2).any():
        group[0] = 2
    return group
