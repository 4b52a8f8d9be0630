"""numpy restatement of the MERGING log-normalising alignment (``wgnn_align_count_ln_merge`` / ``wgnn_align_fill_ln_merge``,
``ResidentPredictor.align`` with a ``GeneMap``), written from the contract in ``include/wgnn.h`` - a helper for the CPU and GPU
tests, not a test module.

    a group = the columns that name one bundle gene (two or more); col_group[j] = the group of column j, or -1
    total[r] = sum over ALL j of float64(x[r, j])                        (members like any other column)
    c        = sum over the group's members that count (finite, > 0), in the row's INPUT order, of float64(x[r, j])
    v        = float32(log1p(c / total[r] * scale))
    one entry (gene, v) is kept iff c > 0 and v > threshold, at the place of the first counting member; every later member
    leaves nothing.  A column that is alone: ``lognorm_reference`` exactly.

Everything is fp64 and plain loops.  The comparison a test may ask is ``lognorm_reference``'s: the counts of the cases here are
float32 multiples of 2^-10 below 2^15 (``merge_case(integer=False)``) or integers below 2^24, a row has under a thousand of them,
so every partial sum is a multiple of 2^-10 below 2^25 - 35 bits, exact in fp64 in any order: totals and merged counts agree bit for bit,
and a value differs only where ``lognorm_reference.fragile`` says the rounding to float32 may.
"""
from types import SimpleNamespace

import numpy as np

from lognorm_reference import _row_total, _value


def group_tables(gene_map):
    """(col_group int32 [n_cols], group_ptr int32 [n_groups + 1], group_cols int32) of a map with repeated ids: the tables the
    contract describes, groups by ascending gene id, members ascending - built by a plain loop."""
    gene_map = np.asarray(gene_map, np.int32)
    members = {}
    for j, g in enumerate(gene_map):
        if g >= 0:
            members.setdefault(int(g), []).append(j)
    col_group = np.full(len(gene_map), -1, np.int32)
    ptr, cols = [0], []
    for g in sorted(members):
        if len(members[g]) > 1:
            col_group[members[g]] = len(ptr) - 1
            cols += members[g]
            ptr.append(len(cols))
    return col_group, np.asarray(ptr, np.int32), np.asarray(cols, np.int32)


def _merge_row(cols, vals, gene_map, col_group, total, thr, scale, out_col, v64):
    """One row's entries (column, count) in input order."""
    done = set()
    for i, (j, x) in enumerate(zip(cols, vals)):
        g = gene_map[j]
        if not (total > 0 and g >= 0 and x > 0):
            continue
        s = col_group[j]
        if s < 0:
            c = float(x)
        else:
            if s in done:                                               # a later member: nothing
                continue
            done.add(s)                                                 # the first counting member: the group's entry
            c = 0.0
            for jj, xx in zip(cols[i:], vals[i:]):
                if col_group[jj] == s and xx > 0:
                    c += float(xx)
        v = _value(c, total, scale)
        if np.float32(v) > thr:
            out_col.append(g); v64.append(v)


def merge_dense(x, gene_map, col_group, threshold, scale=1e4, library_size=None, fp64=False):
    """(rowptr int64 [B+1], col int32, v float32) of a dense [B, n_cols] count matrix; with ``fp64`` also the kept values before
    their rounding to float32."""
    x = np.asarray(x, np.float32)
    thr = np.float32(threshold)
    rowptr, col, v64 = [0], [], []
    cols = list(range(x.shape[1]))
    for r in range(x.shape[0]):
        total = _row_total(x[r], library_size, r)
        _merge_row(cols, list(x[r]), gene_map, col_group, total, thr, scale, col, v64)
        rowptr.append(len(col))
    out = (np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(v64, np.float64).astype(np.float32))
    return out + (np.asarray(v64, np.float64),) if fp64 else out


def merge_csr(rowptr, col, val, gene_map, col_group, threshold, scale=1e4, library_size=None, fp64=False):
    """The same for a CSR over the caller's columns: input order = stored order, whatever the column ids say."""
    rowptr = np.asarray(rowptr, np.int64)
    val = np.asarray(val, np.float32)
    thr = np.float32(threshold)
    out_ptr, out_col, v64 = [0], [], []
    for r in range(len(rowptr) - 1):
        b, e = rowptr[r], rowptr[r + 1]
        total = _row_total(val[b:e], library_size, r)
        _merge_row(list(col[b:e]), list(val[b:e]), gene_map, col_group, total, thr, scale, out_col, v64)
        out_ptr.append(len(out_col))
    out = (np.asarray(out_ptr, np.int64), np.asarray(out_col, np.int32), np.asarray(v64, np.float64).astype(np.float32))
    return out + (np.asarray(v64, np.float64),) if fp64 else out


def premerge_dense(x, col_group):
    """The host route: a float32 matrix with each group's sum at the row's first counting member and zeros at the other
    members (the sum is taken in fp64 and must be exact in float32 - integer counts below 2^24)."""
    x = np.asarray(x, np.float32)
    out = x.copy()
    for s in range(int(col_group.max()) + 1):
        cols = np.flatnonzero(col_group == s)
        for r in range(x.shape[0]):
            on = cols[x[r, cols] > 0]
            if len(on):
                c = float(np.sum(x[r, on].astype(np.float64)))
                assert c == float(np.float32(c)) and c < 2 ** 24
                out[r, cols] = 0
                out[r, on[0]] = c
    return out


def premerge_csr(rowptr, col, val, col_group):
    """The same for a CSR in stored order: the sum at the row's first counting member ENTRY, explicit zeros at the others."""
    val = np.asarray(val, np.float32)
    out = val.copy()
    for r in range(len(rowptr) - 1):
        first = {}
        for k in range(rowptr[r], rowptr[r + 1]):
            s = col_group[col[k]]
            if s < 0 or not val[k] > 0:
                continue
            if s in first:
                c = float(out[first[s]]) + float(val[k])
                assert c == float(np.float32(c)) and c < 2 ** 24
                out[first[s]] = c
                out[k] = 0
            else:
                first[s] = k
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
# rows of merge_case that hold the corners
ROW_EMPTY, ROW_NO_MEMBER, ROW_FIRST_ZERO, ROW_JOINT, ROW_ALL_MEMBERS = 0, 1, 2, 3, 4
# its groups, by the columns they occupy (n_cols >= 700): two members in one float4 (one lane of the 16-byte form), in
# different 64-entry steps, in different 256-entry chunks, five members, one group that is zero in every row
GROUP_QUAD, GROUP_STEPS, GROUP_CHUNKS, GROUP_FIVE, GROUP_ZERO = (8, 9), (20, 100), (30, 300, 600), (5, 70, 140, 400, 690), (50, 500)
FIXED_GROUPS = (GROUP_QUAD, GROUP_STEPS, GROUP_CHUNKS, GROUP_FIVE, GROUP_ZERO)
JOINT_TOTAL, JOINT_COUNT, JOINT_THRESHOLD = 20000, 1, 0.5       # log1p(1 / 20000 * 1e4) = 0.405 < 0.5 < log1p(2 * 0.5) = 0.693


def merge_case(seed, B, n_cols, n_genes, n_random_groups=6, density=0.3, integer=True):
    """A dense batch of counts over a map with groups: the fixed layouts above, ``n_random_groups`` more of 2-3 random columns,
    and the corner rows: ROW_EMPTY all zero; ROW_NO_MEMBER counts on columns that are alone only; ROW_FIRST_ZERO every group's
    first member zero while a later one counts; ROW_JOINT (total JOINT_TOTAL) GROUP_QUAD's members both JOINT_COUNT, which
    passes JOINT_THRESHOLD only jointly; ROW_ALL_MEMBERS every member of every group but GROUP_ZERO counts.  ``integer``: Poisson draws; else float32 multiples of 2^-10 spread over the binades
    2^-10 .. 2^11."""
    assert B >= 8 and n_cols >= 700 and n_genes >= n_cols
    rng = np.random.default_rng(seed)
    gene_map = rng.permutation(n_genes)[:n_cols].astype(np.int32)
    gene_map[rng.random(n_cols) < 0.2] = -1
    fixed = sorted({j for grp in FIXED_GROUPS for j in grp})
    free = np.setdiff1d(np.arange(n_cols), fixed)
    groups = [list(g) for g in FIXED_GROUPS]
    pick = rng.permutation(free)
    for _ in range(n_random_groups):
        k = int(rng.integers(2, 4))
        groups.append(sorted(pick[:k].tolist()))
        pick = pick[k:]
    alone = np.asarray(sorted(pick.tolist()))
    spare = np.setdiff1d(np.arange(n_genes), gene_map[alone])
    for i, grp in enumerate(groups):
        gene_map[grp] = spare[i]                                        # one gene per group, named by no other column
    col_group, group_ptr, group_cols = group_tables(gene_map)
    on = rng.random((B, n_cols)) < density
    if integer:
        x = np.where(on, rng.poisson(3.0, (B, n_cols)) + 1, 0).astype(np.float32)
    else:
        x = np.where(on, rng.integers(1, 2048, (B, n_cols)) * 2.0 ** rng.integers(-10, 1, (B, n_cols)), 0).astype(np.float32)
    members = np.flatnonzero(col_group >= 0)
    x[5:, members[::2]] = np.where(rng.random((B - 5, len(members[::2]))) < 0.7, x[5:, members[::2]] + 1, 0)   # groups often meet
    x[ROW_ALL_MEMBERS, members] += 1
    x[:, list(GROUP_ZERO)] = 0
    x[ROW_EMPTY] = 0
    x[ROW_NO_MEMBER, members] = 0
    for grp in groups:
        if tuple(grp) != GROUP_ZERO:
            x[ROW_FIRST_ZERO, grp[0]] = 0
            x[ROW_FIRST_ZERO, grp[-1]] = 2
    x[ROW_JOINT] = 0
    x[ROW_JOINT, list(GROUP_QUAD)] = JOINT_COUNT
    x[ROW_JOINT, alone[gene_map[alone] < 0][0]] = JOINT_TOTAL - 2 * JOINT_COUNT
    x[ROW_JOINT, alone[gene_map[alone] >= 0][0]] = 0
    return SimpleNamespace(x=x, gene_map=gene_map, col_group=col_group, group_ptr=group_ptr, group_cols=group_cols,
                           n_genes=n_genes, B=B, n_cols=n_cols, groups=groups)


def shuffled_csr(x, seed):
    """The stored form of a count matrix with every row's entries in a random order (explicit zeros: none)."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float32)
    rowptr, col, val = [0], [], []
    for row in x:
        j = rng.permutation(np.flatnonzero(row != 0))
        col += j.tolist(); val += row[j].tolist()
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(val, np.float32)
