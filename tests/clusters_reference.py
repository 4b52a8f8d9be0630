"""fp64 restatement of the per-cluster class tables (``wgnn_group_class_reduce`` / ``ResidentPredictor.annotate``), written
from the contract in ``include/wgnn.h`` in plain loops - a helper for the CPU and GPU tests, not a test module.

Per cell, all in fp64 from the f32 logits l_j:

    m = max_j l_j,  e_j = exp(l_j - m),  Z = sum_j e_j,  p_j = e_j / Z,  conf = max_j p_j = 1 / Z

(``math.exp``, ``math.fsum`` for Z).  A cell is BAD if its logits hold a NaN or a +inf or are all -inf: it is counted in
``tally[k][2]`` and in nothing else.  Over the cells of group k that are not bad, each bin summed with ``math.fsum`` (the exact
sum of its terms, rounded once):

    prob_sum[k, j] = sum p_ij      conf_sum[k] = sum conf_i      votes[k, j] = cells with label j
    tally[k] = (cells that take part, cells with label -1, bad cells)

A cell whose group is outside [0, K) or whose label is outside [-1, C) takes no part at all.

Bound of a device sum against this one (derived, not measured; ``bound``).  u = 2^-52.  Per term: the f32 logits and
l_j - m are exact in fp64 or rounded once (u/2); exp is within 1 ulp (u) of the exact value and amplifies the argument's
rounding by at most |l_j - m| u/2 <= 2^-44 relative for f32 logits that do not underflow - counted as one more u; Z is a sum of
C non-negative terms, (C - 1) u in any order, plus the terms' own 2 u; the divide adds u/2.  Together a term p_ij is within
(C + 5) u of the exact p_ij, and so is the reference's own (its Z is rounded once instead: this side is < 4 u).  A bin adds
n_k non-negative terms in SOME order: at most (n_k - 1) u/2 relative to the sum.  Non-negative terms make every relative
error carry to the sum unamplified, hence

    |got - want| <= (n_k + C + 8) 2^-52 |want| + 2^-1074

with the last term for sums in the denormals.  One f32 step anywhere in the chain is an error of ~2^-24: 2^28 times the bound.

On LATTICE cases every row holds 0.0 on m classes, m a power of two, and -1000.0 or -inf elsewhere: exp is exactly 1 or 0
(exp(-1000) underflows to 0 in fp64), Z = m, p = 1/m or 0, and every partial sum of a bin is a multiple of 2^-6 far below
2^53 * 2^-6: exact in fp64 in any order, so the device must match bit for bit.
"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -52
TINY = 2.0 ** -1074


def cell(logits):
    """(p list [C], conf) of one cell in fp64, or None for a bad cell."""
    ls = [float(v) for v in logits]
    if any(math.isnan(v) or v == math.inf for v in ls):
        return None
    m = max(ls)
    if m == -math.inf:
        return None
    e = [math.exp(v - m) for v in ls]
    z = math.fsum(e)
    p = [v / z for v in e]
    return p, max(p)


def reduce(logits, label, group, n_groups):
    """(prob_sum f64 [K, C], conf_sum f64 [K], votes int32 [K, C], tally int32 [K, 3]) by plain loops and ``math.fsum``.
    ``logits`` [B, >= C] is read over its first C = ``logits.shape[1]`` columns: slice it before the call."""
    logits = np.asarray(logits, np.float32)
    B, C = logits.shape
    K = int(n_groups)
    terms = [[[] for _ in range(C)] for _ in range(K)]
    confs = [[] for _ in range(K)]
    votes = np.zeros((K, C), np.int32)
    tally = np.zeros((K, 3), np.int32)
    for i in range(B):
        k, lab = int(group[i]), int(label[i])
        if not 0 <= k < K or not -1 <= lab < C:
            continue
        got = cell(logits[i])
        if got is None:
            tally[k, 2] += 1
            continue
        p, conf = got
        for j in range(C):
            terms[k][j].append(p[j])
        confs[k].append(conf)
        tally[k, 0] += 1
        if lab < 0:
            tally[k, 1] += 1
        else:
            votes[k, lab] += 1
    prob_sum = np.array([[math.fsum(t) for t in row] for row in terms], np.float64).reshape(K, C)
    conf_sum = np.array([math.fsum(c) for c in confs], np.float64)
    return prob_sum, conf_sum, votes, tally


def bound(want, n_cells, n_classes):
    """The derived bound of the module header for ``want`` [K] or [K, C] with ``n_cells`` [K]."""
    n = np.asarray(n_cells, np.float64)
    n = n[:, None] if np.ndim(want) == 2 else n
    return (n + n_classes + 8.0) * U * np.abs(want) + TINY


def consensus(prob_sum, votes, tally, unsure_rate, rule="vote", min_fraction=0.0):
    """Host restatement of ``ClusterCalls.consensus``: (ids int64 [K], confidence f64 [K]) by plain loops."""
    K, C = votes.shape
    ids, conf = np.zeros(K, np.int64), np.zeros(K)
    for k in range(K):
        n, unsure = int(tally[k, 0]), int(tally[k, 1])
        if n == 0:
            ids[k], conf[k] = -2, math.nan
            continue
        if rule == "vote":
            win = max(range(C), key=lambda j: (int(votes[k, j]), -j))
            conf[k] = int(votes[k, win]) / n
            ids[k] = -1 if unsure > int(votes[k, win]) or conf[k] < min_fraction else win
        elif rule == "mean_prob":
            win = max(range(C), key=lambda j: (float(prob_sum[k, j]), -j))
            conf[k] = float(prob_sum[k, win]) / n
            ids[k] = -1 if conf[k] < float(np.float32(unsure_rate / C)) else win
        else:
            raise ValueError(rule)
    return ids, conf


# ------------------------------------------------------------------------------------------------
# the operands of the GPU tests (built here so that the CPU suite can assert their premises)
# ------------------------------------------------------------------------------------------------
def _groups_and_labels(rng, B, C, K):
    """~15 % of the cells in group -1, group K // 2 without a cell (K >= 3), ~20 % of the labels -1."""
    group = rng.integers(0, K, B).astype(np.int32)
    group[rng.random(B) < 0.15] = -1
    if K >= 3:
        group[group == K // 2] = -1
    label = rng.integers(0, C, B).astype(np.int32)
    label[rng.random(B) < 0.2] = -1
    return group, label


def lattice_case(B, C, K, seed=None):
    """Row i: 0.0 on m_i classes, m_i a power of two <= C drawn per row, elsewhere -1000.0 (even rows) or -inf (odd rows)."""
    rng = np.random.default_rng(seed if seed is not None else 10007 * B + 101 * C + K)
    logits = np.empty((B, C), np.float32)
    powers = [1 << s for s in range(C.bit_length()) if (1 << s) <= C]
    for i in range(B):
        logits[i] = -1000.0 if i % 2 == 0 else -np.inf
        logits[i, rng.choice(C, size=int(rng.choice(powers)), replace=False)] = 0.0
    group, label = _groups_and_labels(rng, B, C, K)
    return SimpleNamespace(B=B, C=C, K=K, logits=logits, group=group, label=label)


def random_case(B, C, K, seed=None):
    """N(0, 3) logits."""
    rng = np.random.default_rng(seed if seed is not None else 20011 * B + 103 * C + K)
    group, label = _groups_and_labels(rng, B, C, K)
    return SimpleNamespace(B=B, C=C, K=K, logits=(3.0 * rng.standard_normal((B, C))).astype(np.float32), group=group, label=label)


# about a dozen (B, C, K) that cover every value of B in 0, 1, 63, 64, 65, 1500, C in 1, 2, 5, 16, 17, 64, 65, 80 and K in
# 1, 3, 200; with K = 1 or 3 and B = 1500 a group spans at least three of the kernel's 256-cell chunks
CASES = [(0, 16, 3), (1, 1, 1), (63, 2, 3), (64, 5, 1), (65, 17, 200), (1500, 16, 3), (1500, 64, 1), (1500, 65, 200),
         (65, 80, 3), (1500, 80, 3), (64, 64, 200), (1500, 1, 3), (63, 65, 1)]
SPECIAL = ("empty_group", "one_group_holds_all", "all_skipped", "one_cell_group", "three_chunks")


def special(name):
    if name == "empty_group":                            # group 1 of 3 without a cell
        c = lattice_case(300, 16, 3, seed=1)
        c.group[c.group == 1] = 0
    elif name == "one_group_holds_all":
        c = lattice_case(700, 5, 3, seed=2)
        c.group[:] = 2
    elif name == "all_skipped":
        c = lattice_case(130, 17, 3, seed=3)
        c.group[:] = -1
    elif name == "one_cell_group":
        c = lattice_case(200, 16, 3, seed=4)
        c.group[c.group == 1] = 0
        c.group[77] = 1
    elif name == "three_chunks":                         # 3 * 256 + 1 cells in one group: four chunks, the last with one cell
        c = lattice_case(900, 16, 3, seed=5)
        c.group[:] = -1
        c.group[100:100 + 3 * 256 + 1] = 1
    else:
        raise KeyError(name)
    return c
