"""A plain numpy / Python-int restatement of ``ops.snn_graph`` and ``ops.louvain_graph`` (``include/wgnn.h`` has the contract),
written from the specification and independent of the device code.

The graph: the union graph of ``[B, k]`` neighbour lists (-1 = none) as a symmetric CSR, weighted by shared-neighbour counts
``|N+(i) & N+(j)|`` with ``N+(i) = {i} | list(i)``, or by 1.

The clustering: a synchronous Louvain whose every decision compares integers.  With ``resolution = num / den`` and ``M`` the sum of
all stored weights, a vertex ``v`` scores a community ``C`` of its neighbours

    score(C) = kin[C] * M * den - num * deg[v] * (tot[C] - (C == own ? deg[v] : 0))

and, in sweep ``t``, moves to the best ``C != own`` (higher score, then lower id) that passes the direction gate (``C < own`` for even
``t``, ``C > own`` for odd), is no swap of two singletons upwards, and scores above ``score(own)``.  All vertices read the state
before the sweep.  A sweep that moved something but did not raise ``Qnum = den * M * IN - num * sum_c tot[c]^2`` is discarded and
only its single best move (largest gain, lowest vertex) is applied.  A level ends after two consecutive sweeps without a move;
communities become the vertices of the next level until a level merges nothing.

``gain_dtype=np.float64`` evaluates the scores in double precision instead: the variant the 64-bit test shows to differ.
"""
from fractions import Fraction
from typing import NamedTuple

import numpy as np


def snn_graph(idx, weights="snn"):
    """``(rowptr int64 [B + 1], col int32, w int32)`` of the neighbour lists ``idx`` [B, k]."""
    idx = np.asarray(idx, np.int64)
    B, k = idx.shape
    if weights not in ("snn", "unit"):
        raise ValueError(weights)
    src = np.repeat(np.arange(B, dtype=np.int64), k)
    dst = idx.ravel()
    ok = (dst >= 0) & (dst != src)
    src, dst = src[ok], dst[ok]
    keys = np.unique(np.concatenate([src * B + dst, dst * B + src]))
    row, col = keys // B, keys % B
    rowptr = np.zeros(B + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=B), out=rowptr[1:])
    if weights == "unit":
        return rowptr, col.astype(np.int32), np.ones(len(col), np.int32)
    sets = [set(int(j) for j in idx[i] if j >= 0) | {i} for i in range(B)]
    w = np.array([len(sets[int(i)] & sets[int(j)]) for i, j in zip(row, col)], np.int32).reshape(-1)
    return rowptr, col.astype(np.int32), w


def resolution_fraction(resolution) -> Fraction:
    frac = Fraction(resolution).limit_denominator(64)
    if frac <= 0:
        raise ValueError(f"resolution = {resolution} must be positive")
    return frac


def guard(M: int, frac: Fraction) -> None:
    if M * M * max(frac.numerator, frac.denominator) >= 2 ** 62:
        raise ValueError(f"M * M * max(num, den) = {M * M * max(frac.numerator, frac.denominator)} >= 2^62: the integer gains "
                         "would not fit 64 bits")


def _rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def qnum(row, col, w, comm, deg, M: int, frac: Fraction) -> int:
    inside = int(w[comm[row] == comm[col]].sum())
    tot = np.zeros(len(comm), np.int64)
    np.add.at(tot, comm, deg)
    return frac.denominator * M * inside - frac.numerator * sum(int(t) * int(t) for t in tot[tot > 0])


def sweep(row, col, w, comm, deg, tot, size, M: int, frac: Fraction, t: int, gain_dtype=np.int64):
    """One synchronous sweep on the state ``(comm, tot, size)``: ``(next, gain)`` - the community every vertex moves to (its own
    when it stays) and ``score(next) - score(own)`` (0 when it stays)."""
    n = len(comm)
    num, den = frac.numerator, frac.denominator
    off = row != col
    r, cu, ww = row[off], comm[col[off]], w[off].astype(np.int64)
    nxt, gain = comm.copy(), np.zeros(n, gain_dtype)
    if len(r) == 0:
        return nxt, gain
    key = r * n + cu
    order = np.argsort(key, kind="stable")
    key, ww = key[order], ww[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    kin = np.add.reduceat(ww, first)
    v, C = key[first] // n, key[first] % n
    own = comm[v]
    kin_own = np.zeros(n, np.int64)
    kin_own[v[C == own]] = kin[C == own]
    T = gain_dtype
    mden = T(M * den) if T is np.int64 else T(M) * T(den)
    s_own = kin_own.astype(T) * mden - T(num) * deg.astype(T) * (tot[comm] - deg).astype(T)
    s = kin.astype(T) * mden - T(num) * deg[v].astype(T) * tot[C].astype(T)
    ok = (C != own) & ((C < own) if t % 2 == 0 else (C > own))
    ok &= ~((size[own] == 1) & (size[C] == 1) & (C > own))
    ok &= s > s_own[v]
    v, C, s = v[ok], C[ok], s[ok]
    if len(v) == 0:
        return nxt, gain
    order = np.lexsort((C, -s, v))                     # per vertex: higher score, then lower id
    v, C, s = v[order], C[order], s[order]
    top = np.concatenate([[True], v[1:] != v[:-1]])
    nxt[v[top]] = C[top]
    gain[v[top]] = s[top] - s_own[v[top]]
    return nxt, gain


def aggregate(row, col, w, comm):
    """The communities as vertices, renumbered densely in ascending order of their ids: ``(dense id per vertex, rowptr, col, w)``
    with the internal weights of a community on its diagonal."""
    uniq, inv = np.unique(comm, return_inverse=True)
    nc = len(uniq)
    key = inv[row] * nc + inv[col]
    order = np.argsort(key, kind="stable")
    key, ww = key[order], w[order].astype(np.int64)
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    sums = np.add.reduceat(ww, first) if len(key) else np.zeros(0, np.int64)
    r, c = key[first] // nc, key[first] % nc
    rowptr = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=nc), out=rowptr[1:])
    return inv.astype(np.int64), rowptr, c.astype(np.int64), sums


class Louvain(NamedTuple):
    cluster: np.ndarray
    level_labels: list
    levels: list
    qnum_trace: list
    modularity: float
    resolution: Fraction
    M: int
    converged: bool


def final_clusters(label, isolated):
    """Ids by descending size, ties by the lowest member index; -1 for an isolated vertex."""
    out = np.full(len(label), -1, np.int64)
    on = ~isolated
    if on.any():
        uniq, first, inv, count = np.unique(label[on], return_index=True, return_inverse=True, return_counts=True)
        first = np.flatnonzero(on)[first]
        order = np.lexsort((first, -count))
        rank = np.empty(len(uniq), np.int64)
        rank[order] = np.arange(len(uniq))
        out[on] = rank[inv]
    return out


def louvain_graph(rowptr, col, w, resolution=1.0, max_sweeps=256, gain_dtype=np.int64) -> Louvain:
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.int64)
    frac = resolution_fraction(resolution)
    B = len(rowptr) - 1
    M = int(w.sum())
    guard(M, frac)
    isolated = np.diff(rowptr) == 0
    member = np.arange(B, dtype=np.int64)              # the current level's vertex of every original vertex
    if M == 0:
        return Louvain(np.full(B, -1, np.int64), [member.copy()], [dict(vertices=B, communities=B, sweeps=0, fallback_moves=0)],
                       [0], 0.0, frac, 0, True)
    row = _rows(rowptr)
    trace, levels, level_labels, converged = None, [], [], True
    while True:
        n = len(rowptr) - 1
        deg = np.zeros(n, np.int64)
        np.add.at(deg, row, w)
        comm, tot, size = np.arange(n, dtype=np.int64), deg.copy(), np.ones(n, np.int64)
        if trace is None:
            trace = [qnum(row, col, w, comm, deg, M, frac)]
        t = idle = fallback = 0
        while True:
            if t >= max_sweeps:
                converged = False
                break
            nxt, gain = sweep(row, col, w, comm, deg, tot, size, M, frac, t, gain_dtype)
            t += 1
            if not (nxt != comm).any():
                idle += 1
                if idle == 2:
                    break
                continue
            idle = 0
            q = qnum(row, col, w, nxt, deg, M, frac)
            if q > trace[-1]:
                comm = nxt
            else:                                      # discarded: the single best move of the sweep
                v = int(np.argmax(gain))               # the first of equal gains: the lowest vertex
                comm = comm.copy()
                comm[v] = nxt[v]
                q = qnum(row, col, w, comm, deg, M, frac)
                assert q > trace[-1], "a single positive-gain move must raise Qnum"
                fallback += 1
            trace.append(q)
            tot = np.zeros(n, np.int64)
            np.add.at(tot, comm, deg)
            size = np.bincount(comm, minlength=n).astype(np.int64)
        inv, c_rowptr, c_col, c_w = aggregate(row, col, w, comm)
        nc = len(c_rowptr) - 1
        member = inv[member]
        levels.append(dict(vertices=n, communities=nc, sweeps=t, fallback_moves=fallback))
        level_labels.append(member.copy())
        if nc == n:
            break
        rowptr, col, w = c_rowptr, c_col, c_w
        row = _rows(rowptr)
    return Louvain(final_clusters(member, isolated), level_labels, levels, trace, trace[-1] / (frac.denominator * M * M), frac, M,
                   converged)


def blobs(B, D, n_blobs, spread, seed, centre_scale=1.0):
    """``B`` points in ``D`` dimensions around ``n_blobs`` Gaussian centres (``spread`` = the centres' scale over the blobs' unit
    spread; 0 = structureless)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(n_blobs, D)) * spread * centre_scale
    return (centres[rng.integers(0, n_blobs, B)] + rng.normal(size=(B, D))).astype(np.float32)


def knn_lists(x, k):
    """Exact k nearest neighbours by ascending (squared distance, index), the row itself left out: int64 [B, k]."""
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) if len(x) <= 512 else \
        (x * x).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * x @ x.T
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)
