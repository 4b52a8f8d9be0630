"""A plain numpy / Python-int restatement of ``ops.leiden_graph`` (``include/wgnn.h`` and DESIGN.md section 3 have the
contract), written from the specification and independent of the device code.  It is a deterministic, synchronous, integer Leiden:
``louvain_reference``'s moving phase from a start partition, a refinement that merges singletons inside every community of the
moving phase's partition ``P``, an aggregation by the refined partition, and a final cut of the last ``P`` into its connected
components.  ``resolution = num / den``, ``M``, ``m_den = M * den``, ``deg`` and ``Qnum`` are ``louvain_graph``'s.

The refinement of a level starts from ``ref = identity``.  In sweep ``r``, from the state before it:

    tot_r[S], size_r[S]   the sum of deg and the count over ref == S
    ext[S]                the stored off-diagonal weight from ref == S into the rest of its P-community
    kinP[v]               the off-diagonal weight from v into its P-community

``v`` may move iff it is alone (``size_r[ref[v]] == 1``) and well connected (``kinP[v] * m_den >= num * deg[v] * (totP[P[v]] -
deg[v])``).  It scores ``S`` by ``kin[S] * m_den - num * deg[v] * tot_r[S]`` (``kin`` over its neighbours in the same P-community)
and proposes the best ``S != ref[v]`` (higher score, lower id) that passes the gate (``S < ref[v]`` for even ``r``, above for
odd), is well connected itself (``ext[S] * m_den >= num * tot_r[S] * (totP[P[v]] - tot_r[S])``) and scores above 0.  A proposal is
accepted iff the vertex whose id is the target's label proposes to stay.  A sweep whose accepted moves do not raise ``Qnum`` is
discarded for its single best accepted move (largest gain, lowest vertex).
"""
from fractions import Fraction
from typing import NamedTuple

import numpy as np

from louvain_reference import _rows, aggregate, final_clusters, guard, qnum, resolution_fraction, sweep


def boundary(row, col, w, P, ref):
    """``(ext, kinP)`` of the state ``(P, ref)``."""
    n = len(P)
    same = (row != col) & (P[row] == P[col])
    kinP = np.zeros(n, np.int64)
    np.add.at(kinP, row[same], w[same])
    out = same & (ref[row] != ref[col])
    ext = np.zeros(n, np.int64)
    np.add.at(ext, ref[row[out]], w[out])
    return ext, kinP


def refine_sweep(row, col, w, P, ref, deg, totP, tot_r, size_r, ext, kinP, M: int, frac: Fraction, r: int):
    """One refinement sweep: ``(prop, gain)`` - the refined community every vertex proposes to join (its own when it stays) and the
    proposal's score (0 when it stays).  Python ints throughout."""
    n = len(P)
    num, mden = frac.numerator, M * frac.denominator
    prop, gain = ref.copy(), np.zeros(n, np.int64)
    start = np.searchsorted(row, np.arange(n + 1))             # the rows are stored in order
    for v in range(n):
        dv, own, tp = int(deg[v]), int(ref[v]), int(totP[P[v]])
        if size_r[own] != 1 or int(kinP[v]) * mden < num * dv * (tp - dv):
            continue
        kin = {}
        for e in range(start[v], start[v + 1]):
            u = int(col[e])
            if u != v and P[u] == P[v]:
                kin[int(ref[u])] = kin.get(int(ref[u]), 0) + int(w[e])
        best = None
        for S, k in kin.items():
            if S == own or (S > own if r % 2 == 0 else S < own):
                continue
            ts = int(tot_r[S])
            if int(ext[S]) * mden < num * ts * (tp - ts):
                continue
            s = k * mden - num * dv * ts
            if s > 0 and (best is None or s > best[0] or (s == best[0] and S < best[1])):
                best = (s, S)
        if best is not None:
            gain[v], prop[v] = best
    return prop, gain


def accept(ref, prop, gain):
    """``(next, gain)``: a proposal holds iff the founder of its target stays at home."""
    ok = prop[prop] == prop
    return np.where(ok, prop, ref), np.where(ok, gain, 0)


def _state(comm, deg):
    n = len(comm)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, comm, deg)
    return tot, np.bincount(comm, minlength=n).astype(np.int64)


def move(row, col, w, comm, deg, M, frac, trace, max_sweeps):
    """``louvain_graph``'s sweep loop from the partition ``comm``: ``(P, sweeps, fallback moves, converged)``; ``trace`` grows."""
    tot, size = _state(comm, deg)
    t = idle = fallback = 0
    while True:
        if t >= max_sweeps:
            return comm, t, fallback, False
        nxt, gain = sweep(row, col, w, comm, deg, tot, size, M, frac, t)
        t += 1
        if not (nxt != comm).any():
            idle += 1
            if idle == 2:
                return comm, t, fallback, True
            continue
        idle = 0
        q = qnum(row, col, w, nxt, deg, M, frac)
        if q > trace[-1]:
            comm = nxt
        else:
            v = int(np.argmax(gain))
            comm = comm.copy()
            comm[v] = nxt[v]
            q = qnum(row, col, w, comm, deg, M, frac)
            assert q > trace[-1], "a single positive-gain move must raise Qnum"
            fallback += 1
        trace.append(q)
        tot, size = _state(comm, deg)


def refine(row, col, w, P, deg, M, frac, max_sweeps, states=None):
    """The refinement of ``P``: ``(ref, sweeps, fallback moves, converged)``.  ``states`` collects what every sweep read and left."""
    n = len(P)
    totP, _ = _state(P, deg)
    ref = np.arange(n, dtype=np.int64)
    running = qnum(row, col, w, ref, deg, M, frac)
    r = idle = fallback = 0
    while True:
        if r >= max_sweeps:
            return ref, r, fallback, False
        tot_r, size_r = _state(ref, deg)
        ext, kinP = boundary(row, col, w, P, ref)
        prop, gain = refine_sweep(row, col, w, P, ref, deg, totP, tot_r, size_r, ext, kinP, M, frac, r)
        nxt, kept = accept(ref, prop, gain)
        if states is not None:
            states.append(dict(r=r, P=P, ref=ref, totP=totP, tot_r=tot_r, size_r=size_r, ext=ext, kinP=kinP, prop=prop, gain=gain,
                               next=nxt, kept=kept))
        r += 1
        if not (nxt != ref).any():
            idle += 1
            if idle == 2:
                return ref, r, fallback, True
            continue
        idle = 0
        q = qnum(row, col, w, nxt, deg, M, frac)
        if q > running:
            ref = nxt
        else:
            v = int(np.argmax(kept))
            ref = ref.copy()
            ref[v] = nxt[v]
            q = qnum(row, col, w, ref, deg, M, frac)
            assert q > running, "a single accepted move must raise Qnum"
            fallback += 1
        running = q


def components(row, col, P):
    """The lowest vertex of every vertex's connected component inside its P-community (min-label propagation)."""
    label = np.arange(len(P), dtype=np.int64)
    same = P[row] == P[col]
    r, c = row[same], col[same]
    while True:
        nxt = label.copy()
        np.minimum.at(nxt, r, label[c])
        if (nxt == label).all():
            return label
        label = nxt


class Leiden(NamedTuple):
    cluster: np.ndarray
    level_labels: list
    refined_labels: list
    levels: list
    qnum_trace: list
    modularity: float
    resolution: Fraction
    M: int
    converged: bool


def leiden_graph(rowptr, col, w, resolution=1.0, max_sweeps=256, states=None) -> Leiden:
    """``states``, a list, collects per level a dict of the level's graph, ``comm0``, ``P`` and the refinement's sweep states."""
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.int64)
    frac = resolution_fraction(resolution)
    B = len(rowptr) - 1
    M = int(w.sum())
    guard(M, frac)
    isolated = np.diff(rowptr) == 0
    member = np.arange(B, dtype=np.int64)
    if M == 0:
        return Leiden(np.full(B, -1, np.int64), [member.copy()], [member.copy()],
                      [dict(vertices=B, communities=B, sweeps=0, fallback_moves=0, refined=B, refine_sweeps=0, refine_fallback_moves=0,
                            split=0)], [0], 0.0, frac, 0, True)
    row = _rows(rowptr)
    comm0 = np.arange(B, dtype=np.int64)
    trace, levels, level_labels, refined_labels, converged = None, [], [], [], True
    while True:
        n = len(rowptr) - 1
        deg = np.zeros(n, np.int64)
        np.add.at(deg, row, w)
        q = qnum(row, col, w, comm0, deg, M, frac)
        if trace is None:
            trace = [q]
        assert q == trace[-1], "the aggregation keeps Qnum"
        P, t, fallback, ok = move(row, col, w, comm0, deg, M, frac, trace, max_sweeps)
        converged &= ok
        sweeps = [] if states is not None else None
        ref, r, r_fallback, ok = refine(row, col, w, P, deg, M, frac, max_sweeps, sweeps)
        converged &= ok
        assert (P[ref] == P).all(), "ref nests in P"
        if states is not None:
            states.append(dict(rowptr=rowptr, row=row, col=col, w=w, deg=deg, comm0=comm0, P=P, ref=ref, sweeps=sweeps))
        inv, c_rowptr, c_col, c_w = aggregate(row, col, w, ref)
        nc = len(c_rowptr) - 1
        dense_P = np.unique(P, return_inverse=True)[1].astype(np.int64)
        levels.append(dict(vertices=n, communities=int(dense_P.max()) + 1, sweeps=t, fallback_moves=fallback, refined=nc,
                           refine_sweeps=r, refine_fallback_moves=r_fallback))
        level_labels.append(dense_P[member])
        refined_labels.append(inv[member])
        if nc == n:
            break
        lowest = np.full(n, nc, np.int64)                  # per P-community: the lowest dense id of its refined communities
        np.minimum.at(lowest, P, inv)
        comm0 = np.zeros(nc, np.int64)
        comm0[inv] = lowest[P]
        member = inv[member]
        rowptr, col, w = c_rowptr, c_col, c_w
        row = _rows(rowptr)
    # the final cut: the last P, every community split into its connected components
    parts = components(row, col, P)
    split = len(np.unique(parts)) - len(np.unique(P))
    levels[-1]["split"] = split
    if split:
        q = qnum(row, col, w, parts, deg, M, frac)
        assert q > trace[-1], "a split into components raises Qnum"
        trace.append(q)
        level_labels.append(np.unique(parts, return_inverse=True)[1].astype(np.int64)[member])
    return Leiden(final_clusters(level_labels[-1], isolated), level_labels, refined_labels, levels, trace,
                  trace[-1] / (frac.denominator * M * M), frac, M, converged)


def recipe_graph(n, seed):
    """The random weighted graph of the issue's recipe as a symmetric CSR ``(rowptr, col, w)``."""
    rng = np.random.default_rng(seed * 100 + n)
    p = rng.choice([0.1, 0.15, 0.25])
    U = np.triu(rng.random((n, n)) < p, 1)
    W = np.where(U, rng.integers(1, 6, (n, n)), 0)
    W = W + W.T
    return dense_csr(W)


def dense_csr(W):
    W = np.asarray(W, np.int64)
    r, c = np.nonzero(W)
    rowptr = np.zeros(len(W) + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=len(W)), out=rowptr[1:])
    return rowptr, c.astype(np.int32), W[r, c].astype(np.int32)


def edges_csr(n, edges):
    W = np.zeros((n, n), np.int64)
    for i, j, x in edges:
        W[i, j] = W[j, i] = x
    return dense_csr(W)


def disconnected(rowptr, col, label):
    """How many communities of ``label`` (ids >= 0) have a disconnected induced subgraph."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rowptr, col, label = np.asarray(rowptr), np.asarray(col), np.asarray(label)
    n = len(label)
    row = _rows(rowptr)
    keep = label[row] == label[col]
    g = csr_matrix((np.ones(int(keep.sum())), (row[keep], col[keep])), shape=(n, n))
    _, part = connected_components(g, directed=False)
    on = label >= 0
    pairs = np.unique(np.stack([label[on], part[on]]), axis=1)
    return int((np.bincount(pairs[0]) > 1).sum())
