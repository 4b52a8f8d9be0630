"""A numpy restatement of the geodesic rounds and the group-edge tables (``include/wgnn.h``: wgnn_geodesic_round;
``ops.distance_graph`` / ``ops.geodesic_rows`` / ``ops.group_edges``; ``tables._paga_connectivities``), and the fixtures of their
tests.  float32 where the contract says float32 - a candidate is ONE numpy float32 add - and Python integers / ``Fraction`` for the
PAGA tables, so that the fp64 figures are checked against exact rationals.  A run is restated round by round: ``states=`` collects
the state after every round.  Nothing here imports the package."""
import heapq
from fractions import Fraction
from typing import NamedTuple

import numpy as np

F = np.float32
INF = F(np.inf)


# ---------------------------------------------------------------------------------------------------------------------------
def csr_from_edges(n, edges):
    """``(rowptr int64 [n + 1], col int32, length float32)``: undirected edges ``(u, v, length)`` stored in both directions,
    columns ascending within a row."""
    rows = [[] for _ in range(n)]
    for u, v, w in edges:
        rows[u].append((v, w))
        rows[v].append((u, w))
    rowptr, col, length = [0], [], []
    for r in rows:
        for v, w in sorted(r):
            col.append(v)
            length.append(w)
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int32), np.asarray(length, F)


def knn_lists(x, k):
    """Exact k nearest neighbours by ascending (squared distance, index), the row itself left out: ``(idx int64 [B, k], d2 float32
    [B, k])``.  The squared distance is the float64 sum of squared differences rounded to float32: ``d2(i, j)`` and ``d2(j, i)`` are
    the same bits, as ``knn_rows`` promises of its own."""
    x = np.asarray(x, np.float64)
    B = len(x)
    d2 = np.empty((B, B), np.float64)
    for r0 in range(0, B, 128):
        d2[r0:r0 + 128] = ((x[r0:r0 + 128, None, :] - x[None, :, :]) ** 2).sum(-1)
    d2 = np.minimum(d2, d2.T).astype(F)                    # pairwise sums may differ in the last bit: one value per pair
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)
    return idx, np.take_along_axis(d2, idx, axis=1)


def distance_graph(idx, d2):
    """``(rowptr int64 [B + 1], col int32, length float32)``: the symmetric union CSR of the lists, ``length = sqrt(d2)`` in float32
    (numpy's is correctly rounded) of the listed direction - the smaller where both are listed and differ."""
    idx, d2 = np.asarray(idx, np.int64), np.asarray(d2, F)
    B, k = idx.shape
    src = np.repeat(np.arange(B, dtype=np.int64), k)
    dst = idx.ravel()
    ok = (dst >= 0) & (dst != src)
    src, dst, root = src[ok], dst[ok], np.sqrt(d2.ravel()[ok])
    assert root.dtype == F
    keys, inv = np.unique(np.concatenate([src * B + dst, dst * B + src]), return_inverse=True)
    length = np.full(len(keys), INF, F)
    np.minimum.at(length, inv, np.concatenate([root, root]))
    rowptr = np.zeros(B + 1, np.int64)
    np.cumsum(np.bincount(keys // B, minlength=B), out=rowptr[1:])
    return rowptr, (keys % B).astype(np.int32), length


# ---------------------------------------------------------------------------------------------------------------------------
def geodesic_round(rowptr, col, length, dist, pred):
    """One round on the state ``(dist float32, pred int32)``: ``(dist', pred', changed)``.  Every vertex takes the least
    ``(dist[u] + length(u, v), u)`` over its stored neighbours with a finite ``dist[u]`` when that candidate is strictly below
    ``dist[v]``."""
    rowptr, col, length = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(length, F)
    dist, pred = np.asarray(dist, F), np.asarray(pred, np.int32)
    n = len(dist)
    out_d, out_p = dist.copy(), pred.copy()
    if len(col) == 0:
        return out_d, out_p, 0
    du = dist[col]
    with np.errstate(over="ignore"):
        cand = np.where(np.isfinite(du), du + length, INF)              # one float32 add per stored entry
    assert cand.dtype == F
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    order = np.lexsort((col, cand, row))                               # per row: ascending (cand, u)
    first = np.flatnonzero(np.concatenate([[True], row[order][1:] != row[order][:-1]]))
    v, best, u = row[order][first], cand[order][first], col[order][first]
    better = best < dist[v]
    out_d[v[better]] = best[better]
    out_p[v[better]] = u[better]
    return out_d, out_p, int(better.sum())


class Geodesic(NamedTuple):
    dist: np.ndarray
    pred: np.ndarray
    rounds: int               # the rounds that changed something
    converged: bool           # a round that changed nothing was run
    reached: int


def start_state(n, roots):
    roots = np.unique(np.atleast_1d(np.asarray(roots, np.int64)))
    if roots.size == 0 or roots[0] < 0 or roots[-1] >= n:
        raise ValueError("roots")
    dist = np.full(n, INF, F)
    dist[roots] = 0
    return dist, np.full(n, -1, np.int32)


def geodesic_rows(rowptr, col, length, roots, max_rounds=None, states=None) -> Geodesic:
    """The run: rounds from the roots' state until one changes nothing, at most ``max_rounds`` (None = n) of them.  ``states``: a list
    that receives ``(dist, pred, changed)`` after every round run."""
    n = len(rowptr) - 1
    dist, pred = start_state(n, roots)
    max_rounds = n if max_rounds is None else int(max_rounds)
    rounds, converged = 0, n == 0
    for _ in range(max_rounds):
        dist, pred, changed = geodesic_round(rowptr, col, length, dist, pred)
        if states is not None:
            states.append((dist.copy(), pred.copy(), changed))
        if changed == 0:
            converged = True
            break
        rounds += 1
    return Geodesic(dist, pred, rounds, converged, int(np.isfinite(dist).sum()))


def dijkstra_f32(rowptr, col, length, roots):
    """A heap Dijkstra whose every add is a float32 add: float32 [n].  Rounding is monotone, so the labels it settles are the
    least float32 path sums - the fixed point of the rounds."""
    n = len(rowptr) - 1
    dist, _ = start_state(n, roots)
    heap = [(0.0, int(r)) for r in np.flatnonzero(dist == 0)]
    heapq.heapify(heap)
    done = np.zeros(n, bool)
    with np.errstate(over="ignore"):
        while heap:
            d, u = heapq.heappop(heap)
            if done[u] or F(d) != dist[u]:
                continue
            done[u] = True
            for e in range(rowptr[u], rowptr[u + 1]):
                v, cand = int(col[e]), dist[u] + length[e]
                if cand < dist[v]:
                    dist[v] = cand
                    heapq.heappush(heap, (float(cand), v))
    return dist


def hops(pred, dist):
    """Edges on every vertex' path to its root (0 at a root, -1 where not reached), walked one vertex at a time."""
    out = np.full(len(pred), -1, np.int64)
    for v in range(len(pred)):
        if np.isfinite(dist[v]):
            h, u = 0, v
            while pred[u] >= 0:
                h, u = h + 1, pred[u]
            out[v] = h
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def group_edges(idx, group, K):
    """``(edges int64 [K, K], size int64 [K])``: the directed list entries counted by the groups of their two ends, one entry at a
    time; an end at -1 does not count."""
    idx, group = np.asarray(idx, np.int64), np.asarray(group, np.int64)
    edges, size = np.zeros((K, K), np.int64), np.zeros(K, np.int64)
    for i in range(len(group)):
        if group[i] >= 0:
            size[group[i]] += 1
        for j in idx[i]:
            if j >= 0 and group[i] >= 0 and group[j] >= 0:
                edges[group[i], group[j]] += 1
    return edges, size


def paga(edges, size):
    """``(out_edges, expected, connectivities)`` from exact rationals: the expected count ``(es[a] ns[b] + es[b] ns[a]) / (n - 1)``
    and the connectivity ``min(1, inter (n - 1) / den)`` (0 where ``inter == 0``), each rounded to float64 once."""
    K = len(size)
    e = [[int(edges[a][b]) for b in range(K)] for a in range(K)]
    ns = [int(s) for s in size]
    es, n = [sum(r) for r in e], sum(ns)
    expected, conn = np.zeros((K, K)), np.zeros((K, K))
    for a in range(K):
        for b in range(K):
            if a == b or n < 2:
                continue
            den, inter = es[a] * ns[b] + es[b] * ns[a], e[a][b] + e[b][a]
            expected[a, b] = float(Fraction(den, n - 1))
            if inter:
                conn[a, b] = float(min(Fraction(1), Fraction(inter * (n - 1), den)))
    return np.asarray(es, np.int64), expected, conn


# ---------------------------------------------------------------------------------------------------------------------------
# Hand graphs: (vertices, undirected edges, root(s)); the expected figures are in tests/test_geodesic_reference.py
T24 = 2.0 ** -24
HAND = {
    "detour": (6, [(0, 1, 4), (0, 2, 1), (2, 3, 1), (3, 1, 1), (1, 4, .5)], 0),
    "ties": (6, [(0, 5, 1), (5, 3, 1), (0, 1, .5), (1, 2, .5), (2, 3, 1), (3, 4, 1)], 0),
    "rounding": (4, [(0, 1, .5), (1, 3, .5 + T24), (0, 2, 1), (2, 3, .75 * T24)], 0),
    "chain": (300, [(v, v + 1, .25) for v in range(299)], 0),
    "chain2": (300, [(v, v + 1, .25) for v in range(299)], [0, 299]),
    "square": (4, [(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)], 0),
    "edgeless": (5, [], 2),
}


def hand(name):
    n, edges, roots = HAND[name]
    return csr_from_edges(n, edges) + (roots,)


def star(n_leaves=300):
    """A hub (vertex 0) with ``n_leaves`` edges of lengths 1 + (leaf % 7) / 8 and a second ring of edges between consecutive leaves
    of length 1/16: the hub's row is longer than one pass of sixteen lanes.  Root: the last leaf."""
    edges = [(0, v, 1 + (v % 7) / 8) for v in range(1, n_leaves + 1)] + [(v, v + 1, 1 / 16) for v in range(1, n_leaves, 3)]
    return csr_from_edges(n_leaves + 1, edges) + (n_leaves,)


def gaussian(B, D, k, seed):
    """kNN graph of ``B`` Gaussian rows in ``D`` dimensions: ``(idx, d2)``."""
    return knn_lists(np.random.default_rng(seed).normal(size=(B, D)).astype(F), k)


def duplicates(B=120, D=4, k=6, seed=3):
    """Gaussian rows of which every third repeats its predecessor: zero lengths, and equal candidates decided by the lower id."""
    x = np.random.default_rng(seed).normal(size=(B, D)).astype(F)
    x[2::3] = x[1::3][:len(x[2::3])]
    return knn_lists(x, k)


def arc(n=800, k=8, seed=7):
    """``n`` points ``(4 cos 3s, 4 sin 3s, 0) + 0.15 N(0, 1)`` with ``s`` sorted uniform: ``(s, idx, d2)`` - a curve, root at 0."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.uniform(size=n))
    x = np.stack([4 * np.cos(3 * s), 4 * np.sin(3 * s), np.zeros(n)], axis=1) + 0.15 * rng.normal(size=(n, 3))
    return (s,) + knn_lists(x.astype(F), k)
