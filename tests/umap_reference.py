"""A numpy restatement of the fuzzy kNN graph and the synchronous 2-D layout (``include/wgnn.h``: wgnn_fuzzy_rows, wgnn_fuzzy_union,
wgnn_layout_init, wgnn_layout_epoch; ``ops.fuzzy_graph`` / ``ops.layout_graph``), and the fixtures of their tests.  float32 where
the contract says float32 (every operation a numpy operation of its own, so none is fused), float64 where it says float64, the sums
in the contract's order: a row's ``p`` is added up entry by entry, a vertex's force lane by lane - ``np.add.at`` adds in index
order, once per lane class - and the sixteen partials fold by halves.  Nothing here imports the package."""
import math
from typing import NamedTuple

import numpy as np

from louvain_reference import blobs, snn_graph

F = np.float32
LANES = 16
U = np.uint64


def mix64(x):
    """The splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)."""
    x = np.asarray(x, U) + U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def epoch_key(seed, epoch):
    return mix64(np.array([(int(seed) << 32) | int(epoch)], U))[0]


# ---------------------------------------------------------------------------------------------------------------------------
def _listed(idx, d2):
    return (np.asarray(idx) >= 0) & np.isfinite(d2)


def _ordered_sum(v):
    out = np.zeros(v.shape[0], np.float64)
    for j in range(v.shape[1]):
        out = out + v[:, j]
    return out


def _terms(listed, x, s):
    with np.errstate(all="ignore"):
        return np.where(listed, np.where(x > 0, np.exp(-x / s[:, None]), 1.0), 0.0)


class FuzzyRows(NamedTuple):
    rho: np.ndarray
    sigma: np.ndarray
    member: np.ndarray
    floored: np.ndarray           # sigma is the floor 1e-3 * mean
    constant: np.ndarray          # every listed distance equals rho (or is 0): every member is exactly 1


def fuzzy_rows(idx, d2) -> FuzzyRows:
    d2 = np.asarray(d2, F)
    n, k = d2.shape
    listed = _listed(idx, d2)
    d = np.sqrt(np.where(listed, d2, F(0)).astype(F)).astype(np.float64)
    positive = listed & (d > 0)
    rho = np.where(positive.any(1), np.where(positive, d, np.inf).min(1), 0.0)
    x = d - rho[:, None]
    count = listed.sum(1)
    target = math.log2(k + 1)
    lo, hi, s = np.zeros(n), np.full(n, np.inf), np.ones(n)
    with np.errstate(all="ignore"):
        for _ in range(64):
            up = _ordered_sum(_terms(listed, x, s)) > target
            hi = np.where(up, s, hi)
            lo = np.where(up, lo, s)
            s = np.where(np.isinf(hi), 2.0 * s, (lo + hi) / 2.0)
        floor = 1e-3 * (_ordered_sum(np.where(listed, d, 0.0)) / count)
    sigma = np.maximum(s, floor)
    member = _terms(listed, x, sigma).astype(F)
    empty = count == 0
    rho[empty], sigma[empty], member[empty] = 0.0, 0.0, 0.0
    return FuzzyRows(rho, sigma, member, ~empty & (floor >= s), ~empty & ~(listed & (x > 0)).any(1))


def fuzzy_residual(idx, d2, rho, sigma):
    """``|p(sigma) - log2(k + 1)|`` per row, in float64 (NaN for a row with nothing listed)."""
    d2 = np.asarray(d2, F)
    listed = _listed(idx, d2)
    d = np.sqrt(np.where(listed, d2, F(0)).astype(F)).astype(np.float64)
    with np.errstate(all="ignore"):
        p = _ordered_sum(_terms(listed, d - np.asarray(rho)[:, None], np.asarray(sigma, np.float64)))
    return np.where(listed.any(1), np.abs(p - math.log2(d2.shape[1] + 1)), np.nan)


def fuzzy_union(idx, member, rowptr, col):
    """``w`` float32 [nnz] of the union CSR: ``(a + b) - a * b`` of the two directions' memberships."""
    idx, member = np.asarray(idx, np.int64), np.asarray(member, F)
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    col = np.asarray(col, np.int64)

    def of(r, c):
        eq = idx[r] == c[:, None]
        return np.where(eq.any(1), member[r, eq.argmax(1)], F(0)).astype(F)

    a, b = of(row, col), of(col, row)
    return ((a + b) - a * b).astype(F)


class Fuzzy(NamedTuple):
    rowptr: np.ndarray
    col: np.ndarray
    w: np.ndarray
    rho: np.ndarray
    sigma: np.ndarray
    member: np.ndarray


def fuzzy_graph(idx, d2) -> Fuzzy:
    rowptr, col, _ = snn_graph(idx, "unit")
    rows = fuzzy_rows(idx, d2)
    return Fuzzy(rowptr, col, fuzzy_union(idx, rows.member, rowptr, col), rows.rho, rows.sigma, rows.member)


# ---------------------------------------------------------------------------------------------------------------------------
def layout_init(n, seed):
    h = mix64(epoch_key(seed, 0xFFFFFFFF) + np.arange(2 * n, dtype=U))
    return (((h >> U(40)).astype(F) * F(2.0 ** -24)) * F(20) - F(10)).reshape(n, 2)


def _clamp4(v):
    return np.where(v < F(-4), F(-4), np.where(v > F(4), F(4), v)).astype(F)


def _power(q, b):
    return q if b == F(1) else np.power(q.astype(np.float64), np.float64(b)).astype(F)


def layout_epoch(rowptr, col, w, wmax, y, epoch, n_epochs, a, b, gamma, alpha, n_neg, seed):
    """``(y_out, fired per vertex)`` of epoch ``epoch``; every argument as wgnn_layout_epoch takes it."""
    rowptr, col, w, y = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, F), np.asarray(y, F)
    a, b, gamma, alpha, wmax = F(a), F(b), F(gamma), F(alpha), F(wmax)
    n, nnz = len(rowptr) - 1, len(col)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    with np.errstate(all="ignore"):
        r = w / wmax
        fires = np.floor(F(epoch + 1) * r) != np.floor(F(epoch) * r)
        e = np.nonzero(fires)[0]
        i, j = row[e], col[e]
        terms = np.zeros((len(e), 1 + n_neg, 2), F)
        valid = np.zeros((len(e), 1 + n_neg), bool)
        pull, push = (F(-2) * a) * b, (F(2) * gamma) * b

        dx = y[i] - y[j]
        q = dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]
        qb = _power(q, b)
        c = ((pull * qb) / q) / (F(1) + a * qb)
        terms[:, 0], valid[:, 0] = _clamp4(c[:, None] * dx), q > 0
        key = epoch_key(seed, epoch)
        for s in range(n_neg):
            h = mix64(key + e.astype(U) * U(n_neg) + U(s))
            t = (((h >> U(32)) * U(n)) >> U(32)).astype(np.int64)
            dx = y[i] - y[t]
            q = dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]
            c = push / ((F(0.001) + q) * (F(1) + a * _power(q, b)))
            terms[:, 1 + s], valid[:, 1 + s] = _clamp4(c[:, None] * dx), (t != i) & (q > 0)
    lane = (e - rowptr[i]) % LANES
    partial = np.zeros((LANES, n, 2), F)
    at = np.broadcast_to(i[:, None], valid.shape)
    for l in range(LANES):
        sel = valid & (lane == l)[:, None]
        np.add.at(partial[l], at[sel], terms[sel])                  # in (edge, term) order: C order of the mask
    width = LANES
    while width > 1:
        width //= 2
        partial[:width] = partial[:width] + partial[width:2 * width]
    out = (y + alpha * partial[0]).astype(F)
    isolated = rowptr[1:] == rowptr[:-1]
    out[isolated] = y[isolated]
    return out, np.bincount(i, minlength=n).astype(np.int64)


class LayoutRun(NamedTuple):
    y: np.ndarray
    n_epochs: int
    n_fired: int


def layout_epochs(n):
    return 500 if n < 10000 else 200


def layout_graph(rowptr, col, w, init="hash", n_epochs=None, a=1.577, b=0.895, gamma=1.0, n_neg=5, lr=1.0, seed=0) -> LayoutRun:
    n = len(rowptr) - 1
    n_epochs = layout_epochs(n) if n_epochs is None else int(n_epochs)
    y = layout_init(n, seed) if isinstance(init, str) else np.array(init, F)
    w = np.asarray(w, F)
    if n == 0 or len(w) == 0 or not w.max() > 0:
        return LayoutRun(y, n_epochs, 0)
    fired = 0
    for t in range(n_epochs):
        y, f = layout_epoch(rowptr, col, w, w.max(), y, t, n_epochs, a, b, gamma, F(lr * (1.0 - t / n_epochs)), n_neg, seed)
        fired += int(f.sum())
    return LayoutRun(y, n_epochs, fired)


def pca_init(x):
    """The first two principal components of the rows, the sign of each fixed by its largest component, scaled to max-abs 10."""
    x = np.asarray(x, np.float64)
    x = x - x.mean(0)
    _, vec = np.linalg.eigh(x.T @ x / len(x))
    axes = vec[:, ::-1][:, :2]
    axes = axes * np.sign(axes[np.abs(axes).argmax(0), np.arange(2)])
    y = x @ axes
    return (y * (10.0 / np.abs(y).max())).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
def knn(x, k):
    """Exact k nearest rows under (squared distance, index), the row itself left out: ``(idx int64 [B, k], d2 float32 [B, k])``."""
    x = np.asarray(x, np.float64)
    sq = (x * x).sum(1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0).astype(F)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(d2, idx, 1)


def ragged_lists(n=70, k=15, seed=3):
    """``n`` cells of three blobs, ``k`` neighbours, and the cases of the contract: rows 0 - 3 are one point (zero distances, and for
    small k nothing positive), row 5's distances are all equal, rows 7 - 9 end in -1 / +inf tails, row 11 lists nobody."""
    x = blobs(n, 6, 3, 2.5, seed=seed)
    x[1:4] = x[0]
    idx, d2 = knn(x, k)
    d2[5] = d2[5, 0]
    for r, keep in ((7, max(k - 1, 0)), (8, max(k // 2, 0)), (9, min(1, k))):
        idx[r, keep:], d2[r, keep:] = -1, np.inf
    idx[11], d2[11] = -1, np.inf
    return idx, d2


def csr_of(n, edges, weights=None):
    """The symmetric CSR (``rowptr`` int64, ``col`` int32 ascending, ``w`` float32) of undirected ``edges``."""
    weights = [1.0] * len(edges) if weights is None else weights
    both = sorted({(a, b): x for (a, b), x in zip(edges, weights)}.items() | {(b, a): x for (a, b), x in zip(edges, weights)}.items())
    row = np.array([p[0][0] for p in both], np.int64)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, np.array([p[0][1] for p in both], np.int32), np.array([p[1] for p in both], F)


def star_graph(leaves=300, seed=0):
    """Vertex 0 joined to ``leaves`` others with weights in (0.2, 1]: a row far longer than the sixteen lanes."""
    w = np.random.default_rng(seed).uniform(0.2, 1.0, leaves).astype(F)
    w[0] = 1.0
    return csr_of(leaves + 1, [(0, v) for v in range(1, leaves + 1)], [float(v) for v in w])


def blob_graph(n, k, seed):
    idx, d2 = knn(blobs(n, 6, 4, 3.0, seed=seed), k)
    return fuzzy_graph(idx, d2)
