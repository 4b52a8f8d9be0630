"""A numpy restatement of the diffusion operator, the Lanczos iteration on it, the Ritz vectors and the diffusion distance
(``include/wgnn.h``: wgnn_diffusion_degree, wgnn_diffusion_weights, wgnn_lanczos_init / apply / dots / update / scale,
wgnn_basis_combine, wgnn_diffusion_distance; ``ops.diffusion_operator`` / ``ops.lanczos_graph`` / ``ops.basis_combine`` /
``ops.diffusion_distance``), and the fixtures of their tests.  float64 throughout, every operation a numpy operation of its own
(so none is fused), the sums in the contract's order: a row sum lane by lane - ``np.add.at`` adds in index order, once per lane
class - with the sixteen partials folded by halves; a dot chunk by chunk, the fold by halves a reshape and slice-adds, the chunks'
values added in ascending order.  The one host step, ``lanczos_ritz``, is the package's own function (the contract says so)."""
from typing import NamedTuple

import numpy as np

from scdeepsort_amd.ops import lanczos_ritz
from louvain_reference import blobs
from umap_reference import U, csr_of, fuzzy_graph, knn, mix64

LANES, CHUNK = 16, 256
BREAKDOWN = 2.0 ** -26
D = np.float64


def _rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def row_sum(rowptr, terms):
    """The row sums of ``terms`` float64 [nnz]: lane ``l`` adds the row's entries ``l, l + 16, ...`` in order from +0.0, the
    partials fold 8, 4, 2, 1."""
    rowptr, terms = np.asarray(rowptr, np.int64), np.asarray(terms, D)
    row = _rows(rowptr)
    lane = (np.arange(len(terms), dtype=np.int64) - rowptr[row]) % LANES
    p = np.zeros((len(rowptr) - 1, LANES), D)
    np.add.at(p, (row, lane), terms)
    for half in (8, 4, 2, 1):
        p = p[:, :half] + p[:, half:2 * half]
    return p[:, 0]


class Operator(NamedTuple):
    t: np.ndarray
    q: np.ndarray
    z: np.ndarray


def diffusion_operator(rowptr, col, w) -> Operator:
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.float32)
    row, wd, on = _rows(rowptr), w.astype(D), w != 0
    q = row_sum(rowptr, wd)
    with np.errstate(all="ignore"):
        K = np.where(on, wd / (q[row] * q[col]), 0.0)
        z = np.sqrt(row_sum(rowptr, K))
        t = np.where(on, K / (z[row] * z[col]), 0.0)
    return Operator(t, q, z)


def lanczos_init(z, mask, seed):
    """``(w0, w1)``: ``z`` and the hash in [-1, 1), both zero outside ``mask``."""
    key = mix64(np.array([(int(seed) << 32) | 0xFFFFFFFE], U))[0]
    with np.errstate(over="ignore"):
        h = mix64(key + np.arange(len(z), dtype=U))
    u = ((h >> U(11)).astype(D) * D(2.0 ** -53)) * D(2.0) - D(1.0)
    return np.where(mask, np.asarray(z, D), 0.0), np.where(mask, u, 0.0)


def apply(rowptr, col, t, x):
    return row_sum(rowptr, np.asarray(t, D) * np.asarray(x, D)[np.asarray(col, np.int64)])


def dots(V, w):
    """``c[r] = V[r] . w``: per chunk of 256 the rounded products (+0.0 past the end) fold by halves, the chunks add in order."""
    V, w = np.atleast_2d(np.asarray(V, D)), np.asarray(w, D)
    n = len(w)
    n_chunks = (n + CHUNK - 1) // CHUNK
    p = np.zeros((V.shape[0], n_chunks * CHUNK), D)
    p[:, :n] = V * w[None, :]
    p = p.reshape(V.shape[0], n_chunks, CHUNK)
    half = CHUNK // 2
    while half >= 1:
        p = p[:, :, :half] + p[:, :, half:2 * half]
        half //= 2
    c = np.zeros(V.shape[0], D)
    for ch in range(n_chunks):
        c = c + p[:, ch, 0]
    return c


def norm(w):
    return np.sqrt(dots(w, w)[0])


def update(V, c, w):
    w = np.array(w, D)
    for r in range(len(c)):
        w = w - V[r] * c[r]
    return w


class Lanczos(NamedTuple):
    V: np.ndarray
    alpha: np.ndarray
    beta: np.ndarray
    n_run: int
    breakdown: bool
    n_cells: int


def _ortho(V, w):
    """classical Gram-Schmidt twice: ``(w, the first pass's coefficients)``."""
    c = dots(V, w)
    w = update(V, c, w)
    return update(V, dots(V, w), w), c


def lanczos_graph(rowptr, col, t, z, mask, n_steps, seed=0) -> Lanczos:
    mask = np.asarray(mask, bool)
    B, n_c = len(mask), int(mask.sum())
    m = max(0, min(int(n_steps), n_c - 1))
    V, alpha, beta = np.zeros((m + 1, B), D), np.zeros(m, D), np.zeros(m, D)
    if n_c == 0:
        return Lanczos(V, alpha, beta, 0, False, 0)
    w0, w1 = lanczos_init(z, mask, seed)
    with np.errstate(all="ignore"):
        b = norm(w0)
        if not b > BREAKDOWN:
            return Lanczos(V, alpha, beta, 0, True, n_c)
        V[0] = w0 / b
        if m >= 1:
            w1, _ = _ortho(V[:1], w1)
            b = norm(w1)
            if not b > BREAKDOWN:
                return Lanczos(V, alpha, beta, 0, True, n_c)
            V[1] = w1 / b
        for j in range(1, m + 1):
            w, c = _ortho(V[:j + 1], apply(rowptr, col, t, V[j]))
            alpha[j - 1], beta[j - 1] = c[j], norm(w)
            if not beta[j - 1] > BREAKDOWN:
                return Lanczos(V, alpha, beta, j, True, n_c)
            if j < m:
                V[j + 1] = w / beta[j - 1]
    return Lanczos(V, alpha, beta, m, False, n_c)


def basis_combine(V, S):
    """``Y`` [B, 1 + n_cols]: column 0 is ``V[0]``, the others the sums over ``j`` ascending, their sign fixed so that the entry
    of largest magnitude (the lowest cell among equal ones) is positive."""
    V, S = np.asarray(V, D), np.asarray(S, D)
    m, n_cols = S.shape
    Y = np.zeros((V.shape[1], n_cols + 1), D)
    Y[:, 0] = V[0]
    for j in range(1, m + 1):
        Y[:, 1:] = Y[:, 1:] + V[j][:, None] * S[j - 1][None, :]
    if Y.shape[0] and n_cols:
        first = np.abs(Y[:, 1:]).argmax(axis=0)                                # the first of equal maxima
        Y[:, 1:] = Y[:, 1:] * np.where(Y[first, np.arange(1, n_cols + 1)] < 0, -1.0, 1.0)
    return Y


def diffusion_weights(eigenvalues):
    with np.errstate(all="ignore"):
        lam = np.asarray(eigenvalues, D)
        g = lam / (1.0 - lam)
    g[0] = 0.0                                                                  # the stationary component is not read
    return g


def diffusion_distance(Y, g, roots):
    Y, g = np.asarray(Y, D), np.asarray(g, D)
    best = np.full(len(Y), np.inf)
    with np.errstate(all="ignore"):
        for r in np.unique(np.atleast_1d(np.asarray(roots, np.int64))):
            s = np.zeros(len(Y), D)
            for l in range(1, len(g)):
                p = g[l] * (Y[r, l] - Y[:, l])
                s = s + p * p
            d = np.sqrt(s)
            best = np.where((d < best) | np.isnan(d), d, best)
    return best


def components(rowptr, col):
    """int64 [B]: the lowest vertex of every vertex's connected component."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    B = len(rowptr) - 1
    _, lab = connected_components(sp.csr_matrix((np.ones(len(col)), np.asarray(col, np.int64), np.asarray(rowptr, np.int64)), shape=(B, B)),
                                  directed=False)
    lowest = np.full(lab.max() + 1 if B else 0, B, np.int64)
    np.minimum.at(lowest, lab, np.arange(B))
    return lowest[lab]


def largest_component(rowptr, col):
    """``(mask, n_components)``: the largest component, ties in size to the one that holds the lowest cell."""
    comp = components(rowptr, col)
    size = np.bincount(comp, minlength=len(comp))
    return comp == int(np.argmax(size)), int((size > 0).sum())


class Diffmap(NamedTuple):
    Y: np.ndarray
    eigenvalues: np.ndarray
    residual: np.ndarray
    run: Lanczos
    op: Operator
    mask: np.ndarray
    n_components: int


def diffmap(rowptr, col, w, n_comps=15, n_steps=128, seed=0) -> Diffmap:
    """``api.ResidentPredictor.diffmap``'s composition from the graph on."""
    mask, n_components = largest_component(rowptr, col)
    op = diffusion_operator(rowptr, col, w)
    run = lanczos_graph(rowptr, col, op.t, op.z, mask, n_steps, seed)
    theta, S, res = lanczos_ritz(run.alpha, run.beta, run.n_run)
    n_found = min(int(n_comps), run.n_run + 1)
    Y = basis_combine(run.V, S[:, :n_found - 1])
    return Diffmap(Y, np.concatenate([[1.0], theta[:n_found - 1]]), np.concatenate([[0.0], res[:n_found - 1]]), run, op, mask,
                   n_components)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
def path_graph(n=5):
    return csr_of(n, [(v, v + 1) for v in range(n - 1)])


def complete_graph(n=8):
    return csr_of(n, [(a, b) for a in range(n) for b in range(a + 1, n)])


def hand_graph():
    """Twelve vertices: a ring 0 - 6 with two chords, a triangle 8 - 10 hanging on it by a ZERO-weight edge (so the structure
    connects what the weights do not), vertex 7 isolated, vertex 11 a leaf of 10."""
    edges = [(v, (v + 1) % 7) for v in range(7)] + [(0, 3), (2, 5), (8, 9), (9, 10), (8, 10), (10, 11), (6, 8)]
    weights = [1.0, 0.5, 0.25, 0.75, 1.0, 0.125, 0.5, 0.3, 0.7, 1.0, 0.6, 0.9, 0.45, 0.0]
    return csr_of(12, edges, weights)


def arc(n=800, k=15, seed=7):
    """``n`` points ``(4 cos 3s, 4 sin 3s, 0) + 0.15 N(0, 1)`` with ``s`` sorted uniform (tests/geodesic_reference.py's curve) and
    the fuzzy graph of their ``k`` nearest neighbours: ``(s, Fuzzy)``."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.uniform(size=n))
    x = np.stack([4 * np.cos(3 * s), 4 * np.sin(3 * s), np.zeros(n)], axis=1) + 0.15 * rng.normal(size=(n, 3))
    return s, fuzzy_graph(*knn(x.astype(np.float32), k))


def blob_cells(n=2000, k=15, seed=11):
    """The fuzzy graph of ``n`` cells of eight well-separated blobs in six dimensions: the graph falls into components (seven
    with these arguments, the largest 516 cells - two blobs that touch)."""
    return fuzzy_graph(*knn(blobs(n, 6, 8, 12.0, seed=seed), k))


def two_parts(n=140, k=6):
    """Two blobs far apart - two components, the second the larger - as one fuzzy graph."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(size=(n // 2 - 10, 4)), 40.0 + rng.normal(size=(n // 2 + 10, 4))]).astype(np.float32)
    return fuzzy_graph(*knn(x, k))


def spearman(a, b):
    rank = lambda v: np.argsort(np.argsort(v, kind="stable"), kind="stable").astype(D)
    ra, rb = rank(a), rank(b)
    return float(np.corrcoef(ra, rb)[0, 1])
