"""numpy restatement of ``wgnn_silhouette_rows`` (``include/wgnn.h``), a plain fp64 silhouette beside it, the error bound and the
fixtures of the silhouette tests.

The restatement (``silhouette``): the squared distances exact in fp64 (``knn_reference.sq_distances``) ROUNDED TO float32 - the
kernel's chain gives these very bits wherever the distances are exact in float32, as on the lattice and on ``blobs`` - then
``np.sqrt`` in float32 (correctly rounded, as the kernel's ``sqrtf``), widened to fp64 and added in the kernel's order: the
member at position ``p`` of its group (members by ascending row) goes to partial ``(p % 64) // 4``, every partial is summed
sequentially in ``p`` from 0.0 (``np.cumsum`` adds sequentially), the 16 partials meet as a balanced tree over the xor offsets
1, 2, 4, 8.  ``a = S_own / (n_g - 1)`` (0 for a singleton), ``b`` the lowest ``S / n_c`` over the other non-empty groups, of equal
means the lower id (``np.argmin`` takes the first), ``score = (b - a) / max(a, b)``; 0 for a singleton and where ``max(a, b) ==
0``; with no other non-empty group ``b = +inf``, ``nearest = -1``, ``score = NaN``.  A row outside ``[0, K)`` or with a non-finite
value takes no part: NaN / NaN / NaN / -1.

``plain`` is the same definition with fp64 square roots and ``np.sum``.

The bound.  Against the exact distance the f32 chain errs by ``gamma(D) = (D + 3) u`` relative (knn_reference), the square root
halves that and adds its own rounding: a distance, and with it every mean of distances (non-negative terms; the fp64 additions
add 2^-53 each), is off by at most ``e = ((D + 3) / 2 + 1) u`` relative, ``u = 2^-24``.  ``(b - a) / max(a, b)`` with ``a`` and
``b`` each off by ``e`` relative moves by at most ``2 e / (1 - e)`` plus the quotient's share, below ``4 e``: ``bound(D)``."""
import functools

import numpy as np

import kmeans_reference as M
import knn_reference as R

TILE, LANE = 64, 4


def bound(D: int) -> float:
    return 4.0 * ((D + 3) / 2.0 + 1.0) * R.U


def lattice_groups() -> np.ndarray:
    """The grouping of ``test_gpu_kmeans_rows._lattice_groups``: 197 cells in 7 groups - group 0 holds 100 cells (two candidate
    tiles, the second partial), 1 is empty, 2 a singleton, 3..6 share 89 cells, 7 cells take no part (-1)."""
    perm = np.random.default_rng(5).permutation(R.LATTICE_N)
    g = np.full(R.LATTICE_N, -1, np.int64)
    g[perm[:100]] = 0
    g[perm[100]] = 2
    g[perm[101:190]] = 3 + np.arange(89) % 4
    g.setflags(write=False)
    return g


def real_groups(N: int) -> np.ndarray:
    """``default_rng(1).integers(-1, 4, N)``: groups 0..3 and some cells at -1."""
    g = np.random.default_rng(1).integers(-1, 4, N)
    g.setflags(write=False)
    return g


def participants(x: np.ndarray, group: np.ndarray, K: int) -> np.ndarray:
    g = np.asarray(group, np.int64)
    return np.isfinite(x).all(axis=1) & (g >= 0) & (g < K)


def group_sums(d: np.ndarray, members: np.ndarray, ordered: bool) -> np.ndarray:
    """float64 [n]: the sum over ``members`` (ascending rows) of the columns of ``d``, in the kernel's order when ``ordered``."""
    if not ordered:
        return d[:, members].sum(axis=1)
    p = np.arange(members.size)
    partial = np.zeros((d.shape[0], TILE // LANE), np.float64)
    for u in range(TILE // LANE):
        cols = members[(p % TILE) // LANE == u]
        if cols.size:
            partial[:, u] = np.cumsum(d[:, cols], axis=1)[:, -1]
    lanes = np.arange(TILE // LANE)
    for off in (1, 2, 4, 8):
        partial = partial + partial[:, lanes ^ off]
    return partial[:, 0]


def _means(x: np.ndarray, group: np.ndarray, K: int, ordered: bool):
    """``(on bool [n], g int64 [n], size int64 [K], mean f64 [n, K], own f64 [n])``: who takes part, their groups, and per row
    the mean distance to every non-empty group (+inf for an empty one) and the SUM over its own group."""
    n = x.shape[0]
    on = participants(x, group, K)
    g = np.where(on, np.asarray(group, np.int64), -1)
    rows = np.where(on[:, None], x, 0)
    d2 = R.sq_distances(rows, rows)
    d = np.sqrt(d2.astype(np.float32)).astype(np.float64) if ordered else np.sqrt(d2)
    size = np.bincount(g[on], minlength=K).astype(np.int64)
    mean = np.full((n, K), np.inf)
    own = np.zeros(n)
    for c in range(K):
        members = np.nonzero(g == c)[0]
        if members.size:
            S = group_sums(d, members, ordered)
            mean[:, c] = S / float(members.size)
            own[members] = S[members]
    return on, g, size, mean, own


def _silhouette(x: np.ndarray, group: np.ndarray, K: int, ordered: bool):
    n = x.shape[0]
    on, g, size, others, own = _means(x, group, K, ordered)
    others[on, g[on]] = np.inf
    nearest = np.where(np.isinf(others).all(axis=1), -1, np.argmin(others, axis=1))
    b = np.where(nearest >= 0, others[np.arange(n), np.maximum(nearest, 0)], np.inf)
    n_g = size[np.maximum(g, 0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(n_g > 1, own / (n_g - 1.0), 0.0)
        top = np.maximum(a, b)
        s = np.where(nearest < 0, np.nan, np.where((n_g <= 1) | (top == 0), 0.0, (b - a) / top))
    return np.where(on, a, np.nan), np.where(on, b, np.nan), np.where(on, s, np.nan), np.where(on, nearest, -1).astype(np.int32), size


def silhouette(x, group, K):
    """``(a f64 [n], b f64 [n], score f64 [n], nearest int32 [n], size int64 [K])`` as ``wgnn_silhouette_rows`` defines them, in
    the caller's row order."""
    return _silhouette(np.asarray(x, np.float32), group, K, True)


def plain(x, group, K):
    """The same definition in plain fp64: exact differences, fp64 square roots, ``np.sum``."""
    return _silhouette(np.asarray(x), group, K, False)


def two_lowest_gap(x, group, K) -> np.ndarray:
    """float64 [n]: ``(m2 - m1) / m2`` of the plain reference's two lowest other-group means (inf with fewer than two)."""
    on, g, _, others, _ = _means(np.asarray(x), group, K, False)
    others[on, g[on]] = np.inf
    if K < 2:
        return np.full(others.shape[0], np.inf)
    two = np.sort(others, axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isinf(two[:, 1]), np.inf, np.where(two[:, 1] == 0, 0.0, (two[:, 1] - two[:, 0]) / two[:, 1]))


@functools.lru_cache(maxsize=None)
def reference(name: str, *case):
    """The restatement of a fixture (computed once): ``reference("lattice", 36)`` with ``lattice_groups()`` and 7 groups,
    ``reference("blobs", 36)`` with the reference k-means labels (K = 5, seed 0)."""
    if name == "lattice":
        out = silhouette(R.lattice(*case), lattice_groups(), 7)
    else:
        out = silhouette(M.blobs(*case), M.reference("blobs", 5, 0, *case)["label"], 5)
    for v in out:
        v.setflags(write=False)
    return out
